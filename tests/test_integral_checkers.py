"""The checker of tests/harness/integrals.py against lookup_accounts_at's checker summed tick by tick,
against the order-free form `opening * L + sum of effect * (t_end - t_r)` written out here, and against
get_account_statements' checker, before any GPU answer is held to it.  No GPU."""
import numpy as np
import pytest

from tests.harness.asof import AsOf
from tests.harness.balances import COLUMNS, MOD, PENDING, POST, VOID, balances_of, u128
from tests.harness.integrals import MOD192, Integrals, balances, ids_body, integrals, period_end
from tests.harness.oracle import OracleEngine
from tests.harness.statements import Statements, request_of, sweep_pairs
from tests.harness import statements
from tests.harness.workload import account_id, make_scenario
from tests.test_balance_checkers import QUERY_SCENARIO
from tigerbeetle_amd.state_machine import average_balances
from tigerbeetle_amd.types import INTEGRAL_DTYPE, U64_MAX

ABSENT = (account_id(5000), account_id(5001))


@pytest.fixture(scope="module")
def ledger():
    """The oracle's small scenario (tests/test_statement_checkers.py's), committed once; never changed."""
    sc = make_scenario(2025, **QUERY_SCENARIO)
    oracle = OracleEngine(4096, 1 << 15)
    for _, op, ts, events in sc.steps:
        oracle.commit(op, ts, b"".join(events))
    transfers, accounts = oracle.export_transfers(), oracle.export_accounts()
    commit_timestamp = oracle.commit_timestamp
    oracle.close()
    return dict(sc=sc, transfers=transfers, accounts=accounts, commit_timestamp=commit_timestamp,
                checker=Integrals(transfers, accounts, commit_timestamp), ids=request_of(accounts, ABSENT))


def weighted_form(transfers, accounts, account, t_open, t_end):
    """opening * L + the sum of effect(r) * (t_end - t_r) over the records in (t_open, t_end], modulo
    2^192, by a pass over the export; opening = current - every effect above t_open, modulo 2^128."""
    amounts = {u128(t, "id"): u128(t, "amount") for t in transfers}
    current = next(balances_of(a) for a in accounts if u128(a, "id") == account)
    above, weighted = [0, 0, 0, 0], [0, 0, 0, 0]
    for t in transfers:
        ts, kind, amount = int(t["timestamp"]), int(t["flags"]), u128(t, "amount")
        if ts <= t_open:
            continue
        if kind & PENDING:
            moved = (amount, 0)
        elif kind & POST:
            moved = (-amounts[u128(t, "pending_id")], amount)
        elif kind & VOID:
            moved = (-amount, 0)
        else:
            moved = (0, amount)
        for side, name in enumerate(("debit_account_id", "credit_account_id")):
            if u128(t, name) == account:
                for k in range(2):
                    above[2 * side + k] += moved[k]
                    if ts <= t_end:
                        weighted[2 * side + k] += moved[k] * (t_end - ts)
    opening = [(c - a) % MOD for c, a in zip(current, above)]
    return tuple((o * (t_end - t_open) + w) % MOD192 for o, w in zip(opening, weighted))


def test_integral_is_the_literal_sum_of_lookup_accounts_at(ledger):
    """Short periods (at most 200 ticks) that straddle a prepare's last timestamp, a post and a void:
    the integral is lookup_accounts_at's checker asked at every t of the period and summed."""
    transfers, accounts, checker = ledger["transfers"], ledger["accounts"], ledger["checker"]
    asof = AsOf(transfers, accounts)
    boundaries = [ts for _, op, ts, _ in ledger["sc"].steps if op == 129]
    post = next(t for t in transfers if int(t["flags"]) & POST and not int(t["flags"]) & PENDING)
    void = next(t for t in transfers if int(t["flags"]) & VOID)
    periods = [(boundaries[2] - 60, boundaries[2] + 40), (boundaries[5] - 150, boundaries[5] + 50), (boundaries[9] - 1, boundaries[9] + 1)]
    touched = 0
    for special in (post, void):
        ts = int(special["timestamp"])
        periods.append((ts - 30, ts + 25))
    for (t_open, t_end), special in zip(periods, (None, None, None, post, void)):
        ids = [u128(a, "id") for a in accounts[:4]]
        if special is not None:
            ids = list(dict.fromkeys([u128(special, "debit_account_id"), u128(special, "credit_account_id")] + ids[:1]))
        assert 0 < t_end - t_open <= 200
        rows, matched, orphan = checker.of(ids, t_open, t_end)
        assert matched == len(rows) == len(ids) and not orphan
        total = {i: [0, 0, 0, 0] for i in ids}
        for t in range(t_open, t_end):
            for rec in asof.at(ids, t)[0]:
                for c, v in enumerate(balances_of(rec)):
                    total[u128(rec, "id")][c] += v
        for row in rows:
            i = u128(row, "id")
            # (An account created inside the period is absent from the early answers: zero, as the definition gives.)
            assert integrals(row) == tuple(total[i]), (t_open, t_end, hex(i))
            assert (int(row["t_open"]), int(row["t_end"])) == (t_open, t_end)
            touched += balances(row, "opening") != balances(row, "closing")
    assert touched >= 6  # the periods hold records of the accounts asked


def test_integral_is_the_order_free_form_and_the_statements_ends(ledger):
    """Over sweep_pairs: opening * L + the weighted effects, opening and closing are Statements', the
    integrals add over a split, an empty period gives zeros."""
    transfers, accounts, checker, ids = ledger["transfers"], ledger["accounts"], ledger["checker"], ledger["ids"]
    commit_timestamp = ledger["commit_timestamp"]
    held = Statements(transfers, accounts)
    three = [u128(a, "id") for a in accounts[:3]]
    nonzero = pending_moves = 0
    for t_open, t_close in sweep_pairs(ledger["sc"].steps, transfers, commit_timestamp):
        rows, matched, orphan = checker.of(ids, t_open, t_close)
        t_end = period_end(t_open, t_close, commit_timestamp)
        if t_end is None:  # (commit_timestamp + 1, 0): the end is below the start
            assert t_close == 0 and t_open > commit_timestamp and matched == 0 and len(rows) == 0
            continue
        want, want_matched, _ = held.of(ids, t_open, t_end)
        assert matched == want_matched == len(rows) and not orphan
        for row, st in zip(rows, want):
            assert u128(row, "id") == u128(st, "id")
            assert balances(row, "opening") == statements.balances(st, "opening"), (t_open, t_close)
            assert balances(row, "closing") == statements.balances(st, "closing"), (t_open, t_close)
            if t_end == t_open:
                assert integrals(row) == (0, 0, 0, 0) and balances(row, "opening") == balances(row, "closing")
                assert average_balances(row) is None
            else:
                assert average_balances(row) == tuple(v // (t_end - t_open) for v in integrals(row))
            nonzero += any(integrals(row))
        for row in rows:
            if u128(row, "id") in three:
                got = weighted_form(transfers, accounts, u128(row, "id"), t_open, t_end)
                assert integrals(row) == got == checker.order_free(u128(row, "id"), t_open, t_end), (t_open, t_close, hex(u128(row, "id")))
                pending_moves += balances(row, "opening")[0] > balances(row, "closing")[0]  # holds released in the period
        # Additivity: I(t0, t2) = I(t0, t1) + I(t1, t2) modulo 2^192, at a split inside the period.
        if t_end - t_open >= 2:
            for t_mid in (t_open + 1, (t_open + t_end) // 2, t_end - 1):
                first = {u128(r, "id"): integrals(r) for r in checker.of(three, t_open, t_mid)[0]}
                second = {u128(r, "id"): integrals(r) for r in checker.of(three, t_mid, t_end)[0]}
                for row in checker.of(three, t_open, t_end)[0]:
                    i = u128(row, "id")
                    parts = tuple((a + b) % MOD192 for a, b in zip(first.get(i, (0, 0, 0, 0)), second[i]))
                    assert parts == integrals(row), (t_open, t_mid, t_end)
    assert nonzero > 500 and pending_moves > 0
    # t_close == 0 is t_close == commit_timestamp.
    assert checker.of(ids, 5, 0)[0].tobytes() == checker.of(ids, 5, commit_timestamp)[0].tobytes()


def test_limits_invalid_periods_and_orphans(ledger):
    transfers, accounts, checker, ids = ledger["transfers"], ledger["accounts"], ledger["checker"], ledger["ids"]
    assert len(ids_body(ids)) == 16 * len(ids)
    whole, matched, _ = checker.of(ids, 0, 0)
    assert matched == len(whole) == len(ids) - 4 and whole.dtype == INTEGRAL_DTYPE
    assert all(balances(r, "opening") == (0, 0, 0, 0) for r in whole) and all(int(r["t_end"]) == ledger["commit_timestamp"] for r in whole)
    for cap in (0, 1, matched - 1, matched, matched + 3):
        cut, m, _ = checker.of(ids, 0, 0, cap)
        assert m == matched and cut.tobytes() == whole[:cap].tobytes()
    t = int(np.sort(transfers["timestamp"])[len(transfers) // 2])
    for t_open, t_close in ((U64_MAX, 0), (0, U64_MAX), (U64_MAX, U64_MAX), (t, t - 1), (5, 1), (ledger["commit_timestamp"] + 1, 0)):
        rows, m, orphan = checker.of(ids, t_open, t_close)
        assert len(rows) == 0 and m == 0 and not orphan
    assert checker.of([], 0, 0)[1] == 0
    assert checker.of(ids, 0, 1)[1] == 0  # no account existed at timestamp 1
    # An orphan post: P is its own amount, and only a period or a tail that holds it says so.
    pending = {u128(p, "id"): p for p in transfers if int(p["flags"]) & PENDING}
    posts = [p for p in transfers if int(p["flags"]) & POST and not int(p["flags"]) & PENDING
             and u128(p, "amount") < u128(pending[u128(p, "pending_id")], "amount")]
    post = posts[-1]
    keep = transfers[[u128(r, "id") != u128(post, "pending_id") for r in transfers]]
    orphaned = Integrals(keep, accounts, ledger["commit_timestamp"])
    ts, debit = int(post["timestamp"]), u128(post, "debit_account_id")
    row, _, orphan = orphaned.of([debit], ts - 1, ts + 10)
    assert orphan
    own, whole_hold = u128(post, "amount"), u128(pending[u128(post, "pending_id")], "amount")
    full = checker.of([debit], ts - 1, ts + 10)[0][0]
    assert balances(full, "closing") == balances(row[0], "closing") and own < whole_hold
    assert (balances(full, "opening")[0] - balances(row[0], "opening")[0]) % MOD == whole_hold - own
    # Ten of the eleven ticks come after the release: the two checkers differ by the hold's remainder for one tick.
    assert integrals(full)[0] - integrals(row[0])[0] == whole_hold - own
    assert orphaned.of([debit], 1, ts - 1)[2] and not orphaned.of([debit], ts, 0)[2]
    assert not orphaned.of(ABSENT, ts - 1, ts)[2]
