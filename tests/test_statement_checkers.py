"""The checker of tests/harness/statements.py against the oracle, against lookup_accounts_at's checker
and against a brute-force pass over the oracle's export, before any GPU answer is held to it.  No GPU."""
import numpy as np

from tests.harness.asof import AsOf
from tests.harness.balances import MOD, PENDING, POST, VOID, balances_of, u128
from tests.harness.oracle import OracleEngine
from tests.harness.statements import SIDES, Statements, balances, ids_body, request_of, sums, sweep_pairs
from tests.harness.workload import account_id, make_scenario
from tests.test_balance_checkers import QUERY_SCENARIO
from tigerbeetle_amd.types import STATEMENT_DTYPE, U64_MAX

ABSENT = (account_id(5000), account_id(5001))


def brute_sums(transfers, amounts, account, t_open, t_close):
    """((in, out, posted, n) of the debit side, the same of the credit side) by masks over the export;
    amounts: {transfer id: amount}."""
    period = transfers["timestamp"] > t_open
    if t_close:
        period &= transfers["timestamp"] <= t_close
    out = []
    for name in ("debit_account_id", "credit_account_id"):
        mine = transfers[period & (transfers[name + "_lo"] == account & U64_MAX) & (transfers[name + "_hi"] == account >> 64)]
        flags = mine["flags"].astype(np.int64)
        pending, post, void = (flags & PENDING) != 0, (flags & POST) != 0, (flags & VOID) != 0
        total = lambda rows: sum(u128(t, "amount") for t in rows)
        held = lambda rows: sum(amounts[u128(t, "pending_id")] for t in rows)
        out.append((total(mine[pending]), held(mine[post | void]), total(mine[~pending & ~void]), len(mine)))
    return tuple(out)


def identities_hold(row):
    opening, closing, (debit, credit) = balances(row, "opening"), balances(row, "closing"), sums(row)
    for side, (p_in, p_out, posted, _) in enumerate((debit, credit)):
        if opening[2 * side] != (closing[2 * side] - p_in + p_out) % MOD or opening[2 * side + 1] != (closing[2 * side + 1] - posted) % MOD:
            return False
    return True


def test_checker_equals_the_oracle_the_asof_checker_and_a_brute_force_pass():
    sc = make_scenario(2025, **QUERY_SCENARIO)
    oracle = OracleEngine(4096, 1 << 15)
    after = {}  # prepare boundary -> {id: balances} as the oracle's accounts stood after that prepare
    for _, op, ts, events in sc.steps:
        oracle.commit(op, ts, b"".join(events))
        after[ts] = {u128(a, "id"): balances_of(a) for a in oracle.export_accounts()}
    transfers, accounts = oracle.export_transfers(), oracle.export_accounts()
    commit_timestamp = oracle.commit_timestamp
    oracle.close()
    checker, asof = Statements(transfers, accounts), AsOf(transfers, accounts)
    amounts = {u128(t, "id"): u128(t, "amount") for t in transfers}
    ids = request_of(accounts, ABSENT)
    boundaries = sorted(after)

    # closing at a boundary is the oracle's accounts after that prepare; opening of (B1, B2] those after B1.
    for k, b2 in enumerate(boundaries):
        b1 = boundaries[k // 2]
        rows, matched, orphan = checker.of(ids, b1, b2)
        assert matched == len(rows) == sum(1 for i in ids if i in after[b2]) and not orphan
        for row in rows:
            i = u128(row, "id")
            assert balances(row, "closing") == after[b2][i], (b2, hex(i))
            assert balances(row, "opening") == after[b1].get(i, (0, 0, 0, 0)), (b1, b2, hex(i))

    # Every swept pair: lookup_accounts_at's checker at both ends, the brute-force sums, the identities.
    partial = voided = moved = 0
    answers = set()
    for t_open, t_close in sweep_pairs(sc.steps, transfers, commit_timestamp):
        rows, matched, orphan = checker.of(ids, t_open, t_close)
        at_close, close_matched, _ = asof.at(ids, t_close)
        assert matched == close_matched == len(rows) and not orphan
        assert [u128(r, "id") for r in rows] == [u128(r, "id") for r in at_close]
        at_open = {u128(r, "id"): balances_of(r) for r in asof.at(ids, t_open)[0]} if t_open >= 1 else {}
        for row, rec in zip(rows, at_close):
            i = u128(row, "id")
            assert balances(row, "closing") == balances_of(rec), (t_open, t_close, hex(i))
            if i in at_open:
                assert balances(row, "opening") == at_open[i], (t_open, t_close, hex(i))
            assert sums(row) == brute_sums(transfers, amounts, i, t_open, t_close), (t_open, t_close, hex(i))
            assert identities_hold(row)
            for side in SIDES:
                out, posted = u128(row, side + "_pending_out"), u128(row, side + "_posted_in")
                partial += out != 0 and posted != 0 and out != posted
            moved += any(sums(row)[s][3] for s in (0, 1))
        if t_open == t_close != 0:  # an empty period; (0, 0) is the whole log
            assert all(sums(r) == ((0, 0, 0, 0), (0, 0, 0, 0)) and balances(r, "opening") == balances(r, "closing") for r in rows)
        answers.add(rows.tobytes())
    voids = transfers[(transfers["flags"] & VOID) != 0]
    for v in voids[:5]:
        ts, debit = int(v["timestamp"]), u128(v, "debit_account_id")
        row = checker.of([debit], ts - 1, ts)[0][0]
        assert sums(row)[0] == (0, u128(v, "amount"), 0, 1) and u128(v, "amount") > 0
        voided += 1
    assert partial > 0 and voided > 0 and moved > 100 and len(answers) > 20
    # (0, 0) is the whole log: closing is now, opening is zero, the counts are the export's.
    rows = checker.of(ids, 0, 0)[0]
    final = {u128(a, "id"): balances_of(a) for a in accounts}
    assert all(balances(r, "closing") == final[u128(r, "id")] and balances(r, "opening") == (0, 0, 0, 0) for r in rows)
    distinct = {u128(r, "id"): r for r in rows}
    assert sum(int(r["debit_transfers"]) for r in distinct.values()) == len(transfers)
    assert sum(int(r["credit_transfers"]) for r in distinct.values()) == len(transfers)


def test_limits_invalid_periods_and_orphans():
    sc = make_scenario(2025, **QUERY_SCENARIO)
    oracle = OracleEngine(4096, 1 << 15)
    for _, op, ts, events in sc.steps:
        oracle.commit(op, ts, b"".join(events))
    transfers, accounts = oracle.export_transfers(), oracle.export_accounts()
    oracle.close()
    checker = Statements(transfers, accounts)
    ids = request_of(accounts, ABSENT)
    assert len(ids_body(ids)) == 16 * len(ids)
    whole, matched, _ = checker.of(ids, 0, 0)
    assert matched == len(whole) == len(ids) - 4 and whole.dtype == STATEMENT_DTYPE
    for cap in (0, 1, matched - 1, matched, matched + 3):
        cut, m, _ = checker.of(ids, 0, 0, cap)
        assert m == matched and cut.tobytes() == whole[:cap].tobytes()
    t = int(np.sort(transfers["timestamp"])[len(transfers) // 2])
    for t_open, t_close in ((U64_MAX, 0), (0, U64_MAX), (U64_MAX, U64_MAX), (t, t - 1), (5, 1)):
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
    orphaned = Statements(keep, accounts)
    ts, debit = int(post["timestamp"]), u128(post, "debit_account_id")
    row, _, orphan = orphaned.of([debit], ts - 1, ts)
    assert orphan and sums(row[0])[0] == (0, u128(post, "amount"), u128(post, "amount"), 1)
    assert sums(checker.of([debit], ts - 1, ts)[0][0])[0] == (0, u128(pending[u128(post, "pending_id")], "amount"), u128(post, "amount"), 1)
    assert orphaned.of([debit], 0, ts - 1)[2] and not orphaned.of([debit], ts, 0)[2]
    assert not orphaned.of(ABSENT, ts - 1, ts)[2]
