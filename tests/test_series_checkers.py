"""The checker of tests/harness/series.py against get_account_statements' checker and against the
identities the header states, before any GPU answer is held to it.  No GPU."""
import pytest

from tests.harness.balances import u128
from tests.harness.oracle import OracleEngine
from tests.harness.series import Series, bounds_sweep, valid_bounds
from tests.harness.statements import SIDES, Statements, balances, request_of, sums
from tests.harness.workload import account_id, make_scenario
from tests.test_balance_checkers import QUERY_SCENARIO
from tigerbeetle_amd.types import STATEMENT_DTYPE, U64_MAX

ABSENT = (account_id(5000), account_id(5001))
NOTHING = ((0, 0, 0, 0), (0, 0, 0, 0))


@pytest.fixture(scope="module")
def ledger():
    sc = make_scenario(2025, **QUERY_SCENARIO)
    oracle = OracleEngine(4096, 1 << 15)
    for _, op, ts, events in sc.steps:
        oracle.commit(op, ts, b"".join(events))
    transfers, accounts = oracle.export_transfers(), oracle.export_accounts()
    commit_timestamp = oracle.commit_timestamp
    oracle.close()
    return dict(series=Series(transfers, accounts), single=Statements(transfers, accounts), ids=request_of(accounts, ABSENT),
                accounts=accounts, sweep=bounds_sweep(sc.steps, transfers, commit_timestamp))


def test_rows_are_the_single_calls_and_the_identities_hold(ledger):
    series, single, ids = ledger["series"], ledger["single"], ledger["ids"]
    created = {u128(a, "id"): int(a["timestamp"]) for a in ledger["accounts"]}
    partial = empty = young = 0
    for bounds in ledger["sweep"]:
        n_buckets, last = len(bounds) - 1, bounds[-1]
        rows, matched, orphan = series.of(ids, bounds)
        found = [i for i in ids if i in created and (last == 0 or created[i] <= last)]
        assert matched == len(rows) == len(found) * n_buckets and not orphan and len(found) > 0
        for r, account in enumerate(found):
            mine = rows[r * n_buckets:(r + 1) * n_buckets]
            assert all(u128(row, "id") == account for row in mine)
            for k, row in enumerate(mine):
                want, m, _ = single.of([account], bounds[k], bounds[k + 1])
                if m:  # wherever the single call yields a row, it is this one
                    assert row.tobytes() == want[0].tobytes(), (bounds, k)
                else:  # created above the bucket's end: zeros on a clean ledger
                    assert created[account] > bounds[k + 1] != 0
                    assert balances(row, "opening") == balances(row, "closing") == (0, 0, 0, 0) and sums(row) == NOTHING
                    young += 1
                if k + 1 < n_buckets:
                    assert balances(row, "closing") == balances(mine[k + 1], "opening")
                empty += bounds[k] == bounds[k + 1] != 0 and sums(row) == NOTHING
                partial += any(u128(row, s + "_pending_out") and u128(row, s + "_posted_in")
                               and u128(row, s + "_pending_out") != u128(row, s + "_posted_in") for s in SIDES)
            # The last closing is the single call's over the whole period, and so are the sums and counts.
            whole = single.of([account], bounds[0], last)[0][0]
            assert balances(mine[-1], "closing") == balances(whole, "closing")
            assert balances(mine[0], "opening") == balances(whole, "opening")
            total = tuple(tuple(sum(sums(row)[side][q] for row in mine) % (1 << 128) for q in range(4)) for side in range(2))
            assert total == sums(whole)
        if n_buckets == 1:
            want, m, _ = single.of(ids, bounds[0], bounds[1])
            assert rows.tobytes() == want.tobytes() and matched == m
    # Non-vacuity: a partial post in some bucket, an empty bucket, an account younger than bounds[1].
    assert partial > 0 and empty > 0 and young > 0
    assert any(created[i] > bounds[1] for bounds in ledger["sweep"] for i in created if len(bounds) > 2
               and (bounds[-1] == 0 or created[i] <= bounds[-1]))


def test_cap_cuts_in_row_order(ledger):
    series, ids = ledger["series"], ledger["ids"]
    bounds = ledger["sweep"][7]
    rows, matched, _ = series.of(ids, bounds)
    assert len(bounds) == 4 and matched > 10
    for cap in (0, 1, 4, matched, matched + 2):
        cut, m, _ = series.of(ids, bounds, cap)
        assert m == matched and cut.tobytes() == rows[:cap].tobytes()


def test_invalid_bounds_give_the_empty_answer(ledger):
    series, ids = ledger["series"], ledger["ids"]
    t = ledger["sweep"][1]
    for bounds in ([U64_MAX, 0], [0, U64_MAX], [t[0], U64_MAX, 0], [t[0], 0, t[1]], [t[1], t[0]], [t[0], t[1], t[0]], [t[1], t[0], 0]):
        assert not valid_bounds(bounds)
        rows, matched, orphan = series.of(ids, bounds)
        assert len(rows) == 0 and rows.dtype == STATEMENT_DTYPE and (matched, orphan) == (0, False)
    for bounds in ([t[0], t[0]], [t[0], t[1], 0], [0, t[0], t[0], 0], [t[1], 0]):
        assert valid_bounds(bounds) and series.of(ids, bounds)[1] > 0
    assert series.of([], t)[1] == 0
