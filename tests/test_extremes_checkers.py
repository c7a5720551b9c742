"""The checker of tests/harness/extremes.py against the oracle's own per-event balances — a second
oracle that commits one event per prepare and exports the accounts after each
(tests/harness/balances.py oracle_rows), and the forward replay that tests/test_balance_checkers.py holds
to it on the query ledger — before any GPU answer is held to the checker.  No GPU."""
import numpy as np
import pytest

from tests.harness.balances import balances_of, oracle_rows, replay_rows, u128
from tests.harness.extremes import Extremes
from tests.harness.oracle import OracleEngine
from tests.harness.statements import request_of, sweep_pairs
from tests.harness.workload import account_id, make_scenario
from tests.test_balance_checkers import CHAIN_FREE, QUERY_SCENARIO
from tigerbeetle_amd import types as T
from tigerbeetle_amd.types import EXTREME_DTYPE, extreme_value, pack_balance_measure

ABSENT = (account_id(5000), account_id(5001))
MEASURES = (T.MEASURE_CREDIT_NET_POSTED, T.MEASURE_CREDIT_AVAILABLE, T.MEASURE_DEBIT_NET_POSTED, T.MEASURE_DEBIT_AVAILABLE,
            T.MEASURE_DEBITS_PENDING, T.MEASURE_DEBITS_POSTED, T.MEASURE_CREDITS_PENDING, T.MEASURE_CREDITS_POSTED)


def committed(sc):
    oracle = OracleEngine(4096, 1 << 15)
    for _, op, ts, events in sc.steps:
        oracle.commit(op, ts, b"".join(events))
    out = oracle.export_transfers(), oracle.export_accounts(), oracle.commit_timestamp
    oracle.close()
    return out


def from_history(history, t_open, t_end, measure):
    """(opening, closing, low, high, t_low, t_high, records) from an account's per-event balances
    [(timestamp, side, balances)], oldest first; before its first event an account holds nothing."""
    value = lambda balances: sum(k * b for k, b in zip(measure, balances))
    opening = 0
    for ts, _, balances in history:
        if ts <= t_open:
            opening = value(balances)
    low = high = closing = opening
    t_low = t_high = t_open
    records = 0
    for ts, _, balances in history:
        if t_open < ts <= t_end:
            closing = value(balances)
            records += 1
            if closing < low:
                low, t_low = closing, ts
            if closing > high:
                high, t_high = closing, ts
    return opening, closing, low, high, t_low, t_high, records


def hold_to(histories, transfers, accounts, commit_timestamp, steps):
    checker = Extremes(transfers, accounts, commit_timestamp)
    stamps = np.sort(transfers["timestamp"])
    periods = [(0, commit_timestamp), (int(stamps[len(stamps) // 4]), int(stamps[3 * len(stamps) // 4])), (int(stamps[10]), int(stamps[11])),
               (int(stamps[50]) - 1, int(stamps[-50])), (steps[2][2], steps[-2][2]), (int(stamps[-1]), commit_timestamp + 9)]
    moved = negative = 0
    for account in (u128(a, "id") for a in accounts):
        history = histories.get(account, [])
        for k, (t_open, t_end) in enumerate(periods):
            for measure in (MEASURES[k % len(MEASURES)], MEASURES[(k + 3) % len(MEASURES)], T.MEASURE_CREDIT_AVAILABLE):
                want = from_history(history, t_open, t_end, measure)
                assert checker.one(account, t_open, t_end, measure) == want, (hex(account), t_open, t_end, measure)
                moved += want[2] != want[3]
                negative += want[2] < 0
    assert moved > 50 and negative > 10
    return checker


def test_checker_equals_the_oracles_per_event_balances():
    sc = make_scenario(7, **CHAIN_FREE)
    transfers, accounts, commit_timestamp = committed(sc)
    histories = oracle_rows(sc.steps)
    assert sum(len(r) for r in histories.values()) == 2 * len(transfers) > 200
    hold_to(histories, transfers, accounts, commit_timestamp, sc.steps)


def test_checker_on_the_query_ledger_and_its_rows():
    """The query ledger (linked chains, limits, balancing transfers), against the forward replay that
    tests/test_balance_checkers.py holds to the oracle; then the rows `of` writes."""
    sc = make_scenario(2025, **QUERY_SCENARIO)
    transfers, accounts, commit_timestamp = committed(sc)
    checker = hold_to(replay_rows(transfers), transfers, accounts, commit_timestamp, sc.steps)
    ids = request_of(accounts, ABSENT)
    seen = set()
    for k, (t_open, t_close) in enumerate(sweep_pairs(sc.steps, transfers, commit_timestamp)):
        measure = MEASURES[k % len(MEASURES)]
        rows, matched, orphan = checker.of(ids, t_open, t_close, measure)
        assert rows.dtype == EXTREME_DTYPE and matched == len(rows) and not orphan
        t_end = t_close if t_close else commit_timestamp
        for r in rows:
            one = checker.one(u128(r, "id"), t_open, t_end, measure)
            assert tuple(extreme_value(r, f) for f in ("opening", "closing", "low", "high")) == one[:4]
            assert (int(r["t_low"]), int(r["t_high"]), int(r["records"]), int(r["t_open"]), int(r["t_end"])) == one[4:] + (t_open, t_end)
            assert int(r["measure"]).to_bytes(8, "little") == pack_balance_measure(measure) and not r["reserved"].any()
            assert one[2] <= one[0] <= one[3] and one[2] <= one[1] <= one[3]
            assert (one[6] == 0) <= (one[0] == one[1] == one[2] == one[3] and one[4] == one[5] == t_open)
        seen.add(rows.tobytes())
        assert len(checker.of(ids, t_open, t_close, measure, cap=3)[0]) == min(3, matched)
    assert len(seen) > 20


def test_a_single_posted_column_only_grows():
    """low == opening at t_open and high == closing, for every account and period."""
    sc = make_scenario(2025, **QUERY_SCENARIO)
    transfers, accounts, commit_timestamp = committed(sc)
    checker = Extremes(transfers, accounts, commit_timestamp)
    stamps = np.sort(transfers["timestamp"])
    grew = 0
    for t_open, t_end in ((0, commit_timestamp), (int(stamps[100]), int(stamps[1500])), (int(stamps[700]), int(stamps[701]))):
        for measure in (T.MEASURE_DEBITS_POSTED, T.MEASURE_CREDITS_POSTED):
            for a in accounts:
                opening, closing, low, high, t_low, t_high, records = checker.one(u128(a, "id"), t_open, t_end, measure)
                assert low == opening and high == closing and t_low == t_open
                assert (t_high == t_open) == (closing == opening)
                grew += closing > opening
    assert grew > 100
    assert balances_of(accounts[0]) == checker.balance_at(u128(accounts[0], "id"), commit_timestamp)
