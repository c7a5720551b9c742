"""The checker of tests/harness/ledgers.py against the oracle and against AsOf, before any GPU answer is
held to it.  No GPU."""
import numpy as np

from tests.harness.asof import AsOf
from tests.harness.balances import MOD, PENDING, POST, balances_of, u128
from tests.harness.ledgers import LedgerBalances, ledgers_body, sums_by_ledger
from tests.harness.oracle import OracleEngine
from tests.harness.workload import make_scenario
from tests.test_balance_checkers import QUERY_SCENARIO
from tigerbeetle_amd.types import LEDGER_BALANCE_DTYPE, pack_account, pack_transfer

LEDGERS = (1, 2, 7, 2**32 - 1)
REQUEST = list(LEDGERS) + [0, 5]


def row_tuple(row):
    return balances_of(row), int(row["accounts"])


def test_checker_equals_the_oracle_and_asof():
    sc = make_scenario(2031, ledgers=LEDGERS, **QUERY_SCENARIO)
    oracle = OracleEngine(4096, 1 << 15)
    recorded = []  # (boundary, {ledger: (sums, accounts)}) after each prepare
    for _, op, ts, events in sc.steps:
        oracle.commit(op, ts, b"".join(events))
        recorded.append((ts, sums_by_ledger(oracle.export_accounts())))
    transfers, accounts = oracle.export_transfers(), oracle.export_accounts()
    oracle.close()
    assert len(transfers) > 700 and len(accounts) > 50
    assert {int(a["ledger"]) for a in accounts} == set(LEDGERS)
    assert {int(t["ledger"]) for t in transfers} == set(LEDGERS)
    checker = LedgerBalances(transfers, accounts)
    assert len(recorded) == 26
    distinct = set()
    for boundary, want in recorded:
        rows, matched, orphan = checker.at(REQUEST, boundary)
        assert matched == len(rows) == len(REQUEST) and not orphan
        assert rows["ledger"].tolist() == REQUEST and not rows["reserved"].any()
        for row, L in zip(rows, REQUEST):
            sums, count = want.get(L, ([0, 0, 0, 0], 0))
            assert row_tuple(row) == (tuple(sums), count), (boundary, L)
            b = balances_of(row)
            assert b[0] == b[2] and b[1] == b[3]  # every row has debits == credits
        distinct.add(rows.tobytes())
    assert len(distinct) > 20
    # Inside the prepares: the per-ledger sum of AsOf over every account.
    asof = AsOf(transfers, accounts)
    ids = [u128(a, "id") for a in accounts]
    boundaries = {b for b, _ in recorded}
    inside = 0
    for T in [int(t) for t in np.sort(transfers["timestamp"])[::97]]:
        inside += T not in boundaries
        records, _, _ = asof.at(ids, T)
        want = sums_by_ledger(records)
        rows, _, orphan = checker.at(REQUEST, T)
        assert not orphan
        for row, L in zip(rows, REQUEST):
            sums, count = want.get(L, ([0, 0, 0, 0], 0))
            assert row_tuple(row) == (tuple(sums), count), (T, L)
            b = balances_of(row)
            assert b[0] == b[2] and b[1] == b[3]
    assert inside > 0
    # Now, and at or above the newest record: the current sums.
    now = sums_by_ledger(accounts)
    for T in (0, int(transfers["timestamp"].max()), int(transfers["timestamp"].max()) + 5):
        rows, _, _ = checker.at(REQUEST, T)
        for row, L in zip(rows, REQUEST):
            sums, count = now.get(L, ([0, 0, 0, 0], 0))
            assert row_tuple(row) == (tuple(sums), count)
    # Before everything: every account is younger than T and every record newer.
    rows, _, _ = checker.at(REQUEST, 1)
    assert all(row_tuple(r) == ((0, 0, 0, 0), 0) for r in rows)


def hand_ledger():
    """Two ledgers by hand: a pending transfer and its partial post on ledger 1, a plain transfer on
    ledger 2, through the oracle."""
    oracle = OracleEngine(64, 1 << 10)
    accounts = b"".join(pack_account(id=i, ledger=1 if i < 3 else 2, code=1) for i in (1, 2, 3, 4))
    assert oracle.commit(128, 100, accounts) == b""
    events = [pack_transfer(id=10, debit_account_id=1, credit_account_id=2, amount=100, ledger=1, code=1, flags=PENDING),
              pack_transfer(id=11, debit_account_id=3, credit_account_id=4, amount=7, ledger=2, code=1),
              pack_transfer(id=12, pending_id=10, amount=60, flags=POST)]
    assert oracle.commit(129, 203, b"".join(events)) == b""
    return oracle


def test_hand_cases():
    oracle = hand_ledger()
    transfers, accounts = oracle.export_transfers(), oracle.export_accounts()
    checker = LedgerBalances(transfers, accounts)
    # A repeated ledger, ledger 0 and an unknown one, at each record's timestamp.
    request = [2, 1, 0, 1, 9]
    rows, matched, orphan = checker.at(request, 201)
    assert matched == 5 and not orphan and rows.dtype == LEDGER_BALANCE_DTYPE
    assert [row_tuple(r) for r in rows] == [((0, 0, 0, 0), 2), ((100, 0, 100, 0), 2), ((100, 0, 100, 0), 4),
                                            ((100, 0, 100, 0), 2), ((0, 0, 0, 0), 0)]
    assert rows["ledger"].tolist() == request
    assert [row_tuple(r) for r in checker.at(request, 202)[0]] == [((0, 7, 0, 7), 2), ((100, 0, 100, 0), 2), ((100, 7, 100, 7), 4),
                                                                   ((100, 0, 100, 0), 2), ((0, 0, 0, 0), 0)]
    for T in (203, 0, 500):
        assert [row_tuple(r) for r in checker.at(request, T)[0]] == [((0, 7, 0, 7), 2), ((0, 60, 0, 60), 2), ((0, 67, 0, 67), 4),
                                                                     ((0, 60, 0, 60), 2), ((0, 0, 0, 0), 0)]
    assert [int(r["accounts"]) for r in checker.at(request, 96)[0]] == [0, 0, 0, 0, 0]
    # cap cuts in request order; matched stays n.
    for cap in (0, 1, 4, 5, 8):
        cut, matched, _ = checker.at(request, 202, cap)
        assert matched == 5 and cut.tobytes() == checker.at(request, 202)[0][:cap].tobytes()
    assert checker.at(request, (1 << 64) - 1)[1] == 0 and checker.at([], 5)[1] == 0
    assert ledgers_body([1, 2**32 - 1]) == b"\x01\x00\x00\x00\xff\xff\xff\xff"
    # An orphan post: summed with P = its own amount, flagged only when its ledger or 0 is asked and
    # T is below it.
    keep = transfers[[u128(t, "id") != 10 for t in transfers]]
    orphaned = LedgerBalances(keep, accounts)
    rows, _, orphan = orphaned.at([1], 202)
    assert orphan and row_tuple(rows[0]) == ((60, 0, 60, 0), 2)
    assert orphaned.at([0], 202)[2] and not orphaned.at([2, 9], 202)[2] and not orphaned.at([1, 0], 203)[2]
    # set_balances: the anchor is the current balance, debits != credits allowed.
    oracle.set_balances(1, 5, 6, 7, 8)
    moved = LedgerBalances(transfers, oracle.export_accounts())
    assert row_tuple(moved.at([1], 0)[0][0]) == ((5, 6 + 0, 7 + 0, 8 + 60), 2)
    assert row_tuple(moved.at([1], 202)[0][0]) == ((5 + 100, (6 - 60) % MOD, 7 + 100, 8), 2)
    # Wrap modulo 2^128: two accounts of a ledger with 2^127 each.
    oracle.set_balances(1, 1 << 127, 0, 0, 0)
    oracle.set_balances(2, (1 << 127) + 3, 0, 0, 0)
    wrapped = LedgerBalances(transfers, oracle.export_accounts())
    assert balances_of(wrapped.at([1], 0)[0][0]) == (3, 0, 0, 0)
    assert balances_of(wrapped.at([0], 0)[0][0]) == (3, 7, 0, 7)
    oracle.close()
