"""The checker of tests/harness/activity.py pinned on hand-built logs, and against the statements' and the
counterparties' checkers on a scenario, before any GPU answer is held to it.  No GPU."""
import numpy as np
import pytest

from tests.harness.activity import (BY_TRANSFERS, BY_VOLUME, CREDITS, DEBITS, REVERSED, ROWS_MAX, Activity, half_sums, id_of,
                                    transfers_of, valid_filter, volume_of)
from tests.harness.balances import PENDING, POST, VOID, u128
from tests.harness.counterparties import Counterparties, flow_sums
from tests.harness.oracle import OracleEngine
from tests.harness.statements import Statements, sums, sweep_pairs
from tests.harness.workload import make_scenario
from tests.test_balance_checkers import QUERY_SCENARIO
from tigerbeetle_amd.types import ACCOUNT_ACTIVITY_DTYPE, TRANSFER_DTYPE, U64_MAX, pack_transfer

MOD = 1 << 128
A, B, C, D = 10, 20, 30, (7 << 64) | 5  # D: an id with a high word
ZERO = (0, 0, 0, 0)
BOTH = DEBITS | CREDITS


def log_of(*records):
    """records: (id, debit, credit, amount, flags, timestamp[, pending_id[, ledger[, code]]])."""
    body = b"".join(pack_transfer(id=r[0], debit_account_id=r[1], credit_account_id=r[2], amount=r[3], flags=r[4], timestamp=r[5],
                                  pending_id=r[6] if len(r) > 6 else 0, ledger=r[7] if len(r) > 7 else 1,
                                  code=r[8] if len(r) > 8 else 1) for r in records)
    return np.frombuffer(body, dtype=TRANSFER_DTYPE)


def rows_of(answer):
    return {id_of(r): (half_sums(r, "debits"), half_sums(r, "credits")) for r in answer[0]}


KINDS = log_of((1, A, B, 100, 0, 10),            # plain A -> B
               (2, A, B, 50, PENDING, 11),       # hold A -> B
               (3, A, B, 30, POST, 12, 2),       # its partial post
               (4, B, A, 70, PENDING, 13),       # hold B -> A
               (5, B, A, 70, VOID, 14, 4),       # its void (stores the pending amount)
               (6, B, A, 9, 0, 15),              # plain B -> A
               (7, C, A, 4, 0, 16),              # C -> A
               (8, B, C, 1000, 0, 17))           # B -> C


def test_each_kind_on_both_sides():
    act = Activity(KINDS)
    rows, matched, orphan = act.of()
    assert matched == 3 and not orphan and [id_of(r) for r in rows] == [A, B, C]
    assert rows_of((rows,)) == {A: ((130, 50, 50, 3), (13, 70, 70, 4)),
                                B: ((1009, 70, 70, 4), (130, 50, 50, 3)),
                                C: ((4, 0, 0, 1), (1000, 0, 0, 1))}
    # One side only: the other half is all zero, and an account seen only there is no group.
    assert rows_of(act.of(flags=DEBITS)) == {A: ((130, 50, 50, 3), ZERO), B: ((1009, 70, 70, 4), ZERO), C: ((4, 0, 0, 1), ZERO)}
    assert rows_of(act.of(15, 16, flags=DEBITS)) == {C: ((4, 0, 0, 1), ZERO)}
    assert rows_of(act.of(15, 16, flags=CREDITS)) == {A: (ZERO, (4, 0, 0, 1))}
    # The period (t_open, t_close]: open below, closed above, 0 closes at now.
    assert rows_of(act.of(11, 13)) == {A: ((30, 0, 50, 1), (0, 70, 0, 1)), B: ((0, 70, 0, 1), (30, 0, 50, 1))}
    assert rows_of(act.of(16, 0)) == {B: ((1000, 0, 0, 1), ZERO), C: (ZERO, (1000, 0, 0, 1))}
    assert act.of(17, 0)[1] == 0 and act.of(13, 13)[1] == 0
    # Double entry: the halves add up to the same four sums.
    assert [sum(v[0][q] for v in rows_of((rows,)).values()) for q in range(4)] == \
        [sum(v[1][q] for v in rows_of((rows,)).values()) for q in range(4)] == [1143, 120, 120, 8]


def test_the_self_record():
    act = Activity(log_of((1, A, A, 5, 0, 10), (2, A, B, 1, 0, 11)))
    assert rows_of(act.of()) == {A: ((6, 0, 0, 2), (5, 0, 0, 1)), B: (ZERO, (1, 0, 0, 1))}
    assert rows_of(act.of(flags=DEBITS)) == {A: ((6, 0, 0, 2), ZERO)}
    assert rows_of(act.of(flags=CREDITS)) == {A: (ZERO, (5, 0, 0, 1)), B: (ZERO, (1, 0, 0, 1))}
    assert act.of(0, 10)[1] == 1 and volume_of(act.of(0, 10)[0][0]) == 10 and transfers_of(act.of(0, 10)[0][0]) == 2


def test_ledger_and_code():
    log = log_of((1, A, B, 1, 0, 10, 0, 7, 12), (2, A, C, 2, 0, 11, 0, 7, 13), (3, B, C, 4, 0, 12, 0, 8, 12),
                 (4, C, D, 8, 0, 13, 0, 8, 13), (5, D, A, 16, PENDING, 14, 0, 7, 12))
    act = Activity(log)
    assert rows_of(act.of(ledger=7)) == {A: ((3, 0, 0, 2), (0, 16, 0, 1)), B: (ZERO, (1, 0, 0, 1)), C: (ZERO, (2, 0, 0, 1)),
                                         D: ((0, 16, 0, 1), ZERO)}
    assert rows_of(act.of(code=13)) == {A: ((2, 0, 0, 1), ZERO), C: ((8, 0, 0, 1), (2, 0, 0, 1)), D: (ZERO, (8, 0, 0, 1))}
    assert rows_of(act.of(ledger=7, code=12)) == {A: ((1, 0, 0, 1), (0, 16, 0, 1)), B: (ZERO, (1, 0, 0, 1)), D: ((0, 16, 0, 1), ZERO)}
    assert rows_of(act.of(0, 13, ledger=7, code=12, flags=CREDITS)) == {B: (ZERO, (1, 0, 0, 1))}
    assert act.of(ledger=9)[1] == 0 and act.of(code=9)[1] == 0 and act.of(ledger=8, code=9)[1] == 0
    assert act.of(ledger=7 | 1 << 16)[1] == 0 and act.of()[1] == 4


def test_an_orphan_post_inside_the_period_outside_it_and_under_a_failing_code():
    log = log_of((1, A, B, 10, 0, 10), (3, A, C, 30, POST, 12, 2, 1, 5), (4, B, A, 1, 0, 14))  # transfer 2 is not resident
    act = Activity(log)
    rows, matched, orphan = act.of()
    assert orphan and matched == 3 and rows_of((rows,))[C] == (ZERO, (30, 0, 30, 1))  # P = its own amount
    assert not act.of(12, 0)[2] and not act.of(0, 11)[2] and act.of(11, 12)[2]
    assert act.of(code=5)[2] and not act.of(code=1)[2] and not act.of(ledger=2)[2] and act.of(ledger=1)[2]
    # Whatever the sides, whether or not its groups are returned, or at or above id_min.
    assert act.of(flags=DEBITS)[2] and act.of(flags=CREDITS)[2]
    assert act.of(limit=1)[2] and len(act.of(limit=1)[0]) == 1
    assert act.of(id_min=C + 1)[1:] == (0, True) and act.of(cap=0)[1:] == (3, True)


def test_orders_ties_and_id_min():
    big = (1 << 64) + 3
    log = log_of((1, A, B, 5, 0, 10), (2, C, A, 5, 0, 11),                 # A 10 / 2 records, B 5 / 1, C 5 / 1
                 (3, D, 40, big, 0, 12), (4, 40, D, (1 << 64) - 3, 0, 13),  # D and 40: 2^65 each, a carry across 2^64, 2 records
                 (5, 50, 60, 7, PENDING, 14),                              # 50, 60: volume 0, a hold only
                 (6, 70, 80, 6, 0, 15), (7, 80, 70, MOD - 1, 0, 16))       # 70, 80: the volume wraps modulo 2^128 to 5
    act = Activity(log)
    by_id = act.of()[0]
    assert [id_of(r) for r in by_id] == [A, B, C, 40, 50, 60, 70, 80, D]  # as 128-bit numbers: D's high word puts it last
    by_volume = act.of(flags=BOTH | BY_VOLUME)[0]
    assert [id_of(r) for r in by_volume] == [40, D, A, B, C, 70, 80, 50, 60]
    assert [volume_of(r) for r in by_volume] == [2 << 64, 2 << 64, 10, 5, 5, 5, 5, 0, 0]
    by_transfers = act.of(flags=BOTH | BY_TRANSFERS)[0]
    assert [id_of(r) for r in by_transfers] == [A, 40, 70, 80, D, B, C, 50, 60]
    assert [transfers_of(r) for r in by_transfers] == [2, 2, 2, 2, 2, 1, 1, 1, 1]
    # The cut falls inside a tie: the id decides who is in.
    assert [id_of(r) for r in act.of(flags=BOTH | BY_VOLUME, limit=1)[0]] == [40]
    assert [id_of(r) for r in act.of(flags=BOTH | BY_VOLUME, limit=4)[0]] == [40, D, A, B]
    assert [id_of(r) for r in act.of(flags=BOTH | BY_TRANSFERS, limit=3)[0]] == [A, 40, 70]
    # Under one side the volume and the count are that side's alone.
    assert [id_of(r) for r in act.of(flags=DEBITS | BY_VOLUME)[0]] == [80, D, 40, 70, A, C, 50]
    assert [id_of(r) for r in act.of(flags=CREDITS | BY_TRANSFERS)[0]] == [A, B, 40, 60, 70, 80, D]
    # id_min narrows the groups under every order; `matched` counts what is left.
    assert [id_of(r) for r in act.of(id_min=C)[0]] == [C, 40, 50, 60, 70, 80, D] and act.of(id_min=C)[1] == 7
    assert [id_of(r) for r in act.of(flags=BOTH | BY_VOLUME, id_min=C)[0]] == [40, D, C, 70, 80, 50, 60]
    assert [id_of(r) for r in act.of(flags=BOTH | BY_TRANSFERS, id_min=60)[0]] == [70, 80, D, 60]
    assert [id_of(r) for r in act.of(id_min=D)[0]] == [D] and act.of(id_min=D + 1)[1] == 0
    assert [id_of(r) for r in act.of(id_min=(1 << 64))[0]] == [D]  # a high word above every low id
    # Paging by id_min with limit 2 gives the unpaged answer.
    pages, cursor = [], 0
    while True:
        page = act.of(id_min=cursor, limit=2)[0]
        if len(page) == 0:
            break
        pages.append(page)
        cursor = id_of(page[-1]) + 1
    assert np.concatenate(pages).tobytes() == by_id.tobytes() and len(pages) == 5


def test_caps():
    log = log_of(*[(100 + i, 1000 + i, 5000 + i, 1 + i, 0, 10 + i) for i in range(10)])
    act = Activity(log)
    whole, matched, _ = act.of()
    assert matched == len(whole) == 20
    for limit, cap, want in ((5, None, 5), (30, 7, 7), (7, 30, 7), (ROWS_MAX + 9, None, 20), (3, 0, 0)):
        rows, m, _ = act.of(limit=limit, cap=cap)
        assert m == 20 and rows.tobytes() == whole[:want].tobytes()
    many = Activity(log_of(*[(100 + i, 5, 10**6 + i, 1, 0, 10 + i) for i in range(ROWS_MAX + 5)]))
    rows, m, _ = many.of(limit=1 << 20)
    assert (len(rows), m) == (ROWS_MAX, ROWS_MAX + 6)


def test_invalid_filters_match_nothing():
    act = Activity(log_of((1, A, B, 5, 0, 10)))
    assert act.of()[1] == 2
    bad = [dict(flags=0), dict(flags=BY_VOLUME), dict(flags=BOTH | BY_VOLUME | BY_TRANSFERS), dict(flags=BOTH | REVERSED),
           dict(flags=BOTH | 1 << 10), dict(flags=BOTH | 1 << 31), dict(reserved=bytes(15) + b"\x01"), dict(reserved0=b"\x00\x01"),
           dict(t_open=U64_MAX), dict(t_close=U64_MAX), dict(t_open=9, t_close=8), dict(limit=0)]
    for kw in bad:
        rows, matched, orphan = act.of(**kw)
        assert len(rows) == 0 and rows.dtype == ACCOUNT_ACTIVITY_DTYPE and (matched, orphan) == (0, False), kw
    assert valid_filter(9, 9, 1, DEBITS) and not valid_filter(9, 8, 1, DEBITS)
    assert valid_filter(0, 0, 1, CREDITS | BY_TRANSFERS) and valid_filter(0, 0, 1, BOTH | BY_VOLUME)


@pytest.fixture(scope="module")
def ledger():
    sc = make_scenario(2025, **QUERY_SCENARIO)
    oracle = OracleEngine(4096, 1 << 15)
    for _, op, ts, events in sc.steps:
        oracle.commit(op, ts, b"".join(events))
    transfers, accounts = oracle.export_transfers(), oracle.export_accounts()
    commit_timestamp = oracle.commit_timestamp
    oracle.close()
    return dict(transfers=transfers, accounts=accounts, everyone=[u128(a, "id") for a in accounts],
                sweep=sweep_pairs(sc.steps, transfers, commit_timestamp))


def test_the_identities_against_the_statements_and_the_counterparties(ledger):
    """A row's halves are the account's statement, `debits` is the sum of `to` over the account's
    counterparties, the halves of all rows add up alike, and a ledger's rows are its accounts' rows."""
    act, cp = Activity(ledger["transfers"]), Counterparties(ledger["transfers"])
    single, everyone = Statements(ledger["transfers"], ledger["accounts"]), ledger["everyone"]
    ledger_of = {u128(a, "id"): int(a["ledger"]) for a in ledger["accounts"]}
    busy = 0
    for t_open, t_close in ledger["sweep"][::2]:
        statements = {u128(r, "id"): sums(r) for r in single.of(everyone, t_open, t_close)[0]}
        rows, matched, orphan = act.of(t_open, t_close)
        assert matched == len(rows) and not orphan
        total = [[0, 0, 0, 0], [0, 0, 0, 0]]
        for n, r in enumerate(rows):
            x = id_of(r)
            if x in statements:
                (d_in, d_out, d_posted, d_n), (c_in, c_out, c_posted, c_n) = statements[x]
                assert half_sums(r, "debits") == (d_posted, d_in, d_out, d_n) and half_sums(r, "credits") == (c_posted, c_in, c_out, c_n)
                busy += 1
            if n % 9 == 0:
                paid = cp.of(x, t_open, t_close, DEBITS)[0]
                assert tuple(sum(flow_sums(p, "to")[q] for p in paid) % MOD for q in range(4)) == half_sums(r, "debits")
            for half, name in zip(total, ("debits", "credits")):
                for q, v in enumerate(half_sums(r, name)):
                    half[q] += v
        assert [v % MOD for v in total[0][:3]] == [v % MOD for v in total[1][:3]] and total[0][3] == total[1][3]
        for L in sorted(set(ledger_of.values())):
            assert act.of(t_open, t_close, ledger=L)[0].tobytes() == rows[[ledger_of[id_of(r)] == L for r in rows]].tobytes()
    assert busy > 200
