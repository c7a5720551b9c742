"""The checker of tests/harness/counterparties.py pinned on hand-built logs, and against the flow
matrix's and the statements' checkers on a scenario, before any GPU answer is held to it.  No GPU."""
import numpy as np
import pytest

from tests.harness.balances import PENDING, POST, VOID, u128
from tests.harness.counterparties import (BY_VOLUME, CREDITS, DEBITS, REVERSED, ROWS_MAX, Counterparties, flow_sums, id_of,
                                          valid_filter, volume_of)
from tests.harness.matrix import FlowMatrix, cell_sums
from tests.harness.oracle import OracleEngine
from tests.harness.statements import Statements, sums, sweep_pairs
from tests.harness.workload import make_scenario
from tests.test_balance_checkers import QUERY_SCENARIO
from tigerbeetle_amd.types import COUNTERPARTY_DTYPE, TRANSFER_DTYPE, U64_MAX, pack_transfer

MOD = 1 << 128
A, B, C, D = 10, 20, 30, (7 << 64) | 5  # D: an id with a high word
ZERO = (0, 0, 0, 0)


def log_of(*records):
    """records: (id, debit, credit, amount, flags, timestamp[, pending_id])."""
    body = b"".join(pack_transfer(id=r[0], debit_account_id=r[1], credit_account_id=r[2], amount=r[3], flags=r[4], timestamp=r[5],
                                  pending_id=r[6] if len(r) > 6 else 0, ledger=1, code=1) for r in records)
    return np.frombuffer(body, dtype=TRANSFER_DTYPE)


def rows_of(answer):
    return {id_of(r): (flow_sums(r, "to"), flow_sums(r, "from")) for r in answer[0]}


def test_each_kind_in_both_directions():
    log = log_of((1, A, B, 100, 0, 10),            # plain A -> B
                 (2, A, B, 50, PENDING, 11),       # hold A -> B
                 (3, A, B, 30, POST, 12, 2),       # its partial post
                 (4, B, A, 70, PENDING, 13),       # hold B -> A
                 (5, B, A, 70, VOID, 14, 4),       # its void (stores the pending amount)
                 (6, B, A, 9, 0, 15),              # plain B -> A
                 (7, C, A, 4, 0, 16),              # C -> A
                 (8, B, C, 1000, 0, 17))           # names no A
    cp = Counterparties(log)
    rows, matched, orphan = cp.of(A)
    assert matched == 2 and not orphan and [id_of(r) for r in rows] == [B, C]
    assert rows_of((rows,)) == {B: ((130, 50, 50, 3), (9, 70, 70, 3)), C: (ZERO, (4, 0, 0, 1))}
    # One side only: the other half is all zero, and a counterparty seen only there is no group.
    assert rows_of(cp.of(A, flags=DEBITS)) == {B: ((130, 50, 50, 3), ZERO)}
    assert rows_of(cp.of(A, flags=CREDITS)) == {B: (ZERO, (9, 70, 70, 3)), C: (ZERO, (4, 0, 0, 1))}
    # The period (t_open, t_close]: open below, closed above, 0 closes at now.
    assert rows_of(cp.of(A, 11, 13)) == {B: ((30, 0, 50, 1), (0, 70, 0, 1))}
    assert rows_of(cp.of(A, 15, 0)) == {C: (ZERO, (4, 0, 0, 1))}
    assert cp.of(A, 16, 0)[1] == 0 and cp.of(A, 13, 13)[1] == 0
    # From the other end: B's counterparties.
    assert rows_of(cp.of(B)) == {A: ((9, 70, 70, 3), (130, 50, 50, 3)), C: ((1000, 0, 0, 1), ZERO)}
    # A subject no record names, and a subject outside any account table: ids are as the records carry them.
    assert cp.of(99)[1] == 0 and rows_of(cp.of(C)) == {A: ((4, 0, 0, 1), ZERO), B: (ZERO, (1000, 0, 0, 1))}


def test_the_self_record():
    log = log_of((1, A, A, 5, 0, 10), (2, A, B, 1, 0, 11))
    cp = Counterparties(log)
    assert rows_of(cp.of(A)) == {A: ((5, 0, 0, 1), (5, 0, 0, 1)), B: ((1, 0, 0, 1), ZERO)}
    assert rows_of(cp.of(A, flags=DEBITS)) == {A: ((5, 0, 0, 1), ZERO), B: ((1, 0, 0, 1), ZERO)}
    assert rows_of(cp.of(A, flags=CREDITS)) == {A: (ZERO, (5, 0, 0, 1))}


def test_an_orphan_post_inside_and_outside_the_period():
    log = log_of((1, A, B, 10, 0, 10), (3, A, C, 30, POST, 12, 2), (4, B, A, 1, 0, 14))  # transfer 2 is not resident
    cp = Counterparties(log)
    rows, matched, orphan = cp.of(A)
    assert orphan and rows_of((rows,))[C] == ((30, 0, 30, 1), ZERO)  # P = its own amount
    assert not cp.of(A, 12, 0)[2] and not cp.of(A, 0, 11)[2] and cp.of(A, 11, 12)[2]
    assert not cp.of(A, flags=CREDITS)[2] and cp.of(A, flags=DEBITS)[2] and cp.of(C, flags=CREDITS)[2]
    # Whether or not its group is returned, or at or above id_min.
    assert cp.of(A, limit=1)[2] and len(cp.of(A, limit=1)[0]) == 1
    assert cp.of(A, id_min=C + 1)[1:] == (0, True) and cp.of(A, cap=0)[1:] == (2, True)


def test_orders_volume_ties_and_id_min():
    big = (1 << 64) + 3
    log = log_of((1, A, B, 5, 0, 10), (2, C, A, 5, 0, 11),             # B and C: volume 5, a tie
                 (3, A, D, big, 0, 12), (4, D, A, (1 << 64) - 3, 0, 13),  # D: to + from carries across 2^64
                 (5, A, 40, 7, PENDING, 14),                            # 40: volume 0, a hold only
                 (6, A, 50, 6, 0, 15), (7, 50, A, MOD - 1, 0, 16))      # 50: the volume wraps modulo 2^128 to 5
    cp = Counterparties(log)
    by_id = cp.of(A)[0]
    assert [id_of(r) for r in by_id] == [B, C, 40, 50, D]  # as 128-bit numbers: D's high word puts it last
    by_volume = cp.of(A, flags=DEBITS | CREDITS | BY_VOLUME)[0]
    assert [id_of(r) for r in by_volume] == [D, B, C, 50, 40]
    assert [volume_of(r) for r in by_volume] == [2 << 64, 5, 5, 5, 0]
    # The cut falls inside the tie: the id decides who is in.
    assert [id_of(r) for r in cp.of(A, flags=3 | BY_VOLUME, limit=2)[0]] == [D, B]
    assert [id_of(r) for r in cp.of(A, flags=3 | BY_VOLUME, limit=3)[0]] == [D, B, C]
    # Under one side the volume is that side's alone.
    assert [id_of(r) for r in cp.of(A, flags=DEBITS | BY_VOLUME)[0]] == [D, 50, B, 40]
    # id_min narrows the groups under either order; `matched` counts what is left.
    assert [id_of(r) for r in cp.of(A, id_min=C)[0]] == [C, 40, 50, D] and cp.of(A, id_min=C)[1] == 4
    assert [id_of(r) for r in cp.of(A, flags=3 | BY_VOLUME, id_min=C)[0]] == [D, C, 50, 40]
    assert [id_of(r) for r in cp.of(A, id_min=D)[0]] == [D] and cp.of(A, id_min=D + 1)[1] == 0
    assert [id_of(r) for r in cp.of(A, id_min=(1 << 64))[0]] == [D]  # a high word above every low id
    # Paging by id_min with limit 2 gives the unpaged answer.
    pages, cursor = [], 0
    while True:
        page = cp.of(A, id_min=cursor, limit=2)[0]
        if len(page) == 0:
            break
        pages.append(page)
        cursor = id_of(page[-1]) + 1
    assert np.concatenate(pages).tobytes() == by_id.tobytes() and len(pages) == 3


def test_caps():
    log = log_of(*[(100 + i, A, 1000 + i, 1 + i, 0, 10 + i) for i in range(20)])
    cp = Counterparties(log)
    whole, matched, _ = cp.of(A)
    assert matched == len(whole) == 20
    for limit, cap, want in ((5, None, 5), (30, 7, 7), (7, 30, 7), (ROWS_MAX + 9, None, 20), (3, 0, 0)):
        rows, m, _ = cp.of(A, limit=limit, cap=cap)
        assert m == 20 and rows.tobytes() == whole[:want].tobytes()
    many = Counterparties(log_of(*[(100 + i, A, 10**6 + i, 1, 0, 10 + i) for i in range(ROWS_MAX + 5)]))
    rows, m, _ = many.of(A, limit=1 << 20)
    assert (len(rows), m) == (ROWS_MAX, ROWS_MAX + 5)


def test_invalid_filters_match_nothing():
    cp = Counterparties(log_of((1, A, B, 5, 0, 10)))
    assert cp.of(A)[1] == 1
    bad = [dict(account=0), dict(account=MOD - 1), dict(flags=0), dict(flags=BY_VOLUME), dict(flags=3 | REVERSED),
           dict(flags=3 | 1 << 9), dict(reserved=bytes(7) + b"\x01"), dict(t_open=U64_MAX), dict(t_close=U64_MAX),
           dict(t_open=9, t_close=8), dict(limit=0)]
    for kw in bad:
        kw = dict(dict(account=A), **kw)
        rows, matched, orphan = cp.of(**kw)
        assert len(rows) == 0 and rows.dtype == COUNTERPARTY_DTYPE and (matched, orphan) == (0, False), kw
    assert valid_filter(A, 9, 9, 1, DEBITS) and not valid_filter(A, 9, 8, 1, DEBITS)


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


def test_the_identities_against_the_matrix_and_the_statements(ledger):
    """`to` is the flow matrix's cell (a, x) and `from` its cell (x, a); the halves add up to the
    subject's statement."""
    cp, matrix = Counterparties(ledger["transfers"]), FlowMatrix(ledger["transfers"], ledger["accounts"])
    single, everyone = Statements(ledger["transfers"], ledger["accounts"]), ledger["everyone"]
    busy = 0
    for t_open, t_close in ledger["sweep"][::2]:
        statements = {u128(r, "id"): sums(r) for r in single.of(everyone, t_open, t_close)[0]}
        for a in everyone[::7]:
            rows, matched, orphan = cp.of(a, t_open, t_close)
            assert matched == len(rows) and not orphan
            total = [[0, 0, 0, 0], [0, 0, 0, 0]]
            for r in rows:
                x = id_of(r)
                if x in statements and a in statements:  # both found at t_close
                    assert flow_sums(r, "to") == cell_sums(matrix.of([a], [x], t_open, t_close)[0][0])
                    assert flow_sums(r, "from") == cell_sums(matrix.of([x], [a], t_open, t_close)[0][0])
                for half, direction in zip(total, ("to", "from")):
                    for q, v in enumerate(flow_sums(r, direction)):
                        half[q] += v
                busy += 1
            if a in statements:
                (d_in, d_out, d_posted, d_n), (c_in, c_out, c_posted, c_n) = statements[a]
                assert [v % MOD for v in total[0]] == [d_posted, d_in, d_out, d_n]
                assert [v % MOD for v in total[1]] == [c_posted, c_in, c_out, c_n]
    assert busy > 200
