"""The account-set scan's calls back to back on one engine (csrc/k_account_scan.h, the driver in
csrc/query.h): lookup_accounts_at, get_account_statements, get_account_balance_integrals and
get_account_statement_series share buffers and one host driver, and the files that test each of them
give each its own engine.  Here one engine, and a two-shard node, answer them interleaved; what one
call leaves in a shared buffer must not reach the next.  The answers are held to each other by the
calls' definitions (no tolerance: every column is exact modulo 2^128), to the checkers of
tests/harness and, the node's, to the single engine's bytes."""
import numpy as np
import pytest

from tests.harness import integrals as integrals_h
from tests.harness.asof import AsOf
from tests.harness.balances import balances_of, u128
from tests.harness.integrals import Integrals
from tests.harness.series import Series
from tests.harness.statements import Statements, balances, sums
from tests.harness.workload import account_id
from tigerbeetle_amd.types import TransferFlags, pack_account, pack_transfer

pytestmark = pytest.mark.gpu

PENDING = int(TransferFlags.pending)
POST = int(TransferFlags.post_pending_transfer)
VOID = int(TransferFlags.void_pending_transfer)
N_ACC, FIRST, SECOND = 8, 600, 500  # 1,100 transfers in two prepares: two 512-record tiles, 18 waves
A = account_id(0)
BASE = 10**12


def bodies():
    """Account A alone in every lane of the wave at positions 128-191 of the single engine's log; a
    pending transfer of A in the first prepare and its partial post in the second, another and its
    void; amounts whose sums carry across the 64-bit word."""
    batch = []
    for i in range(FIRST + SECOND):
        dr = 1 + i % (N_ACC - 1)
        cr = 1 + (dr + i // 7) % (N_ACC - 1)
        if cr == dr:
            cr = 1 + dr % (N_ACC - 1)
        ev = dict(id=1000 + i, debit_account_id=account_id(dr), credit_account_id=account_id(cr), amount=1 + i, ledger=1, code=1)
        other = account_id(1 + i % (N_ACC - 1))
        if 128 <= i < 192:
            ev.update(amount=(1 << 64) - 1 - i, flags=PENDING if i % 7 == 3 else 0)
            ev.update(debit_account_id=A, credit_account_id=other) if i % 2 == 0 else ev.update(debit_account_id=other, credit_account_id=A)
        elif i == 1050:  # above every period's end
            ev.update(debit_account_id=A, credit_account_id=other)
        elif i == 10:
            ev.update(debit_account_id=A, credit_account_id=other, amount=1 << 100, flags=PENDING)
        elif i == 61:
            ev.update(debit_account_id=other, credit_account_id=A, amount=1 << 64, flags=PENDING)
        elif i == 700:
            ev.update(debit_account_id=0, credit_account_id=0, amount=(1 << 64) - 1, pending_id=1010, flags=POST)
        elif i == 900:
            ev.update(debit_account_id=0, credit_account_id=0, amount=0, pending_id=1061, flags=VOID)
        batch.append(pack_transfer(**ev))
    return b"".join(batch[:FIRST]), b"".join(batch[FIRST:])


def at(i):
    """Event i's timestamp: a prepare's events end at its timestamp."""
    return BASE + 10**6 + i + 1 if i < FIRST else BASE + 2 * 10**6 + (i - FIRST) + 1


def commit(engine):
    accounts = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(N_ACC))
    assert engine.commit(128, BASE, accounts) == b""
    first, second = bodies()
    assert engine.commit(129, at(FIRST - 1), first) == b""
    assert engine.commit(129, at(FIRST + SECOND - 1), second) == b""


def interleaved(engine, ids, t0, tm, t1):
    """The calls, back to back on the one engine, in the order that hands each buffer from call to call."""
    return [engine.lookup_accounts_at(ids, t0),
            engine.get_account_statements(ids, t0, t1),
            engine.get_account_balance_integrals(ids, t0, t1),
            engine.get_account_statement_series(ids, [t0, tm, t1]),
            engine.lookup_accounts_at(ids, t1),
            engine.get_account_statements(ids, t0, t1),
            engine.lookup_accounts_at(ids, 0)]


def test_calls_interleaved_on_one_engine_and_on_a_node(gpu_engine_factory):
    single = gpu_engine_factory(accounts_max=64, transfers_max=1 << 12)
    node = gpu_engine_factory(accounts_max=64, transfers_max=1 << 12, pass_events_max=2048, pass_batches_max=16, devices=(0, 0))
    commit(single)
    commit(node)
    transfers, accounts = single.export_transfers(), single.export_accounts()
    assert len(transfers) == FIRST + SECOND
    by_time = transfers[np.argsort(transfers["timestamp"], kind="stable")]
    assert [int(t) for t in by_time["timestamp"][[0, 128, 700, FIRST + SECOND - 1]]] == [at(0), at(128), at(700), at(FIRST + SECOND - 1)]
    wave = by_time[128:192]
    assert all(A in (u128(t, "debit_account_id"), u128(t, "credit_account_id")) for t in wave)
    # t0 cuts the first tile behind A's wave and both pending transfers; the post, the tile edge and
    # the prepares' border lie in the period, the void in its second bucket, 99 records above t1.
    t0, tm, t1 = at(300), at(640), at(1000)
    ids = [account_id(i) for i in range(N_ACC)] + [A, account_id(5000)]  # A twice, and an id nobody has
    found = N_ACC + 1
    answers = interleaved(single, ids, t0, tm, t1)
    at0, stmt, integ, series, at1, stmt_again, now = [a[0] for a in answers]
    assert [(a[1], a[2]) for a in answers] == [(found, True)] * 3 + [(2 * found, True)] + [(found, True)] * 3
    assert [len(a[0]) for a in answers] == [found] * 3 + [2 * found] + [found] * 3

    assert [balances(r, "opening") for r in stmt] == [balances_of(a) for a in at0]
    assert [balances(r, "closing") for r in stmt] == [balances_of(a) for a in at1]
    assert [integrals_h.balances(r, "opening") for r in integ] == [balances(r, "opening") for r in stmt]
    assert [integrals_h.balances(r, "closing") for r in integ] == [balances(r, "closing") for r in stmt]
    assert [balances(r, "opening") for r in series[0::2]] == [balances(r, "opening") for r in stmt]
    assert [balances(r, "closing") for r in series[1::2]] == [balances(r, "closing") for r in stmt]
    for whole, early, late in zip(stmt, series[0::2], series[1::2]):
        assert sums(whole) == tuple(tuple(x + y for x, y in zip(e, l)) for e, l in zip(sums(early), sums(late)))
    assert stmt_again.tobytes() == stmt.tobytes()
    assert now.tobytes() == AsOf(transfers, accounts).at(ids, 0)[0].tobytes()
    assert stmt[0].tobytes() == stmt[N_ACC].tobytes() and at0[0].tobytes() == at0[N_ACC].tobytes()  # A, and A again
    # The planted records are where the period has them: the partial post releases the whole hold.
    assert sums(stmt[0])[0][1] >= 1 << 100 and sums(stmt[0])[1][1] >= 1 << 64
    assert balances_of(at0[0]) != balances_of(at1[0]) != balances_of(now[0])

    commit_timestamp = single.commit_timestamp
    assert at0.tobytes() == AsOf(transfers, accounts).at(ids, t0)[0].tobytes()
    assert at1.tobytes() == AsOf(transfers, accounts).at(ids, t1)[0].tobytes()
    assert stmt.tobytes() == Statements(transfers, accounts).of(ids, t0, t1)[0].tobytes()
    assert integ.tobytes() == Integrals(transfers, accounts, commit_timestamp).of(ids, t0, t1)[0].tobytes()
    assert series.tobytes() == Series(transfers, accounts).of(ids, [t0, tm, t1])[0].tobytes()

    shards = interleaved(node, ids, t0, tm, t1)
    for mine, theirs in zip(answers, shards):
        assert theirs[0].tobytes() == mine[0].tobytes() and theirs[1:] == mine[1:]
