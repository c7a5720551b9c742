"""get_pending_transfers (include/tbgpu.h tbgpu_get_pending_transfers, csrc/k_pending.h): the two-phase
transfers of a window with their state and the record that resolved them.  Rows, states, `count`,
`matched` and `complete` are compared byte for byte with the checker of tests/harness/pending.py
(itself held to the oracle in tests/test_pending_checkers.py)."""
import ctypes
import itertools
import random

import numpy as np
import pytest

from tests.harness.balances import PENDING, POST, VOID, u128
from tests.harness.oracle import OracleEngine
from tests.harness.pending import NS, PendingTransfers
from tests.harness.shard_double import homes_of
from tests.harness.workload import account_id, make_scenario
from tests.test_balance_checkers import CHAIN_FREE, QUERY_SCENARIO
from tests.test_gpu_query import by_id, commit_all, posted_states
from tigerbeetle_amd import _lib
from tigerbeetle_amd._lib import EnginePanic
from tigerbeetle_amd.types import (PENDING_EXPIRED, PENDING_FILTER_DTYPE, PENDING_OPEN, PENDING_POSTED, PENDING_ROWS_MAX,
                                   PENDING_STATES, PENDING_VOIDED, RESULT_DTYPE, TRANSFER_DTYPE, U64_MAX, TransferFlags,
                                   pack_account, pack_transfer)

pytestmark = pytest.mark.gpu

LINKED = int(TransferFlags.linked)
RESOLVED = PENDING_POSTED | PENDING_VOIDED
MASKS = (PENDING_OPEN, PENDING_EXPIRED, PENDING_POSTED, PENDING_VOIDED, PENDING_STATES)
# k_query.h: QUERY_THREADS positions a tile of the selection.  k_pending.h: PENDING_THREADS positions a
# tile of the join, PENDING_TILES tiles a workgroup.
WAVE = 64
TILE = 256
JOIN_WORKGROUP = 256 * 16


def check(engine, checker, evicted=False, **filter):
    """One request: rows, states, matched and complete as the checker has them."""
    want, want_states, matched, resolved = checker.at(**filter)
    got, states, got_matched, complete = engine.get_pending_transfers(**filter)
    assert len(got) == len(want) == len(states), (filter, len(got), len(want))
    assert states.tobytes() == want_states.tobytes(), filter
    assert got.tobytes() == want.tobytes(), filter
    assert (got_matched, complete) == (matched, resolved and not evicted), filter
    return got, states, matched


def ledger_of(sc):
    oracle = OracleEngine(4096, 1 << 15)
    replies = commit_all(sc, oracle)
    transfers, posted = oracle.export_transfers(), oracle.export_posted()
    return dict(sc=sc, replies=replies, transfers=transfers, posted=posted, accounts=oracle.export_accounts(),
                commit_timestamp=oracle.commit_timestamp, checker=PendingTransfers(transfers, posted, oracle.commit_timestamp))


@pytest.fixture(scope="module")
def ledgers():
    """Both scenarios, the oracle that committed each, its exports and the checker over them (never changed)."""
    return {7: ledger_of(make_scenario(7, **CHAIN_FREE)), 2025: ledger_of(make_scenario(2025, **QUERY_SCENARIO))}


def accounts_of(checker):
    """Three accounts that pending transfers name on the debit side and on the credit side."""
    debit = sorted({u128(p, "debit_account_id") for p in checker.pending})
    credit = sorted({u128(p, "credit_account_id") for p in checker.pending})
    return [debit[0], credit[-1], debit[len(debit) // 2]]


def sweep(engine, ledger, seen):
    checker, commit_timestamp = ledger["checker"], ledger["commit_timestamp"]
    stamps = [int(p["timestamp"]) for p in checker.pending]
    first, mid = stamps[0], stamps[len(stamps) // 2]
    nows = (0, first, commit_timestamp, commit_timestamp + 3 * NS, U64_MAX - 1)
    windows = (dict(), dict(timestamp_min=mid), dict(timestamp_max=mid - 1), dict(timestamp_min=stamps[3], timestamp_max=stamps[-4]))
    sides = ((True, True), (True, False), (False, True), (False, False))
    whom = [(0, s) for s in sides[:1]] + [(a, s) for a in accounts_of(checker) for s in sides]

    def limits_for(**filter):
        k = checker.at(**filter)[2]
        return sorted({1, max(k - 1, 1), max(k, 1), k + 1})

    # Every state mask, account choice and clock; the window, direction and limit take turns.
    turn = itertools.cycle(itertools.product(windows, (False, True), range(4)))
    for now, mask, (account, (d, c)) in itertools.product(nows, MASKS, whom):
        win, rev, li = next(turn)
        base = dict(account_id=account, states=mask, debits=d, credits=c, now=now, **win)
        limit = limits_for(**base)[li % len(limits_for(**base))]
        _, states, matched = check(engine, checker, reversed=rev, limit=limit, **base)
        seen["queries"] += 1
        seen["cut"] |= matched > len(states) > 0
        seen["states"] |= set(states.tolist())
        seen["named"] |= account != 0 and matched > 0
    # Any account, every state: the whole product of window, direction, limit and clock.
    for win, rev, now in itertools.product(windows, (False, True), nows):
        base = dict(now=now, **win)
        for limit in limits_for(**base):
            check(engine, checker, reversed=rev, limit=limit, **base)
            seen["queries"] += 1
        k = checker.at(**base)[2]
        got, _, _ = check(engine, checker, reversed=rev, limit=k, out_cap_rows=max(k // 2, 1), **base)
        assert len(got) == max(k // 2, 1)
    check(engine, checker, timestamp_min=stamps[-1] + 1)
    check(engine, checker, account_id=account_id(5000))


@pytest.mark.parametrize("seed", [7, 2025])
def test_single_engine_sweep(seed, ledgers, gpu_engine_factory):
    ledger = ledgers[seed]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    assert commit_all(ledger["sc"], engine) == ledger["replies"]
    assert engine.commit_timestamp == ledger["commit_timestamp"]
    seen = dict(queries=0, cut=False, states=set(), named=False)
    sweep(engine, ledger, seen)
    assert seen["queries"] > 380 and seen["cut"] and seen["named"]
    assert seen["states"] == {PENDING_OPEN, PENDING_EXPIRED, PENDING_POSTED, PENDING_VOIDED}
    # Nothing past `count` rows and states is written.
    k = 5
    f = np.frombuffer(engine.pending_filter(limit=k), dtype=PENDING_FILTER_DTYPE)
    rows = ctypes.create_string_buffer(b"\xAB" * (256 * 8), 256 * 8)
    states = ctypes.create_string_buffer(b"\xCD" * 8, 8)
    res = _lib.tbgpu_query_result()
    assert engine.lib.tbgpu_get_pending_transfers(engine.h, f.ctypes.data, rows, states, 8, ctypes.byref(res)) == _lib.STATUS_OK
    want, want_states, matched, _ = ledger["checker"].at(limit=k)
    assert (res.count, res.matched, res.complete) == (k, matched, 1)
    assert rows.raw == want.tobytes() + b"\xAB" * (256 * 3) and states.raw == want_states.tobytes() + b"\xCD" * 3


def test_open_and_expired_holds_are_the_pending_balances(ledgers, gpu_engine_factory):
    """No checker: on an engine that only committed, an account's debits_pending is the summed amount of
    its OPEN | EXPIRED rows under DEBITS, its credits_pending the same under CREDITS — paged by
    timestamp_min = last + 1."""
    ledger = ledgers[2025]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(ledger["sc"], engine)
    held, pages, accounts = 0, 0, engine.export_accounts()
    for a in accounts:
        for side, column in ((dict(debits=True, credits=False), "debits_pending"), (dict(debits=False, credits=True), "credits_pending")):
            total, after = 0, 0
            while True:
                rows, states, matched, complete = engine.get_pending_transfers(u128(a, "id"), states=PENDING_OPEN | PENDING_EXPIRED,
                                                                               timestamp_min=after, limit=7, **side)
                assert complete and not (states & RESOLVED).any()
                total += sum(u128(r["pending"], "amount") for r in rows)
                pages += 1
                if matched == len(rows):
                    break
                after = int(rows[-1]["pending"]["timestamp"]) + 1
            assert total == u128(a, column), (hex(u128(a, "id")), column)
            held += total > 0
    assert held > 20 and pages > 2 * len(accounts)  # holds on many accounts, and some took several pages


def hand_log(n):
    """n transfer events, every one ok, so log position = event index: pending transfers at the last
    lane of a wave, the last position of a tile and the first of the next; resolutions in the same wave,
    in the next record, in the next tile and at the log's last position — as far as n has room."""
    events = [dict(id=1000 + i, debit_account_id=account_id(i % 4), credit_account_id=account_id(4 + i % 3), amount=1 + i, ledger=1,
                   code=1) for i in range(n)]
    pairs = [(60, 62, POST), (WAVE - 1, WAVE, VOID), (10, TILE + 1, POST), (TILE - 1, n - 1, POST), (TILE, TILE + 44, VOID),
             (TILE - 2, None, 0), (WAVE, None, 0), (JOIN_WORKGROUP - 1, JOIN_WORKGROUP, POST), (100, JOIN_WORKGROUP + 1, VOID)]
    placed, used = [], set()
    for p, r, flag in pairs:
        if p >= n or p in used:
            continue
        if r is not None and (r >= n or r <= p or r in used):
            r = None  # no room: the pending transfer alone
        events[p].update(flags=PENDING, timeout=p % 3)
        used.add(p)
        if r is not None:
            amount = events[p]["amount"] - (1 if p % 2 == 0 else 0) if flag == POST else 0
            events[r] = dict(id=1000 + r, pending_id=1000 + p, amount=amount, flags=flag)
            used.add(r)
        placed.append((p, r))
    return [pack_transfer(**e) for e in events], placed


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 600, JOIN_WORKGROUP - 1, JOIN_WORKGROUP, JOIN_WORKGROUP + 2])
def test_wave_tile_and_workgroup_edges(n, gpu_engine_factory):
    engine = gpu_engine_factory(transfers_max=1 << 13)
    oracle = OracleEngine(64, 1 << 13)
    accounts = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(8))
    assert engine.commit(128, 10**12, accounts) == oracle.commit(128, 10**12, accounts) == b""
    events, placed = hand_log(n)
    ts = 10**12 + 10**6
    assert engine.commit_many(129, [ts], [b"".join(events)]) == [oracle.commit(129, ts, b"".join(events))] == [b""]
    assert engine.stats()["log_used"] == n  # position = event index
    assert engine.export_transfers().tobytes() == oracle.export_transfers().tobytes()
    checker = PendingTransfers(oracle.export_transfers(), oracle.export_posted(), oracle.commit_timestamp)
    first = ts - n + 1
    assert [int(p["timestamp"]) - first for p in checker.pending] == sorted(p for p, _ in placed)
    assert len(placed) >= (4 if n < TILE + 2 else 7)
    rows, states, _ = check(engine, checker)
    where = {int(r["pending"]["timestamp"]) - first: (int(r["resolution"]["timestamp"]) - first if st & RESOLVED else None)
             for r, st in zip(rows, states)}
    assert where == dict(placed)  # every planted resolution was found where it was put
    for mask, rev, limit in itertools.product(MASKS, (False, True), (1, 2, len(placed))):
        check(engine, checker, states=mask, reversed=rev, limit=limit, now=ts + 2 * NS)
    for p, r in placed:  # a window of one pending transfer, wherever its resolution lies
        got, _, matched = check(engine, checker, timestamp_min=first + p, timestamp_max=first + p)
        assert matched == 1 and (int(got[0]["resolution"]["timestamp"]) == first + r if r is not None else True)


def test_the_set_at_its_largest(gpu_engine_factory):
    """4,096 pending transfers, all posted: a request for more returns TBGPU_PENDING_ROWS_MAX rows, each
    with its resolution; the second page gets the last one."""
    n = PENDING_ROWS_MAX + 1
    engine = gpu_engine_factory(transfers_max=1 << 14)
    accounts = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(8))
    assert engine.commit(128, 10**12, accounts) == b""
    body = b"".join(pack_transfer(id=10**6 + i, debit_account_id=account_id(i % 4), credit_account_id=account_id(4 + i % 3),
                                  amount=10 + i, ledger=1, code=1, flags=PENDING, timeout=i % 2) for i in range(n))
    assert engine.commit(129, 10**12 + 10**6, body) == b""
    order = list(range(n))
    random.Random(4).shuffle(order)  # the posts in another order than their pending transfers
    body = b"".join(pack_transfer(id=2 * 10**6 + i, pending_id=10**6 + i, amount=10 + i - (i % 3 == 0), flags=POST) for i in order)
    assert engine.commit(129, 10**12 + 2 * 10**6, body) == b""
    checker = PendingTransfers(engine.export_transfers(), engine.export_posted(), engine.commit_timestamp)
    assert len(checker.pending) == len(checker.resolving) == n
    rows, states, matched = check(engine, checker, limit=8190, out_cap_rows=8190)
    assert len(rows) == PENDING_ROWS_MAX and matched == n and (states == PENDING_POSTED).all()
    assert (rows["resolution"]["pending_id_lo"] == rows["pending"]["id_lo"]).all()
    last = int(rows[-1]["pending"]["timestamp"])
    rows, _, matched = check(engine, checker, timestamp_min=last + 1, limit=8190, out_cap_rows=8190)
    assert len(rows) == matched == 1 and int(rows[0]["resolution"]["pending_id_lo"]) == 10**6 + n - 1
    rows, _, _ = check(engine, checker, reversed=True, limit=8190, out_cap_rows=8190)
    assert len(rows) == PENDING_ROWS_MAX and int(rows[0]["pending"]["id_lo"]) == 10**6 + n - 1
    check(engine, checker, states=PENDING_OPEN | PENDING_EXPIRED | PENDING_VOIDED)


def test_dead_records_never_match_or_resolve(gpu_engine_factory):
    """A failed post, a duplicate post that returned pending_transfer_already_posted, and a rolled-back
    chain that held a pending transfer and its post: their log positions hold records that name a
    pending transfer, and none of them matches or resolves."""
    engine = gpu_engine_factory(transfers_max=1 << 12)
    oracle = OracleEngine(64, 1 << 12)
    accounts = b"".join(pack_account(id=i, ledger=1, code=1) for i in (1, 2, 3))
    assert engine.commit(128, 10**12, accounts) == oracle.commit(128, 10**12, accounts) == b""
    plain = dict(debit_account_id=1, credit_account_id=2, ledger=1, code=1)
    events = [
        pack_transfer(id=10, amount=100, flags=PENDING, **plain),
        pack_transfer(id=11, amount=50, flags=PENDING, timeout=1, **plain),
        pack_transfer(id=20, pending_id=10, amount=101, flags=POST),               # exceeds_pending_transfer_amount
        pack_transfer(id=21, pending_id=10, amount=60, flags=POST),                # ok
        pack_transfer(id=22, pending_id=10, amount=60, flags=POST),                # pending_transfer_already_posted
        pack_transfer(id=30, amount=7, flags=PENDING | LINKED, **plain),           # a chain that rolls back ...
        pack_transfer(id=31, pending_id=30, flags=POST | LINKED),
        pack_transfer(id=32, amount=1, debit_account_id=3, credit_account_id=3, ledger=1, code=1),  # ... here
        pack_transfer(id=40, pending_id=11, flags=VOID),                           # ok
        pack_transfer(id=41, pending_id=11, flags=VOID),                           # pending_transfer_already_voided
        pack_transfer(id=50, amount=9, flags=PENDING, **plain),
    ]
    ts = 10**12 + 1000
    reply = engine.commit(129, ts, b"".join(events))
    assert reply == oracle.commit(129, ts, b"".join(events))
    assert np.frombuffer(reply, dtype=RESULT_DTYPE)["index"].tolist() == [2, 4, 5, 6, 7, 9]
    assert engine.stats()["log_used"] > len(engine.export_transfers())
    checker = PendingTransfers(oracle.export_transfers(), oracle.export_posted(), oracle.commit_timestamp)
    rows, states, matched = check(engine, checker)
    assert matched == 3 and states.tolist() == [PENDING_POSTED, PENDING_VOIDED, PENDING_OPEN]
    assert [u128(r["pending"], "id") for r in rows] == [10, 11, 50]
    assert [u128(r["resolution"], "id") for r in rows] == [21, 40, 0]
    for mask, rev in itertools.product(MASKS, (False, True)):
        check(engine, checker, states=mask, reversed=rev, now=ts + 5 * NS)


def test_restart_and_unordered_log(gpu_engine_factory):
    """tbgpu_load_transfers of pending records, one with posted state 1 and no post record: POSTED, a
    zero resolution, complete = 0.  The post record loaded afterwards, behind records with later
    timestamps: the answer is ordered by timestamp and resolved."""
    oracle = OracleEngine(64, 1 << 10)
    accounts = b"".join(pack_account(id=i, ledger=1, code=1) for i in (1, 2))
    assert oracle.commit(128, 10**12, accounts) == b""
    plain = dict(debit_account_id=1, credit_account_id=2, ledger=1, code=1)
    events = [pack_transfer(id=10 + i, amount=100 + i, flags=PENDING, timeout=i % 2, **plain) for i in range(6)]
    events += [pack_transfer(id=20, pending_id=11, amount=70, flags=POST), pack_transfer(id=21, pending_id=14, flags=VOID)]
    assert oracle.commit(129, 10**12 + 1000, b"".join(events)) == b""
    transfers = oracle.export_transfers()
    transfers = transfers[np.argsort(transfers["timestamp"])]
    states = posted_states(transfers, oracle.export_posted())
    assert states.tolist() == [0, 1, 0, 0, 2, 0, 0, 0]
    engine = gpu_engine_factory(transfers_max=1 << 12)
    engine.load_accounts(oracle.export_accounts())
    engine.set_commit_timestamp(oracle.commit_timestamp)
    first = np.array([5, 1, 3, 0, 4, 2])  # the pending records, out of timestamp order
    engine.load_transfers(transfers[first], states[first])
    checker = PendingTransfers(engine.export_transfers(), engine.export_posted(), engine.commit_timestamp)
    rows, got_states, matched, complete = engine.get_pending_transfers()
    assert matched == 6 and not complete
    assert got_states.tolist() == [PENDING_OPEN, PENDING_POSTED, PENDING_OPEN, PENDING_OPEN, PENDING_VOIDED, PENDING_OPEN]
    assert rows["resolution"].tobytes() == bytes(128 * 6) and rows["pending"].tobytes() == transfers[:6].tobytes()
    for rev, limit, mask in itertools.product((False, True), (1, 2, 6), MASKS):
        check(engine, checker, reversed=rev, limit=limit, states=mask, now=10**12 + 1000 + NS)
    assert engine.get_pending_transfers(states=PENDING_OPEN)[3]  # no resolved row returned: complete
    engine.load_transfers(transfers[[7, 6]], states[[7, 6]])  # the void, then the post
    assert engine.export_transfers().tobytes() == oracle.export_transfers().tobytes()
    checker = PendingTransfers(oracle.export_transfers(), oracle.export_posted(), oracle.commit_timestamp)
    for keys_max in (0, 256):
        engine.query_keys_max(keys_max)
        rows, got_states, _ = check(engine, checker)
        assert [u128(r["resolution"], "id") for r in rows] == [0, 20, 0, 0, 21, 0]
        for rev, limit, mask in itertools.product((False, True), (1, 2, 6), MASKS):
            check(engine, checker, reversed=rev, limit=limit, states=mask, now=10**12 + 1000 + NS)


def test_unordered_log_over_several_rounds(gpu_engine_factory):
    """The newer half committed, the older half loaded shuffled: pending transfers and their
    resolutions on either side of the seam, and more matches than a round's keys."""
    kw = dict(n_accounts=8, n_transfer_batches=24, batch_len=(100, 300), p_pending=0.4, p_dup=0.05, p_linked=0.05,
              p_limit=0.0, p_balancing=0.0, p_invalid=0.05, id_space=1 << 40)
    sa = make_scenario(31, p_post_void=0.25, **kw)
    last = sa.steps[-1][2]
    sb = make_scenario(32, p_post_void=0.25, start_ts=last + 10**9, **kw)
    oracle = OracleEngine(64, 1 << 15)
    engine1 = gpu_engine_factory(transfers_max=1 << 15)
    engine2 = gpu_engine_factory(transfers_max=1 << 15)
    commit_all(sa, oracle, engine1, engine2, steps=[s for s in sa.steps if s[1] == 128])
    commit_all(sa, oracle, engine1, steps=[s for s in sa.steps if s[1] == 129])
    half_a = engine1.export_transfers()
    states = posted_states(half_a, engine1.export_posted())
    commit_all(sb, oracle, engine2, steps=[s for s in sb.steps if s[1] == 129])
    order = np.random.default_rng(5).permutation(len(half_a))
    engine2.load_transfers(half_a[order], states[order])
    assert engine2.export_transfers().tobytes() == oracle.export_transfers().tobytes()
    checker = PendingTransfers(oracle.export_transfers(), oracle.export_posted(), oracle.commit_timestamp)
    n = len(checker.pending)
    assert n > 2 * 256  # three rounds of keys at 256
    for keys_max in (0, 256):
        engine2.query_keys_max(keys_max)
        for rev, limit in itertools.product((False, True), (3, n // 2, n - 3, PENDING_ROWS_MAX)):
            _, got_states, _ = check(engine2, checker, reversed=rev, limit=limit)
        assert set(got_states.tolist()) == {PENDING_OPEN, PENDING_EXPIRED, PENDING_POSTED, PENDING_VOIDED}
        check(engine2, checker, states=RESOLVED, timestamp_min=last - 10**9, timestamp_max=last + 2 * 10**9)
        check(engine2, checker, account_id=u128(checker.pending[0], "debit_account_id"), credits=False, now=last)


def test_eviction(ledgers, gpu_engine_factory):
    ledger = ledgers[2025]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(ledger["sc"], engine)
    engine.checkpoint_delta()
    assert engine.evict_transfers(2500) > 0
    resident = engine.export_transfers()
    assert 0 < len(resident) < len(ledger["transfers"])
    checker = PendingTransfers(resident, engine.export_posted(), engine.commit_timestamp)
    assert 0 < len(checker.pending) < len(ledger["checker"].pending)
    for mask, rev, limit in itertools.product(MASKS, (False, True), (1, 25, PENDING_ROWS_MAX)):
        check(engine, checker, evicted=True, states=mask, reversed=rev, limit=limit)
    # A pending transfer comes back alone, its post evicted with it: POSTED, and no resolution resident.
    here = set(resident["timestamp"].tolist())
    gone = [(p, r) for p, r in ((p, ledger["checker"].resolving.get(u128(p, "id"))) for p in ledger["checker"].pending)
            if r is not None and int(p["timestamp"]) not in here and int(r["timestamp"]) not in here]
    assert gone
    back = np.array([gone[0][0]], dtype=TRANSFER_DTYPE)
    engine.load_transfers(back, posted_states(back, ledger["posted"]))
    checker = PendingTransfers(engine.export_transfers(), engine.export_posted(), engine.commit_timestamp)
    rows, states, _ = check(engine, checker, evicted=True)
    assert rows[0]["pending"].tobytes() == back.tobytes() and states[0] & RESOLVED and not rows[0]["resolution"]["timestamp"]
    assert not checker.at()[3]


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=["node2", "node3"])
def test_node(devices, ledgers, gpu_engine_factory):
    ledger = ledgers[2025]
    checker = ledger["checker"]
    engine = gpu_engine_factory(accounts_max=4096, transfers_max=1 << 14, pass_events_max=2048, pass_batches_max=16,
                                devices=devices)
    assert commit_all(ledger["sc"], engine) == ledger["replies"]
    rows, states, _ = check(engine, checker)
    resolved = rows[(states & RESOLVED) != 0]
    ids = lambda part: np.stack([resolved[part]["id_lo"], resolved[part]["id_hi"]], axis=1)
    away = homes_of(ids("pending"), len(devices)) != homes_of(ids("resolution"), len(devices))
    assert away.any() and not away.all()  # resolutions on the pending transfer's shard and on another
    nows = (0, ledger["commit_timestamp"] + 3 * NS, U64_MAX - 1)
    accounts = [0] + accounts_of(checker)
    for mask, account, rev, now in itertools.product(MASKS, accounts, (False, True), nows):
        k = checker.at(account_id=account, states=mask, now=now)[2]
        for limit in {1, max(k - 1, 1), k + 1}:
            check(engine, checker, account_id=account, states=mask, reversed=rev, now=now, limit=limit)
    mid = int(checker.pending[len(checker.pending) // 2]["timestamp"])
    check(engine, checker, timestamp_min=mid, limit=50, out_cap_rows=20)
    check(engine, checker, timestamp_max=mid, reversed=True, states=RESOLVED)


def test_read_only_and_allocation_free(ledgers, gpu_engine_factory):
    """40 calls around which the allocation counts, commit_timestamp, the exports and the commit-path
    counters stand still; one more inside an asynchronous write-back; then the next commit answers as
    the twin's."""
    ledger = ledgers[2025]
    sc = ledger["sc"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    twin = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, engine, twin, steps=sc.steps[:-1])
    resident = engine.export_transfers()
    checker = PendingTransfers(resident, engine.export_posted(), engine.commit_timestamp)
    before = (engine.commit_timestamp, engine.export_accounts().tobytes(), resident.tobytes(), engine.export_posted().tobytes())
    rng = random.Random(3)
    accounts = [0] + accounts_of(checker)
    allocations, live = engine.lib.tbgpu_debug_allocations(), engine.lib.tbgpu_debug_live()
    stats = engine.stats()
    for _ in range(40):
        engine.get_pending_transfers(rng.choice(accounts), states=rng.choice(MASKS), reversed=rng.random() < 0.5,
                                     now=rng.choice((0, 1, engine.commit_timestamp + NS)), limit=rng.choice((1, 30, PENDING_ROWS_MAX)))
    assert (engine.lib.tbgpu_debug_allocations(), engine.lib.tbgpu_debug_live()) == (allocations, live)
    after = engine.stats()
    assert all(after[k] == stats[k] for k in ("passes", "events", "transfers", "accounts", "log_used"))
    assert before == (engine.commit_timestamp, engine.export_accounts().tobytes(), engine.export_transfers().tobytes(),
                      engine.export_posted().tobytes())
    # One between an asynchronous write-back's start and its wait leaves the delta alone.
    caps = (1 << 14, 1 << 14, 1 << 14)
    engine.checkpoint_delta_async(caps)
    allocations = engine.lib.tbgpu_debug_allocations()
    check(engine, checker)
    assert engine.lib.tbgpu_debug_allocations() == allocations
    delta = engine.checkpoint_delta_wait()
    sync = twin.checkpoint_delta(caps)
    assert len(delta.transfers) == len(resident)
    assert delta.transfers.tobytes() == sync.transfers.tobytes() and delta.posted.tobytes() == sync.posted.tobytes()
    assert by_id(delta.accounts) == by_id(sync.accounts) and delta.created_after == sync.created_after
    # ... and the next commit still answers as the twin and the oracle did.
    _, op, ts, batch = sc.steps[-1]
    assert engine.commit(op, ts, b"".join(batch)) == twin.commit(op, ts, b"".join(batch)) == ledger["replies"][-1]
    check(engine, ledger["checker"])
    assert engine.export_transfers().tobytes() == ledger["transfers"].tobytes()
    assert engine.export_posted().tobytes() == twin.export_posted().tobytes()


def test_after_commit_device_async_without_a_sync(gpu_engine_factory):
    """The call drains a pending tbgpu_commit_device_async itself."""
    engine = gpu_engine_factory(transfers_max=1 << 12)
    oracle = OracleEngine(64, 1 << 12)
    accounts = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(8))
    assert engine.commit(128, 10**12, accounts) == oracle.commit(128, 10**12, accounts) == b""
    events, placed = hand_log(600)
    body = b"".join(events)
    ts = 10**12 + 1000
    assert oracle.commit(129, ts, body) == b""
    window = engine.log_window(600)
    engine.to_device(window, np.frombuffer(body, dtype=np.uint8))
    res, rb = engine.alloc(600 * 8), engine.alloc(4)
    engine.commit_device_async(129, [ts], [600], window, res, rb)
    checker = PendingTransfers(oracle.export_transfers(), oracle.export_posted(), oracle.commit_timestamp)
    _, states, matched = check(engine, checker)
    assert matched == len(placed) and (states & RESOLVED).any()
    assert int(engine.to_host(rb, 4).view(np.uint32)[0]) == 0
    engine.free(res)
    engine.free(rb)


def test_on_an_engine_a_device_panic_stopped(gpu_engine_factory):
    """tests/test_gpu_alloc.py's way to a device panic (a post whose checked `-=` traps after the setup
    action zeroed the pending balance).  The stopped engine still answers."""
    engine = gpu_engine_factory()
    accounts = b"".join(pack_account(id=i, ledger=1, code=1) for i in (1, 2, 3))
    assert engine.commit(128, 10, accounts) == b""
    plain = dict(debit_account_id=1, credit_account_id=2, ledger=1, code=1)
    assert engine.commit(129, 20, pack_transfer(id=10, amount=100, flags=PENDING, **plain)) == b""
    assert engine.commit(129, 25, pack_transfer(id=12, amount=7, flags=PENDING, timeout=1, **plain)
                         + pack_transfer(id=13, pending_id=12, flags=VOID)) == b""
    healthy = engine.get_pending_transfers()
    assert healthy[1].tolist() == [PENDING_OPEN, PENDING_VOIDED] and healthy[2:] == (2, True)
    engine.set_balances(1, 0, 0, 0, 0)
    with pytest.raises(EnginePanic):
        engine.commit(129, 30, pack_transfer(id=11, pending_id=10, flags=POST))
    with pytest.raises(EnginePanic, match="stopped"):
        engine.commit(129, 40, pack_transfer(id=14, amount=1, **plain))
    checker = PendingTransfers(engine.export_transfers(), engine.export_posted(), engine.commit_timestamp)
    allocations = engine.lib.tbgpu_debug_allocations()
    for mask, rev in itertools.product(MASKS, (False, True)):
        check(engine, checker, states=mask, reversed=rev)
    rows, states, matched, complete = engine.get_pending_transfers(1, credits=False)
    assert matched == 2 and u128(rows[1]["resolution"], "id") == 13 and states[1] == PENDING_VOIDED
    assert engine.lib.tbgpu_debug_allocations() == allocations


def raw_filter(**fields):
    f = np.zeros(1, dtype=PENDING_FILTER_DTYPE)
    base = dict(limit=3, flags=PENDING_STATES | 3)
    base.update(fields)
    for k, v in base.items():
        f[k] = v
    return f


def test_invalid_filters(ledgers, gpu_engine_factory):
    ledger = ledgers[7]
    engine = gpu_engine_factory(transfers_max=1 << 12)
    empty = engine.get_pending_transfers_raw(raw_filter().tobytes())  # an empty engine
    assert len(empty[0]) == 0 and empty[2:] == (0, True)
    commit_all(ledger["sc"], engine)
    a = max(accounts_of(ledger["checker"]), key=lambda x: ledger["checker"].at(x)[2])
    named = dict(account_id_lo=a & U64_MAX, account_id_hi=a >> 64)
    valid = engine.get_pending_transfers_raw(raw_filter(**named).tobytes())
    assert len(valid[0]) == 3 and valid[2] > 3 and valid[3]
    any_account = engine.get_pending_transfers_raw(raw_filter().tobytes())
    assert any_account[2] == len(ledger["checker"].pending)
    # With account id 0 the side bits are ignored.
    assert engine.get_pending_transfers_raw(raw_filter(flags=PENDING_STATES).tobytes())[2] == any_account[2]
    reserved = np.zeros(16, dtype=np.uint8)
    reserved[15] = 1
    invalid = [dict(account_id_lo=U64_MAX, account_id_hi=U64_MAX), dict(flags=PENDING_STATES, **named), dict(flags=3),
               dict(flags=PENDING_STATES | 3 | 8), dict(flags=PENDING_STATES | 3 | 1 << 31), dict(reserved=reserved),
               dict(timestamp_min=U64_MAX), dict(timestamp_max=U64_MAX), dict(now=U64_MAX), dict(timestamp_min=9, timestamp_max=8),
               dict(limit=0)]
    for fields in invalid:
        rows, states, matched, complete = engine.get_pending_transfers_raw(raw_filter(**fields).tobytes())
        assert len(rows) == 0 and matched == 0 and complete, fields
    rows, states, matched, complete = engine.get_pending_transfers_raw(raw_filter().tobytes(), 0)  # no room: matched stays
    assert len(rows) == 0 and matched == any_account[2]
    assert engine.get_pending_transfers_raw(raw_filter(now=U64_MAX - 1, timestamp_min=1, timestamp_max=U64_MAX - 1).tobytes())[2] == any_account[2]
    # NULL arguments.
    fn = engine.lib.tbgpu_get_pending_transfers
    f = raw_filter()
    sentinel = b"\xAB" * 2560
    out = ctypes.create_string_buffer(sentinel, len(sentinel))
    st = ctypes.create_string_buffer(b"\xCD" * 10, 10)
    res = _lib.tbgpu_query_result(count=77, complete=77, matched=77)
    untouched = lambda: out.raw == sentinel and st.raw == b"\xCD" * 10 and (res.count, res.complete, res.matched) == (77, 77, 77)
    assert fn(engine.h, None, out, st, 10, ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, f.ctypes.data, None, st, 10, ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, f.ctypes.data, out, None, 10, ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, f.ctypes.data, out, st, 10, None) == _lib.STATUS_INVALID and out.raw == sentinel
    bad = raw_filter(limit=0)
    assert fn(engine.h, bad.ctypes.data, out, st, 10, ctypes.byref(res)) == _lib.STATUS_OK
    assert out.raw == sentinel and st.raw == b"\xCD" * 10 and (res.count, res.matched, res.complete) == (0, 0, 1)
    assert fn(engine.h, f.ctypes.data, out, st, 10, ctypes.byref(res)) == _lib.STATUS_OK
    assert res.count == 3 and out.raw == any_account[0].tobytes() + sentinel[768:]
    assert st.raw == any_account[1].tobytes() + b"\xCD" * 7
