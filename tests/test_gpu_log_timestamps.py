"""The timestamp plane (csrc/tb_device.h tb_log_ts): an in-place create keeps its event's bytes, its
timestamp lives in Tables.xts, and every reader of the log takes a record's timestamp — and hands a
record to a caller — through tb_log_ts / tb_log_load.  So an engine that committed in place must
answer every read entry point with the bytes of an engine that committed the same prepares through
`commit` (kernel 1 stores whole records there, timestamp in the field), and with the oracle's where
the harness has one: at wave, tile and prepare edges, across calls, in a log that mixes both kinds of
record with loaded ones, after an eviction moved the plane with the log, and on a node whose homes
commit in place."""
import numpy as np
import pytest

from tests.harness.asof import AsOf
from tests.harness.oracle import OracleEngine
from tests.harness.pending import PendingTransfers
from tests.harness.workload import Scenario, account_id, run_oracle
from tests.test_gpu_differential import assert_same_state
from tests.test_gpu_inplace import run_inplace
from tigerbeetle_amd.types import (CreateTransferResult, TRANSFER_DTYPE, TransferFlags as TF, U64_MAX, pack_account,
                                   pack_transfer)

pytestmark = pytest.mark.gpu

NS = 1_000_000_000
N_ACCOUNTS = 64
T0 = 10**12
PREPARES = (1, 63, 64, 65, 255, 256, 257, 300)  # a wave edge, a tile edge, a prepare boundary inside a wave


def accounts_step(ts=T0, n=N_ACCOUNTS):
    return ("commit", 128, ts, [pack_account(id=account_id(i), ledger=1 + i % 2, code=1 + i % 7, user_data_64=i % 5)
                                for i in range(n)])


def create(tid, k, flags=0, timeout=0, amount=None, **kw):
    """A create between two accounts of one ledger (account i is on ledger 1 + i % 2)."""
    dr = (2 * k) % N_ACCOUNTS
    cr = (2 * k + 2 + 4 * (k % 5)) % N_ACCOUNTS
    ev = dict(id=tid, debit_account_id=account_id(dr), credit_account_id=account_id(cr), ledger=1 + dr % 2,
              amount=1 + k % 97 if amount is None else amount, code=1 + k % 3, flags=int(flags), timeout=timeout,
              user_data_128=k % 4, user_data_64=k % 3, user_data_32=k % 2)
    ev.update(kw)
    return pack_transfer(**ev)


def edge_scenario():
    """Creates, pendings, posts and voids of earlier prepares' pendings, a linked chain and failing events
    in prepares of PREPARES events.  Returns (scenario, transfer ids, first and last in-place timestamp)."""
    sc = Scenario()
    sc.steps.append(accounts_step())
    ts, tid, ids, pend = T0 + 10, 1, [], []
    first_ts = None
    for b, L in enumerate(PREPARES):
        events = []
        new_pend = []
        for k in range(L):
            r = (7 * b + k) % 16
            if r == 3 and pend:  # post or void a pending transfer of an earlier prepare
                p = pend.pop(0)
                events.append(pack_transfer(id=tid, pending_id=p, flags=int(TF.post_pending_transfer if k % 2 else
                                                                         TF.void_pending_transfer)))
            elif r == 5:
                events.append(create(tid, k, TF.pending, timeout=(0, 1, 1000)[k % 3]))
                new_pend.append(tid)
            elif r == 9 and k + 2 < L:  # a linked chain of two: both commit
                events.append(create(tid, k, TF.linked))
            elif r == 11:  # fails: no such account
                events.append(create(tid, k, debit_account_id=account_id(N_ACCOUNTS + 3)))
            elif r == 13:  # fails: its timestamp is not zero
                events.append(create(tid, k, timestamp=7))
            elif r == 14 and ids:  # fails: exists
                events.append(create(ids[len(ids) // 2], len(ids) // 2))
                tid -= 1
            elif r == 15 and k + 2 < L:  # a chain whose second member fails: both roll back
                events.append(create(tid, k, TF.linked))
                tid += 1
                events.append(create(tid, k, ledger=9))
            else:
                events.append(create(tid, k))
            ids.append(tid)
            tid += 1
        events = events[:L]
        pend += new_pend
        ts += 1 + len(events) + (3 * NS if b == 4 else 0)
        if first_ts is None:
            first_ts = ts - len(events) + 1
        sc.steps.append(("commit", 129, ts, events))
    return sc, ids, first_ts, ts


def rows(x):
    """A comparable form of an entry point's answer: arrays as bytes."""
    if isinstance(x, np.ndarray):
        return x.tobytes()
    if isinstance(x, (tuple, list)):
        return tuple(rows(v) for v in x)
    return x


def answers(engine, ids, windows, lookup_ts, delta=True):
    """Every read entry point's answer as bytes.  windows: (timestamp_min, timestamp_max) pairs."""
    id_rows = np.array([[i & U64_MAX, i >> 64] for i in ids], dtype=np.uint64)
    accts = [account_id(i) for i in (0, 1, 2, 7, 10, 33, N_ACCOUNTS + 3)]
    out = {"fetch": rows(engine.fetch_transfers(id_rows)),
           "lookup": engine.commit(131, lookup_ts, id_rows[:8000].tobytes()),
           "export": rows(engine.export_transfers()), "posted": rows(engine.export_posted()),
           "accounts": rows(engine.export_accounts())}
    for lo, hi in windows:
        w = dict(timestamp_min=lo, timestamp_max=hi)
        k = "%d..%d " % (lo, hi)
        for a in accts[:4]:
            for rev in (False, True):
                out[k + "account %d %d" % (a, rev)] = rows(engine.get_account_transfers(a, reversed=rev, **w))
                out[k + "balances %d %d" % (a, rev)] = rows(engine.get_account_balances(a, reversed=rev, **w))
        out[k + "debits"] = rows(engine.get_account_transfers(accts[0], credits=False, limit=5, **w))
        out[k + "fields"] = rows(engine.query_transfers(ledger=1, code=2, **w))
        out[k + "fields rev"] = rows(engine.query_transfers(user_data_64=1, reversed=True, limit=40, **w))
        out[k + "many"] = rows(engine.get_account_transfers_many(
            [engine.account_filter(a, reversed=bool(j % 2), **w) for j, a in enumerate(accts)]))
        out[k + "changes"] = rows(engine.get_change_events(limit=4000, **w))
        out[k + "pending"] = rows(engine.get_pending_transfers(**w))
        out[k + "pending of"] = rows(engine.get_pending_transfers(accts[1], reversed=True, now=hi or 0, **w))
        out[k + "statements"] = rows(engine.get_account_statements(accts, lo, hi))
        out[k + "ledgers"] = rows(engine.get_ledger_balances([1, 2, 0, 9], lo))
        out[k + "at"] = rows(engine.lookup_accounts_at(accts, lo))
        out[k + "at hi"] = rows(engine.lookup_accounts_at(accts, hi))
    if delta:
        d = engine.checkpoint_delta()
        order = np.argsort(d.accounts, order=("id_hi", "id_lo"))
        out["delta"] = (rows(d.accounts[order]), rows(np.asarray(d.accounts_before)[order]), rows(d.transfers),
                        rows(d.posted), d.created_after)
    return out


def assert_same_answers(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], "%s differs" % k


def edge_windows(first, last):
    w = [(0, 0)]
    for t in (first, last):
        for d in (-1, 0, 1):
            w += [(t + d, 0), (1, t + d)]
    return w + [(first, last), (first + 1, last - 1)]


def check_spec(engine, first, last):
    """The harness's own definitions of two queries over the engine's exported state."""
    resident, accounts = engine.export_transfers(), engine.export_accounts()
    spec = PendingTransfers(resident, engine.export_posted(), engine.commit_timestamp)
    asof = AsOf(resident, accounts)
    ids = [account_id(i) for i in (0, 1, 2, 7, 10, 33)]
    for t in (first - 1, first, first + 1, last - 1, last, last + 1):
        got = engine.get_pending_transfers(timestamp_min=t, now=last)
        want = spec.at(timestamp_min=t, now=last)
        assert rows(got[0]) == rows(want[0]) and rows(got[1]) == rows(want[1]) and got[2] == want[2], t
        got = engine.lookup_accounts_at(ids, t)
        want = asof.at(ids, t)
        assert rows(got[0]) == rows(want[0]) and got[1] == want[1], t


OPTS = dict(accounts_max=4096, transfers_max=1 << 14, pass_events_max=8192, pass_batches_max=4)


def test_in_place_against_copy(gpu_engine_factory):
    sc, ids, first, last = edge_scenario()
    oracle = OracleEngine(4096, 1 << 14)
    expected = run_oracle(sc, oracle)
    ok = sum(L for L in PREPARES) - sum(len(r) // 8 for r in expected[1:])
    assert ok > 600 and any(expected[1:])  # most events commit, and some fail
    placed, copied = gpu_engine_factory(**OPTS), gpu_engine_factory(**OPTS)
    assert run_inplace(sc, placed) == expected
    assert run_oracle(sc, copied) == expected
    assert_same_state(oracle, placed)
    assert_same_state(oracle, copied)
    assert placed.stats()["dependent_events"] > 0  # the ordered path stored records in the same window
    id_rows = np.array([[i & U64_MAX, i >> 64] for i in ids], dtype=np.uint64)
    want, state = oracle.fetch_transfers(id_rows)
    got = placed.fetch_transfers(id_rows)
    assert rows(got[0][got[1] != 0]) == rows(want[state != 0]) and rows(got[1]) == rows(state)
    windows = edge_windows(first, last)
    assert_same_answers(answers(placed, ids, windows, last + 10), answers(copied, ids, windows, last + 10))
    check_spec(placed, first, last)


@pytest.mark.parametrize("later", ["in place", "host commit"])
def test_pending_created_in_place_resolved_later(later, gpu_engine_factory):
    """p.timestamp + timeout one below, at and one above the resolving event's timestamp: the pending
    record's timestamp is read from the plane by kernel 1 and by the ordered path."""
    sc = Scenario()
    sc.steps.append(accounts_step())
    n, timeout = 130, 2
    t1 = T0 + 1000  # the pendings' prepare: event k's timestamp is t1 - n + 1 + k
    sc.steps.append(("commit", 129, t1, [create(1 + k, k, TF.pending, timeout=timeout if k % 2 else 0)
                                         for k in range(n)]))
    second = []
    for k in range(n):  # post, void, and a same-prepare pair on one pending id (the ordered path)
        f = TF.post_pending_transfer if k % 3 else TF.void_pending_transfer
        second.append(pack_transfer(id=1000 + k, pending_id=1 + (k if k % 7 else k - 1 if k else 0), flags=int(f)))
    for shift in (-1, 0, 1):
        # Event j = 65 resolves pending 65 (timeout 2 s): its timestamp against that pending's expiry.
        j = 65
        expiry = t1 - n + 1 + j + timeout * NS
        t2 = expiry + shift + (n - 1 - j)  # event j's timestamp = t2 - n + 1 + j = expiry + shift
        steps = sc.steps[:2] + [("commit", 129, t2, second)]
        one = Scenario()
        one.steps = steps
        oracle = OracleEngine(4096, 1 << 12)
        expected = run_oracle(one, oracle)
        engine = gpu_engine_factory(**OPTS)
        first_two = Scenario()
        first_two.steps = steps[:2]
        assert run_inplace(first_two, engine) == expected[:2]
        if later == "in place":
            last = Scenario()
            last.steps = steps[2:]
            got = run_inplace(last, engine)[0]
        else:
            got = engine.commit(129, t2, b"".join(second))
        assert got == expected[2], shift
        codes = np.frombuffer(expected[2], dtype=np.uint32).reshape(-1, 2)
        at_j = codes[codes[:, 0] == j]
        assert (len(at_j) == 1 and at_j[0, 1] == CreateTransferResult.pending_transfer_expired) == (shift >= 0)
        assert_same_state(oracle, engine)
        check_spec(engine, t1 - n + 1, t2)


def test_mixed_log(gpu_engine_factory):
    """A copy-committed prepare, an in-place one and loaded records in one log: one window query across
    all three kinds of record."""
    oracle = OracleEngine(4096, 1 << 12)
    engine = gpu_engine_factory(**OPTS)
    sc = Scenario()
    sc.steps.append(accounts_step())
    a = [create(1 + k, k, TF.pending if k % 5 == 0 else 0) for k in range(100)]
    b = [create(200 + k, k) for k in range(100)]
    sc.steps.append(("commit", 129, T0 + 200, a))
    expected = run_oracle(sc, oracle)
    assert run_oracle(sc, engine) == expected  # through `commit`: whole records, timestamp in the field
    placed = Scenario()
    placed.steps = [("commit", 129, T0 + 400, b)]
    assert run_inplace(placed, engine) == run_oracle(placed, oracle)
    loaded = np.frombuffer(b"".join(create(500 + k, k, timestamp=T0 + 500 + k) for k in range(50)), dtype=TRANSFER_DTYPE)
    engine.load_transfers(loaded, np.zeros(len(loaded), dtype=np.uint8))
    oracle.upsert_transfers(loaded, np.ones(len(loaded), dtype=np.uint8))
    assert rows(engine.export_transfers()) == rows(oracle.export_transfers())
    lo, hi = T0 + 200 - 10, T0 + 500 + 10  # the tail of the copied prepare, the placed one, the head of the loaded
    got, matched, complete = engine.query_transfers(timestamp_min=lo, timestamp_max=hi)
    resident = oracle.export_transfers()
    resident = resident[np.argsort(resident["timestamp"], kind="stable")]
    want = resident[(resident["timestamp"] >= lo) & (resident["timestamp"] <= hi)]
    assert len(want) == 11 + 100 + 11 and matched == len(want) and complete
    assert rows(got) == rows(want)
    ev, matched, _ = engine.get_change_events(timestamp_min=lo, timestamp_max=hi)
    assert matched == len(want) and rows(ev["transfer"]["timestamp"]) == rows(want["timestamp"])
    acct = account_id(0)
    got, _, _ = engine.get_account_transfers(acct, timestamp_min=lo, timestamp_max=hi)
    lo64, hi64 = acct & U64_MAX, acct >> 64
    on = ((want["debit_account_id_lo"] == lo64) & (want["debit_account_id_hi"] == hi64)) | \
         ((want["credit_account_id_lo"] == lo64) & (want["credit_account_id_hi"] == hi64))
    assert on.sum() >= 3 and rows(got) == rows(want[on])


def test_eviction_moves_the_plane(gpu_engine_factory):
    """In-place commits, a write-back, the eviction of a prefix: the kept records' timestamps moved with
    them (queries, lookups and the next commit's two-phase checks read them at their new positions)."""
    sc, ids, first, last = edge_scenario()
    oracle = OracleEngine(4096, 1 << 14)
    expected = run_oracle(sc, oracle)
    engine = gpu_engine_factory(**OPTS)
    assert run_inplace(sc, engine) == expected
    engine.checkpoint_delta()
    before = engine.export_transfers()
    before = before[np.argsort(before["timestamp"], kind="stable")]
    keep = 300 + 257 + 100  # the last two prepares and a part of the one before: the cut is inside a tile
    evicted = engine.evict_transfers(keep)
    assert 0 < evicted < len(before)
    kept = engine.export_transfers()
    kept = kept[np.argsort(kept["timestamp"], kind="stable")]
    assert len(kept) == len(before) - evicted and rows(kept) == rows(before[evicted:])
    got, matched, complete = engine.query_transfers()
    assert rows(got) == rows(kept) and matched == len(kept) and not complete
    t_mid = int(kept["timestamp"][len(kept) // 2])
    for lo, hi in ((t_mid, 0), (0, t_mid), (t_mid - 1, t_mid + 1), (int(kept["timestamp"][0]), int(kept["timestamp"][-1]))):
        want = kept[(kept["timestamp"] >= lo) & ((kept["timestamp"] <= hi) | (hi == 0))]
        got, matched, _ = engine.query_transfers(timestamp_min=lo, timestamp_max=hi)
        assert rows(got) == rows(want) and matched == len(want), (lo, hi)
        ev, matched, _ = engine.get_change_events(timestamp_min=lo, timestamp_max=hi, limit=4000)
        assert matched == len(want) and rows(ev["transfer"]["timestamp"]) == rows(want["timestamp"])
    id_rows = np.stack([kept["id_lo"], kept["id_hi"]], axis=1)
    got, state = engine.fetch_transfers(id_rows)
    assert state.all() and rows(got) == rows(kept)
    # A kept pending transfer, voided in place after the move: its timestamp passes `p.timestamp < ts`.
    posted = {int(t) for t, _ in engine.export_posted()}
    open_ = [t for t in kept if int(t["flags"]) & int(TF.pending) and int(t["timestamp"]) not in posted and not int(t["timeout"])]
    assert open_
    void = Scenario()
    void.steps = [("commit", 129, last + 100, [pack_transfer(id=9000, pending_id=int(open_[0]["id_lo"]),
                                                             flags=int(TF.void_pending_transfer))])]
    assert run_inplace(void, engine) == [b""]


def test_node_in_place_homes(gpu_engine_factory):
    """Two logical shards: routed prepares are committed in place on their homes.  The node's answers
    equal a single engine's."""
    sc = Scenario()
    sc.steps.append(accounts_step())
    ts, tid = T0 + 10, 1
    for L in (300, 65, 257):
        ts += 1 + L
        sc.steps.append(("commit", 129, ts, [create(tid + k, k, TF.pending if k % 9 == 0 else 0) for k in range(L)]))
        tid += L
    ids = list(range(1, tid))
    oracle = OracleEngine(4096, 1 << 12)
    expected = run_oracle(sc, oracle)
    single = gpu_engine_factory(**OPTS)
    node = gpu_engine_factory(accounts_max=4096, transfers_max=1 << 14, pass_events_max=8192, pass_batches_max=16,
                              devices=(0, 0))
    assert run_oracle(sc, single) == expected and run_oracle(sc, node) == expected
    assert_same_state(oracle, node)
    first = T0 + 10 + 2
    windows = [(0, 0), (first + 100, 0), (1, ts - 100), (first + 299, first + 301)]
    assert_same_answers(answers(node, ids, windows, ts + 10, delta=False), answers(single, ids, windows, ts + 10, delta=False))
