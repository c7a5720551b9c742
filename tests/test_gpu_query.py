"""get_account_transfers (include/tbgpu.h tbgpu_get_account_transfers, csrc/k_query.h): the account
filter query over the HBM transfer log.  The reference has no such operation, so the checker is a
brute-force numpy filter, sort and cut over the oracle's exported transfers; records are compared
byte for byte, with `matched` and `complete`."""
import ctypes
import itertools
import random

import numpy as np
import pytest

from tests.harness.oracle import OracleEngine
from tests.harness.workload import account_id, make_scenario
from tigerbeetle_amd import _lib
from tigerbeetle_amd.types import (ACCOUNT_FILTER_DTYPE, BATCH_MAX, TRANSFER_DTYPE, U64_MAX, TransferFlags,
                                   pack_account, pack_transfer)

pytestmark = pytest.mark.gpu

SCENARIO = dict(n_accounts=64, n_transfer_batches=24, batch_len=(100, 400), p_pending=0.3, p_post_void=0.25, p_dup=0.05,
                p_linked=0.05, p_limit=0.05, p_balancing=0.02, p_invalid=0.05)
PV = int(TransferFlags.post_pending_transfer | TransferFlags.void_pending_transfer)


def brute(transfers, account, debits=True, credits=True, reversed=False, timestamp_min=0, timestamp_max=0, limit=8190,
          out_cap_records=None):
    """(the first records by timestamp under the limit, every match) over exported transfers."""
    lo, hi = account & U64_MAX, account >> 64
    m = np.zeros(len(transfers), dtype=bool)
    if debits:
        m |= (transfers["debit_account_id_lo"] == lo) & (transfers["debit_account_id_hi"] == hi)
    if credits:
        m |= (transfers["credit_account_id_lo"] == lo) & (transfers["credit_account_id_hi"] == hi)
    m &= transfers["timestamp"] >= timestamp_min
    if timestamp_max:
        m &= transfers["timestamp"] <= timestamp_max
    sel = transfers[m]
    sel = sel[np.argsort(sel["timestamp"], kind="stable")]
    if reversed:
        sel = sel[::-1]
    k = min(limit, BATCH_MAX, limit if out_cap_records is None else out_cap_records)
    return sel[:k], len(sel)


def check(engine, transfers, account, complete=True, **filter):
    want, matched = brute(transfers, account, **filter)
    got, got_matched, got_complete = engine.get_account_transfers(account, **filter)
    assert got.tobytes() == want.tobytes(), (hex(account), filter, len(got), len(want))
    assert got_matched == matched and got_complete == complete, (hex(account), filter)
    return got, matched


def ids_of(transfers):
    return sorted({(int(h) << 64) | int(l) for f in ("debit_account_id", "credit_account_id")
                   for l, h in zip(transfers[f + "_lo"], transfers[f + "_hi"])})


def commit_all(sc, *engines, steps=None):
    replies = []
    for _, op, ts, events in (sc.steps if steps is None else steps):
        body = b"".join(events)
        out = [e.commit(op, ts, body) for e in engines]
        assert all(o == out[0] for o in out)
        replies.append(out[0])
    return replies


def posted_states(transfers, posted):
    """tbgpu_load_transfers' posted_state of each record from exported {pending timestamp, voided} pairs."""
    state = {int(ts): 2 if v else 1 for ts, v in posted}
    return np.array([state.get(int(t), 0) for t in transfers["timestamp"]], dtype=np.uint8)


def windows(transfers, account):
    """open, [median, open], [open, median], [one match's timestamp, the same]."""
    median = int(np.sort(transfers["timestamp"])[len(transfers) // 2])
    mine, _ = brute(transfers, account)
    one = int(mine["timestamp"][len(mine) // 2])
    return [dict(), dict(timestamp_min=median), dict(timestamp_max=median), dict(timestamp_min=one, timestamp_max=one)]


def sweep(engine, transfers, limits, seen):
    """The product of sides, direction, limit and window for every account of the export."""
    for account in ids_of(transfers):
        for (d, c), rev, limit, win in itertools.product(((True, False), (False, True), (True, True)), (False, True),
                                                         limits, windows(transfers, account)):
            got, matched = check(engine, transfers, account, debits=d, credits=c, reversed=rev, limit=limit, **win)
            seen["queries"] += 1
            seen["cut"] |= matched > len(got) == limit
            seen["post_void"] |= bool(np.any(got["flags"] & PV))


@pytest.fixture(scope="module")
def ledger():
    """The scenario, the oracle that committed all of it, its replies and its exports (never changed)."""
    sc = make_scenario(2025, **SCENARIO)
    oracle = OracleEngine(4096, 1 << 15)
    replies = commit_all(sc, oracle)
    return dict(sc=sc, replies=replies, transfers=oracle.export_transfers(), posted=oracle.export_posted(),
                accounts=oracle.export_accounts(), commit_timestamp=oracle.commit_timestamp)


def test_brute_force_single_engine(ledger, gpu_engine_factory):
    sc, transfers = ledger["sc"], ledger["transfers"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    assert commit_all(sc, engine) == ledger["replies"]
    seen = dict(queries=0, cut=False, post_void=False)
    sweep(engine, transfers, (1, 25, 8190), seen)
    accounts = ids_of(transfers)
    hot = max(accounts, key=lambda a: brute(transfers, a)[1])
    last = int(transfers["timestamp"].max())
    check(engine, transfers, hot, timestamp_min=last + 1)                 # a window with no match
    check(engine, transfers, hot, timestamp_min=1, timestamp_max=2)
    got, matched = check(engine, transfers, account_id(5000))             # an account that does not exist
    assert matched == 0 and len(got) == 0
    got, matched = check(engine, transfers, hot, limit=25, out_cap_records=10)
    assert len(got) == 10 and matched > 25
    # Non-vacuity.
    assert seen["queries"] >= len(accounts) * 72 and seen["cut"] and seen["post_void"]
    named = 0
    for _, op, _, events in sc.steps:
        if op == 129:
            t = np.frombuffer(b"".join(events), dtype=TRANSFER_DTYPE)
            lo, hi = hot & U64_MAX, hot >> 64
            named += int((((t["debit_account_id_lo"] == lo) & (t["debit_account_id_hi"] == hi))
                          | ((t["credit_account_id_lo"] == lo) & (t["credit_account_id_hi"] == hi))).sum())
    assert named > brute(transfers, hot)[1]  # dead log positions naming the account were skipped
    assert engine.stats()["log_used"] > len(transfers)


def test_inplace_log_failed_events_never_match(gpu_engine_factory):
    """One 600-event prepare committed in place (tbgpu_log_window): failing events that name the queried
    account as their debit account — id 0, and duplicates of earlier ok events — sit at the wave and
    tile boundaries of the scan and hold log positions, but never match."""
    engine = gpu_engine_factory(transfers_max=1 << 12)
    oracle = OracleEngine(64, 1 << 12)
    n_acc, A = 8, account_id(0)
    body = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(n_acc))
    assert engine.commit(128, 10**12, body) == oracle.commit(128, 10**12, body) == b""
    rng = random.Random(7)
    bad = {63: "zero", 64: "dup", 255: "dup", 256: "zero", 511: "dup"}
    events = []
    for i in range(600):
        dr = rng.randrange(n_acc)
        cr = (dr + 1 + rng.randrange(n_acc - 1)) % n_acc
        ev = dict(id=1000 + i, debit_account_id=account_id(dr), credit_account_id=account_id(cr), amount=1 + i, ledger=1,
                  code=1)
        if i in bad:
            ev.update(debit_account_id=A, credit_account_id=account_id(1), id=0 if bad[i] == "zero" else 1000 + i - 40)
        events.append(pack_transfer(**ev))
    body = b"".join(events)
    ts = 10**12 + 1000
    expected = oracle.commit(129, ts, body)
    failed = np.frombuffer(expected, dtype=np.uint32)[0::2].tolist()
    assert failed == sorted(bad)  # exactly the planted events failed
    window = engine.log_window(600)
    engine.to_device(window, np.frombuffer(body, dtype=np.uint8))
    res, rb = engine.alloc(600 * 8), engine.alloc(4)
    engine.commit_device_async(129, [ts], [600], window, res, rb)
    # The query drains the pending call itself.
    transfers = oracle.export_transfers()
    got, matched = check(engine, transfers, A, credits=False)
    t = np.frombuffer(body, dtype=TRANSFER_DTYPE)
    named = int(((t["debit_account_id_lo"] == A & U64_MAX) & (t["debit_account_id_hi"] == A >> 64)).sum())
    assert matched == named - len(bad) and matched > 0
    for rev in (False, True):
        check(engine, transfers, A, reversed=rev)
        check(engine, transfers, A, reversed=rev, limit=3)
    n_reply = int(engine.to_host(rb, 4).view(np.uint32)[0])
    assert bytes(engine.to_host(res, n_reply)) == expected
    engine.free(res)
    engine.free(rb)


def test_unordered_log(gpu_engine_factory):
    """Half B committed first, then half A (earlier timestamps) loaded in shuffled order: the log is out
    of timestamp order and the answer is by timestamp regardless — with the whole key buffer, and with
    one small enough that every account's matches take several rounds."""
    kw = dict(n_accounts=8, n_transfer_batches=40, batch_len=(100, 400), p_pending=0.3, p_dup=0.05, p_linked=0.05,
              p_limit=0.0, p_balancing=0.0, p_invalid=0.05, id_space=1 << 40)
    # Nothing in B depends on A (no limits, no balancing, its posts and voids name its own pending
    # transfers, disjoint ids), so B commits alike with and without A before it.
    sa = make_scenario(31, p_post_void=0.25, **kw)
    last = sa.steps[-1][2]
    sb = make_scenario(32, p_post_void=0.25, start_ts=last + 10**9, **kw)
    acct_steps = [s for s in sa.steps if s[1] == 128]
    a_steps = [s for s in sa.steps if s[1] == 129]
    b_steps = [s for s in sb.steps if s[1] == 129]
    oracle = OracleEngine(64, 1 << 15)
    engine1 = gpu_engine_factory(transfers_max=1 << 15)
    engine2 = gpu_engine_factory(transfers_max=1 << 15)
    commit_all(sa, oracle, engine1, engine2, steps=acct_steps)
    commit_all(sa, oracle, engine1, steps=a_steps)
    half_a = engine1.export_transfers()
    states = posted_states(half_a, engine1.export_posted())
    commit_all(sb, oracle, engine2, steps=b_steps)
    order = np.random.default_rng(5).permutation(len(half_a))
    engine2.load_transfers(half_a[order], states[order])
    transfers = oracle.export_transfers()
    assert engine2.export_transfers().tobytes() == transfers.tobytes()
    assert len(half_a) > 1000 and len(transfers) - len(half_a) > 1000 and states.max() == 2
    for keys_max in (0, 256):
        engine2.query_keys_max(keys_max)
        rounds = False
        for account in ids_of(transfers):
            in_a = brute(half_a, account)[1]
            total = brute(transfers, account)[1]
            assert 3 < in_a < total - 3
            rounds |= total > 3 * 256
            # limits that cut inside A, inside B and across the seam, from either end
            for rev, limit in itertools.product((False, True), (3, in_a + 3, total - 3, total - in_a + 3, 8190)):
                check(engine2, transfers, account, reversed=rev, limit=limit)
            check(engine2, transfers, account, credits=False, timestamp_min=last - 10**9, timestamp_max=last + 2 * 10**9)
        assert rounds  # more matches than three rounds' keys at 256


def test_eviction_and_reload(ledger, gpu_engine_factory):
    sc, transfers = ledger["sc"], ledger["transfers"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, engine)
    accounts = ids_of(transfers)
    hot = max(accounts, key=lambda a: brute(transfers, a)[1])
    check(engine, transfers, hot, complete=True)
    engine.checkpoint_delta()
    assert engine.evict_transfers(2500) > 0
    resident = engine.export_transfers()
    assert 0 < len(resident) < len(transfers)
    for account in accounts[:8] + [hot]:
        for rev, limit in itertools.product((False, True), (1, 25, 8190)):
            check(engine, resident, account, complete=False, reversed=rev, limit=limit)
    # Two evicted records of the account come back at the log's end, out of timestamp order.
    here = set(resident["timestamp"].tolist())
    mine, _ = brute(transfers, hot)
    gone = mine[[int(t) not in here for t in mine["timestamp"]]]
    assert len(gone) >= 2
    back = gone[[len(gone) // 2, 0]]
    engine.load_transfers(back, posted_states(back, ledger["posted"]))
    resident = engine.export_transfers()
    for rev, limit in itertools.product((False, True), (1, 2, 25, 8190)):
        got, _ = check(engine, resident, hot, complete=False, reversed=rev, limit=limit)
    assert set(back["timestamp"].tolist()) <= set(got["timestamp"].tolist())


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=["node2", "node3"])
def test_node(devices, gpu_engine_factory):
    sc = make_scenario(2026, **dict(SCENARIO, n_accounts=16, n_transfer_batches=6))
    oracle = OracleEngine(4096, 1 << 14)
    engine = gpu_engine_factory(accounts_max=4096, transfers_max=1 << 14, pass_events_max=2048, pass_batches_max=16,
                                devices=devices)
    commit_all(sc, oracle, engine)
    transfers = oracle.export_transfers()
    seen = dict(queries=0, cut=False, post_void=False)
    sweep(engine, transfers, (1, 7, 8190), seen)
    assert seen["cut"] and seen["post_void"] and seen["queries"] >= 10 * 72
    got, matched = check(engine, transfers, account_id(5000))
    assert matched == 0


def raw_filter(**fields):
    f = np.zeros(1, dtype=ACCOUNT_FILTER_DTYPE)
    base = dict(account_id_lo=account_id(0) & U64_MAX, account_id_hi=account_id(0) >> 64, limit=10, flags=3)
    base.update(fields)
    for k, v in base.items():
        f[k] = v
    return f


def test_invalid_filters(ledger, gpu_engine_factory):
    steps = ledger["sc"].steps[:4]
    engine = gpu_engine_factory(transfers_max=1 << 12)
    empty = engine.get_account_transfers_raw(raw_filter().tobytes())
    assert len(empty[0]) == 0 and empty[1:] == (0, True)  # a valid filter on an empty engine
    commit_all(ledger["sc"], engine, steps=steps)
    account = ids_of(engine.export_transfers())[0]
    good = dict(account_id_lo=account & U64_MAX, account_id_hi=account >> 64)
    got, matched, _ = engine.get_account_transfers_raw(raw_filter(**good).tobytes())
    assert matched > 0 and len(got) == min(matched, 10)
    reserved = np.zeros(24, dtype=np.uint8)
    reserved[23] = 1
    invalid = [dict(account_id_lo=0, account_id_hi=0), dict(account_id_lo=U64_MAX, account_id_hi=U64_MAX),
               dict(timestamp_min=U64_MAX), dict(timestamp_max=U64_MAX), dict(timestamp_min=10**12, timestamp_max=10**12 - 1),
               dict(limit=0), dict(flags=0), dict(flags=4), dict(flags=3 | 8), dict(flags=3 | (1 << 31)),
               dict(reserved=reserved)]
    for fields in invalid:
        got, matched, complete = engine.get_account_transfers_raw(raw_filter(**dict(good, **fields)).tobytes())
        assert len(got) == 0 and matched == 0 and complete, fields
    # NULL arguments are a status, nothing else is.
    f = ctypes.create_string_buffer(raw_filter(**good).tobytes(), 64)
    out = ctypes.create_string_buffer(128 * 10)
    res = _lib.tbgpu_query_result()
    fn = engine.lib.tbgpu_get_account_transfers
    assert fn(engine.h, None, out, 10, ctypes.byref(res)) == _lib.STATUS_INVALID
    assert fn(engine.h, f, None, 10, ctypes.byref(res)) == _lib.STATUS_INVALID
    assert fn(engine.h, f, out, 10, None) == _lib.STATUS_INVALID
    assert fn(engine.h, f, out, 10, ctypes.byref(res)) == _lib.STATUS_OK and res.count > 0


def by_id(accounts):
    return accounts[np.lexsort((accounts["id_lo"], accounts["id_hi"]))].tobytes()


def test_read_only_and_allocation_free(ledger, gpu_engine_factory):
    sc, transfers = ledger["sc"], ledger["transfers"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    twin = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, engine, twin, steps=sc.steps[:-1])
    resident = engine.export_transfers()
    before = (engine.commit_timestamp, engine.export_accounts().tobytes(), resident.tobytes(),
              engine.export_posted().tobytes())
    rng = random.Random(3)
    accounts = ids_of(resident)
    allocations = engine.lib.tbgpu_debug_allocations()
    stats = engine.stats()
    for _ in range(50):
        check(engine, resident, rng.choice(accounts), debits=rng.random() < 0.7, credits=True, reversed=rng.random() < 0.5,
              limit=rng.choice((1, 5, 8190)), timestamp_min=rng.choice((0, int(resident["timestamp"][len(resident) // 3]))))
    assert engine.lib.tbgpu_debug_allocations() == allocations
    after = engine.stats()
    assert all(after[k] == stats[k] for k in ("passes", "events", "transfers", "accounts", "log_used"))
    assert before == (engine.commit_timestamp, engine.export_accounts().tobytes(), engine.export_transfers().tobytes(),
                      engine.export_posted().tobytes())
    # A query between an asynchronous write-back's start and its wait leaves the delta alone.
    caps = (1 << 14, 1 << 14, 1 << 14)
    engine.checkpoint_delta_async(caps)
    check(engine, resident, accounts[0])
    check(engine, resident, accounts[-1], reversed=True, limit=5)
    delta = engine.checkpoint_delta_wait()
    sync = twin.checkpoint_delta(caps)
    assert len(delta.transfers) == len(resident)
    assert delta.transfers.tobytes() == sync.transfers.tobytes() and delta.posted.tobytes() == sync.posted.tobytes()
    assert by_id(delta.accounts) == by_id(sync.accounts) and delta.created_after == sync.created_after
    # ... and the next commit still answers as the oracle did.
    _, op, ts, events = sc.steps[-1]
    assert engine.commit(op, ts, b"".join(events)) == ledger["replies"][-1]
    assert engine.commit_timestamp == ledger["commit_timestamp"]
    assert engine.export_transfers().tobytes() == transfers.tobytes()
    assert engine.export_accounts().tobytes() == ledger["accounts"].tobytes()
