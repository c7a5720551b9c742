"""query_transfers / query_accounts (include/tbgpu.h, csrc/k_query.h, csrc/k_query_filter.h): the field
filter over the HBM transfer log and over the account table.  The reference has neither operation, so
the checker is a brute-force numpy filter, stable sort by timestamp and cut over the oracle's exports;
records are compared byte for byte, with `matched` and `complete`."""
import ctypes
import itertools
import random

import numpy as np
import pytest

from tests.harness.oracle import OracleEngine
from tests.harness.workload import account_id, make_scenario
from tests.test_gpu_query import by_id, commit_all, posted_states
from tigerbeetle_amd import _lib
from tigerbeetle_amd.types import (BATCH_MAX, QUERY_FILTER_DTYPE, TRANSFER_DTYPE, U64_MAX, TransferFlags, pack_account,
                                   pack_transfer)

pytestmark = pytest.mark.gpu

FIELDS = ("user_data_128", "user_data_64", "user_data_32", "ledger", "code")
U128_VALUES = (0, 9, (3 << 64) | 9, (4 << 64) | 9)  # three share the low word
U64_VALUES = (0, 7, (1 << 40) + 1)
N_ACCOUNTS, FIRST_PREPARE = 9000, 8190
LEDGER_SIZES = {1: 8195, 2: 500, 3: 305}  # ledger 1: five more than one reply holds
PV = int(TransferFlags.post_pending_transfer | TransferFlags.void_pending_transfer)


def draw_fields(rng):
    return dict(user_data_128=rng.choice(U128_VALUES), user_data_64=rng.choice(U64_VALUES),
                user_data_32=rng.randrange(4), code=1 + rng.randrange(5))


def make_workload(seed, ledger_sizes, first_prepare, n_prepares, per_prepare, pool):
    """[(operation, timestamp, body)]: the accounts in two create_accounts prepares, then create_transfers
    prepares among the first `pool` accounts of each ledger — plain, pending, post / void, linked chains
    (half of them failing at their last member, so the chain is rolled back), duplicate ids and invalid
    events, so that dead log positions exist."""
    rng = random.Random(seed)
    ledgers = [l for l, n in ledger_sizes.items() for _ in range(n)]
    rng.shuffle(ledgers)
    events = [pack_account(id=account_id(i), ledger=l, **draw_fields(rng)) for i, l in enumerate(ledgers)]
    steps, ts = [], 10**12
    for chunk in (events[:first_prepare], events[first_prepare:]):
        ts += 10**6 + len(chunk)
        steps.append((128, ts, b"".join(chunk)))
    pools = {l: [account_id(i) for i, x in enumerate(ledgers) if x == l][:pool] for l in ledger_sizes}
    next_id, pending, used = [1000], [], []

    def plain(linked=False):
        ledger = rng.choice(list(pools))
        dr, cr = rng.sample(pools[ledger], 2)
        flags = int(TransferFlags.pending) if rng.random() < 0.25 else 0
        ev = dict(id=next_id[0], debit_account_id=dr, credit_account_id=cr, amount=1 + rng.randrange(1000), ledger=ledger,
                  flags=flags | (int(TransferFlags.linked) if linked else 0), **draw_fields(rng))
        next_id[0] += 1
        if flags:
            pending.append((ev["id"], ledger, ev["code"]))
        used.append(ev["id"])
        return ev

    for _ in range(n_prepares):
        batch = []
        while len(batch) < per_prepare:
            r = rng.random()
            if r < 0.04 and len(batch) + 3 <= per_prepare:
                chain = [plain(linked=True), plain(linked=True), plain()]
                if rng.random() < 0.5:
                    chain[2]["code"] = 0
                batch += chain
            elif r < 0.20 and pending:
                pid, ledger, code = rng.choice(pending)
                flag = TransferFlags.post_pending_transfer if rng.random() < 0.6 else TransferFlags.void_pending_transfer
                ev = dict(draw_fields(rng), id=next_id[0], pending_id=pid, flags=int(flag), ledger=rng.choice((0, ledger)),
                          code=rng.choice((0, code)))
                next_id[0] += 1
                batch.append(ev)
            elif r < 0.25 and used:
                batch.append(dict(plain(), id=rng.choice(used)))
            elif r < 0.30:
                batch.append(dict(plain(), **rng.choice((dict(id=0), dict(ledger=0), dict(code=0), dict(amount=0)))))
            else:
                batch.append(plain())
        ts += 10**6 + len(batch)
        steps.append((129, ts, b"".join(pack_transfer(**ev) for ev in batch)))
    return steps


def run(steps, *engines):
    replies = []
    for op, ts, body in steps:
        out = [e.commit(op, ts, body) for e in engines]
        assert all(o == out[0] for o in out)
        replies.append(out[0])
    return replies


def ledger_of(steps, n_account_steps, accounts_hint=16384):
    """The oracle that committed `steps`, its replies and exports (never changed); accounts0: the
    accounts before any transfer."""
    oracle = OracleEngine(accounts_hint, 1 << 14)
    replies = run(steps[:n_account_steps], oracle)
    accounts0 = oracle.export_accounts()
    replies += run(steps[n_account_steps:], oracle)
    return dict(steps=steps, replies=replies, accounts0=accounts0, accounts=oracle.export_accounts(),
                transfers=oracle.export_transfers(), posted=oracle.export_posted(), commit_timestamp=oracle.commit_timestamp)


@pytest.fixture(scope="module")
def world():
    return ledger_of(make_workload(77, LEDGER_SIZES, FIRST_PREPARE, 20, 300, 24), 2)


@pytest.fixture(scope="module")
def small_world():
    """The same shape at a node test's size: 600 accounts, 1,600 transfer events."""
    return ledger_of(make_workload(78, {1: 400, 2: 150, 3: 50}, 450, 8, 200, 12), 2, accounts_hint=4096)


def brute(records, flt, reversed=False, timestamp_min=0, timestamp_max=0, limit=8190, out_cap_records=None):
    """(the first records by timestamp under the limit, every match) over exported accounts or transfers."""
    m = np.ones(len(records), dtype=bool)
    v = flt.get("user_data_128", 0)
    if v:
        m &= (records["user_data_128_lo"] == (v & U64_MAX)) & (records["user_data_128_hi"] == (v >> 64))
    for f in FIELDS[1:]:
        if flt.get(f, 0):
            m &= records[f] == flt[f]
    m &= records["timestamp"] >= timestamp_min
    if timestamp_max:
        m &= records["timestamp"] <= timestamp_max
    sel = records[m]
    sel = sel[np.argsort(sel["timestamp"], kind="stable")]
    if reversed:
        sel = sel[::-1]
    k = min(limit, BATCH_MAX, limit if out_cap_records is None else out_cap_records)
    return sel[:k], len(sel)


def check(query, records, flt, complete=True, **kw):
    want, matched = brute(records, flt, **kw)
    got, got_matched, got_complete = query(**flt, **kw)
    assert (got_matched, got_complete, len(got)) == (matched, complete, len(want)), (flt, kw)
    assert got.tobytes() == want.tobytes(), (flt, kw)
    return got, matched


def values_of(records, field):
    if field == "user_data_128":
        return sorted({(int(h) << 64) | int(l) for l, h in zip(records["user_data_128_lo"], records["user_data_128_hi"])} - {0})
    return sorted(set(records[field].tolist()) - {0})


def value_at(rec, field):
    return (int(rec["user_data_128_hi"]) << 64) | int(rec["user_data_128_lo"]) if field == "user_data_128" else int(rec[field])


def filters_of(records, rng):
    """Each single field at each of its values and at a value nothing carries; every pair of fields and
    all five at the values of a record that has them all non-zero; all five at values nothing carries."""
    out = [{f: v} for f in FIELDS for v in values_of(records, f)]
    out.append(dict(ledger=9))
    full = [r for r in records if all(value_at(r, f) for f in FIELDS)]
    assert full
    for f, g in itertools.combinations(FIELDS, 2):
        r = rng.choice(full)
        out.append({f: value_at(r, f), g: value_at(r, g)})
    r = rng.choice(full)
    out.append({f: value_at(r, f) for f in FIELDS})
    out.append(dict({f: value_at(r, f) for f in FIELDS}, user_data_32=77))
    return out


def windows(records, flt):
    """open, [median, open], [open, median], [one match's timestamp, the same]."""
    median = int(np.sort(records["timestamp"])[len(records) // 2])
    out = [dict(), dict(timestamp_min=median), dict(timestamp_max=median)]
    mine, _ = brute(records, flt)
    if len(mine):
        one = int(mine["timestamp"][len(mine) // 2])
        out.append(dict(timestamp_min=one, timestamp_max=one))
    return out


def sweep(query, records, limits, seed=5):
    seen = dict(queries=0, cut=False, none=False, split=False)
    for flt in filters_of(records, random.Random(seed)):
        for rev, limit, win in itertools.product((False, True), limits, windows(records, flt)):
            got, matched = check(query, records, flt, reversed=rev, limit=limit, **win)
            seen["queries"] += 1
            seen["cut"] |= matched > len(got) == limit
            seen["none"] |= matched == 0
        v = flt.get("user_data_128", 0)
        if len(flt) == 1 and v >> 64:  # records equal in the low word, apart in the high one
            low = int((records["user_data_128_lo"] == (v & U64_MAX)).sum())
            seen["split"] |= 0 < brute(records, flt)[1] < low
    return seen


# ---- query_accounts ------------------------------------------------------------------------------
def accounts_engine(world, factory, **kw):
    engine = factory(accounts_max=16384, transfers_max=1 << 14, **kw)
    assert run(world["steps"], engine) == world["replies"]
    return engine


def test_query_accounts_sweep(world, gpu_engine_factory):
    engine, accounts = accounts_engine(world, gpu_engine_factory), world["accounts"]
    assert len(accounts) == N_ACCOUNTS and engine.export_accounts().tobytes() == accounts.tobytes()
    assert int((accounts["debits_posted_lo"] | accounts["credits_posted_lo"] | accounts["debits_pending_lo"]).astype(bool).sum()) > 40
    seen = sweep(engine.query_accounts, accounts, (1, 25, 8190))
    assert seen["queries"] >= 27 * 2 * 3 * 3 and seen["cut"] and seen["none"] and seen["split"]


def test_query_accounts_selection_at_capacity(world, gpu_engine_factory):
    engine, accounts = accounts_engine(world, gpu_engine_factory), world["accounts"]
    q = engine.query_accounts
    by_ts = accounts[np.argsort(accounts["timestamp"], kind="stable")]
    for rev in (False, True):
        got, matched = check(q, accounts, {}, reversed=rev, limit=8190)
        assert matched == N_ACCOUNTS and len(got) == 8190
        assert got.tobytes() == (by_ts[::-1][:8190] if rev else by_ts[:8190]).tobytes()
        assert engine.query_select_scans() >= 1
        got, matched = check(q, accounts, {}, reversed=rev, limit=8190, out_cap_records=10)
        assert matched == N_ACCOUNTS and len(got) == 10
        # matched just above what one reply holds ...
        got, matched = check(q, accounts, dict(ledger=1), reversed=rev, limit=8190)
        assert matched == 8195 and len(got) == 8190
        # ... and just below (the window leaves ten of the ledger's accounts out; the second engine of
        # test_query_accounts_loaded_out_of_order holds ten fewer to begin with)
        mine = by_ts[by_ts["ledger"] == 1]
        win = dict(timestamp_max=int(mine["timestamp"][-11])) if rev else dict(timestamp_min=int(mine["timestamp"][10]))
        got, matched = check(q, accounts, dict(ledger=1), reversed=rev, limit=8190, **win)
        assert matched == len(got) == 8185
        assert engine.query_select_scans() == 0
        got, matched = check(q, accounts, dict(ledger=1), reversed=rev, limit=8185, **win)
        assert matched == len(got) == 8185
        got, matched = check(q, accounts, dict(ledger=1), reversed=rev, limit=8184, **win)
        assert matched == 8185 and len(got) == 8184
    # one timestamp: more matches than wanted cannot happen, the span is zero
    one = int(by_ts["timestamp"][4000])
    got, matched = check(q, accounts, {}, timestamp_min=one, timestamp_max=one)
    assert matched == 1


def test_query_accounts_select_early_exit(world, gpu_engine_factory):
    """The select stops at the pass whose picked digit is wanted whole.  The facts about the fixture
    that the expected pass counts rest on are asserted first."""
    engine, accounts = accounts_engine(world, gpu_engine_factory), world["accounts"]
    ts = accounts["timestamp"].astype(np.uint64)
    lo, hi = int(ts.min()), int(ts.max())
    assert len(ts) == N_ACCOUNTS and hi - lo == 1008999 and 1 << 11 <= hi - lo < 1 << 22  # the passes at shift 11 and 0 alone
    digits = [np.bincount((v >> np.uint64(11)).astype(np.int64)) for v in (ts - np.uint64(lo), np.uint64(hi) - ts)]
    assert digits[0][digits[0] > 0].tolist() == [2048, 2048, 2048, 2046, 810]  # the occupied digits, ascending
    assert digits[1][digits[1] > 0].tolist()[:2] == [810, 662]                  # ... and under REVERSED
    for rev, limit, scans in ((False, 2047, 2), (False, 2048, 1), (False, 2049, 2), (False, 4096, 1), (False, 8190, 1),
                              (True, 809, 2), (True, 810, 1), (True, 811, 2)):
        got, matched = check(engine.query_accounts, accounts, {}, reversed=rev, limit=limit)
        assert matched == N_ACCOUNTS and len(got) == limit
        assert engine.query_select_scans() == scans, (rev, limit)
    got, matched = check(engine.query_accounts, accounts, {}, out_cap_records=0)
    assert matched == N_ACCOUNTS and len(got) == 0


def test_query_accounts_loaded_out_of_order(world, gpu_engine_factory):
    """The second prepare's accounts are created first; the first prepare's (earlier timestamps) are then
    loaded in shuffled order, all but ten of ledger 1.  The table's slots are in no order anyway; the
    answers still equal brute force, and ledger 1 now matches just under one reply's worth."""
    engine = gpu_engine_factory(accounts_max=16384, transfers_max=1 << 12)
    op, ts, body = world["steps"][1]
    assert engine.commit(op, ts, body) == world["replies"][1]
    accounts0 = world["accounts0"]
    cut = int(np.sort(accounts0["timestamp"])[FIRST_PREPARE - 1])
    early = accounts0[accounts0["timestamp"] <= cut]
    assert len(early) == FIRST_PREPARE
    drop = set(early[early["ledger"] == 1]["timestamp"][:10].tolist())
    keep = early[[int(t) not in drop for t in early["timestamp"]]]
    engine.load_accounts(keep[np.random.default_rng(3).permutation(len(keep))])
    held = accounts0[[int(t) not in drop for t in accounts0["timestamp"]]]
    assert by_id(engine.export_accounts()) == by_id(held) and len(held) == N_ACCOUNTS - 10
    q = engine.query_accounts
    for rev in (False, True):
        got, matched = check(q, held, dict(ledger=1), reversed=rev)
        assert matched == len(got) == 8185
        got, matched = check(q, held, {}, reversed=rev)
        assert matched == N_ACCOUNTS - 10 and len(got) == 8190
        for flt, limit in itertools.product((dict(code=3), dict(user_data_128=U128_VALUES[2]), dict(ledger=2, user_data_64=7)),
                                            (1, 25, 8190)):
            check(q, held, flt, reversed=rev, limit=limit)
            check(q, held, flt, reversed=rev, limit=limit, timestamp_min=cut - 50, timestamp_max=cut + 50)


# ---- query_transfers -----------------------------------------------------------------------------
def test_query_transfers_sweep(world, gpu_engine_factory):
    engine, transfers = accounts_engine(world, gpu_engine_factory), world["transfers"]
    assert engine.export_transfers().tobytes() == transfers.tobytes()
    assert engine.stats()["log_used"] > len(transfers) + 100  # dead log positions
    assert np.any(transfers["flags"] & PV) and np.any(transfers["flags"] & int(TransferFlags.linked))
    seen = sweep(engine.query_transfers, transfers, (1, 25, 8190))
    assert seen["queries"] >= 27 * 2 * 3 * 3 and seen["cut"] and seen["none"] and seen["split"]
    got, matched = check(engine.query_transfers, transfers, {}, limit=8190, out_cap_records=10)
    assert matched == len(transfers) and len(got) == 10


def test_query_transfers_inplace_log_failed_events_never_match(gpu_engine_factory):
    """One 600-event prepare committed in place (tbgpu_log_window): failing events that carry the queried
    code — id 0, and duplicates of earlier ok events — sit at the wave and tile boundaries of the scan
    and hold log positions, but never match."""
    engine = gpu_engine_factory(transfers_max=1 << 12)
    oracle = OracleEngine(64, 1 << 12)
    n_acc = 8
    body = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(n_acc))
    assert engine.commit(128, 10**12, body) == oracle.commit(128, 10**12, body) == b""
    rng = random.Random(7)
    bad = {63: "zero", 64: "dup", 255: "dup", 256: "zero", 511: "dup"}
    events = []
    for i in range(600):
        dr = rng.randrange(n_acc)
        cr = (dr + 1 + rng.randrange(n_acc - 1)) % n_acc
        ev = dict(id=1000 + i, debit_account_id=account_id(dr), credit_account_id=account_id(cr), amount=1 + i, ledger=1,
                  code=7 if i % 5 == 0 else 1 + i % 3, user_data_32=i % 2)
        if i in bad:
            ev.update(code=7, id=0 if bad[i] == "zero" else 1000 + i - 40)
        events.append(pack_transfer(**ev))
    body = b"".join(events)
    ts = 10**12 + 1000
    expected = oracle.commit(129, ts, body)
    assert np.frombuffer(expected, dtype=np.uint32)[0::2].tolist() == sorted(bad)  # exactly the planted events failed
    window = engine.log_window(600)
    engine.to_device(window, np.frombuffer(body, dtype=np.uint8))
    res, rb = engine.alloc(600 * 8), engine.alloc(4)
    engine.commit_device_async(129, [ts], [600], window, res, rb)
    # The query drains the pending call itself.
    transfers = oracle.export_transfers()
    got, matched = check(engine.query_transfers, transfers, dict(code=7))
    named = int((np.frombuffer(body, dtype=TRANSFER_DTYPE)["code"] == 7).sum())
    assert matched == named - len(bad) and matched > 0
    for rev, flt in itertools.product((False, True), (dict(code=7), dict(code=7, user_data_32=1), dict(ledger=1))):
        check(engine.query_transfers, transfers, flt, reversed=rev)
        check(engine.query_transfers, transfers, flt, reversed=rev, limit=3)
    n_reply = int(engine.to_host(rb, 4).view(np.uint32)[0])
    assert bytes(engine.to_host(res, n_reply)) == expected
    engine.free(res)
    engine.free(rb)


def test_query_transfers_unordered_log(gpu_engine_factory):
    """tests/test_gpu_query.py test_unordered_log's engine — half B committed, then the earlier half A
    loaded in shuffled order — under the field filter, with the whole key buffer and with 256 keys a
    round."""
    kw = dict(n_accounts=8, n_transfer_batches=40, batch_len=(100, 400), p_pending=0.3, p_dup=0.05, p_linked=0.05,
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
    transfers = oracle.export_transfers()
    assert engine2.export_transfers().tobytes() == transfers.tobytes()
    q = engine2.query_transfers
    for keys_max in (0, 256):
        engine2.query_keys_max(keys_max)
        rounds = False
        for flt in (dict(code=1), dict(ledger=2), dict(code=2, ledger=1), dict(user_data_128=3), dict(user_data_64=5), {}):
            in_a, total = brute(half_a, flt)[1], brute(transfers, flt)[1]
            assert 3 < in_a < total - 3
            rounds |= total > 3 * 256
            # limits that cut inside A, inside B and across the seam, from either end
            for rev, limit in itertools.product((False, True), (3, in_a + 3, total - 3, total - in_a + 3, 8190)):
                check(q, transfers, flt, reversed=rev, limit=limit)
            check(q, transfers, flt, timestamp_min=last - 10**9, timestamp_max=last + 2 * 10**9)
        assert rounds  # more matches than three rounds' keys at 256


def test_query_transfers_eviction(world, gpu_engine_factory):
    engine, transfers = accounts_engine(world, gpu_engine_factory), world["transfers"]
    check(engine.query_transfers, transfers, dict(ledger=1), complete=True)
    engine.checkpoint_delta()
    assert engine.evict_transfers(2500) > 0
    resident = engine.export_transfers()
    assert 0 < len(resident) < len(transfers)
    for flt, rev, limit in itertools.product(({}, dict(ledger=1), dict(code=2, user_data_32=1), dict(user_data_128=U128_VALUES[3])),
                                             (False, True), (1, 25, 8190)):
        check(engine.query_transfers, resident, flt, complete=False, reversed=rev, limit=limit)
    # accounts are never evicted
    check(engine.query_accounts, world["accounts"], dict(ledger=2), complete=True)


# ---- nodes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=["node2", "node3"])
def test_node(devices, small_world, gpu_engine_factory):
    """After the transfers every home holds imported copies of foreign accounts: each account is still
    answered once, by its owner, with the oracle's balances."""
    w = small_world
    engine = gpu_engine_factory(accounts_max=4096, transfers_max=1 << 14, pass_events_max=2048, pass_batches_max=16,
                                devices=devices)
    assert run(w["steps"], engine) == w["replies"]
    accounts, transfers = w["accounts"], w["transfers"]
    got, matched = check(engine.query_accounts, accounts, {})
    assert matched == len(accounts) == 600 and len(set(zip(got["id_lo"].tolist(), got["id_hi"].tolist()))) == 600
    assert int((got["debits_posted_lo"] | got["credits_posted_lo"]).astype(bool).sum()) > 10
    seen = sweep(engine.query_accounts, accounts, (1, 7, 8190))
    assert seen["cut"] and seen["none"] and seen["split"]
    seen = sweep(engine.query_transfers, transfers, (1, 7, 8190))
    assert seen["cut"] and seen["none"] and seen["split"]
    got, matched = check(engine.query_transfers, transfers, {})
    assert matched == len(transfers) > 500


# ---- the call contract ---------------------------------------------------------------------------
def raw_filter(**fields):
    f = np.zeros(1, dtype=QUERY_FILTER_DTYPE)
    for k, v in dict(dict(ledger=1, limit=10), **fields).items():
        f[k] = v
    return f


def test_invalid_filters(small_world, gpu_engine_factory):
    engine = gpu_engine_factory(transfers_max=1 << 12)
    queries = (engine.query_transfers_raw, engine.query_accounts_raw)
    for q in queries:
        empty = q(raw_filter().tobytes())
        assert len(empty[0]) == 0 and empty[1:] == (0, True)  # a valid filter on an empty engine
    run(small_world["steps"][:4], engine)
    reserved = np.zeros(6, dtype=np.uint8)
    reserved[5] = 1
    invalid = [dict(timestamp_min=U64_MAX), dict(timestamp_max=U64_MAX), dict(timestamp_min=10**12, timestamp_max=10**12 - 1),
               dict(limit=0), dict(flags=2), dict(flags=1 | 4), dict(flags=1 << 31), dict(reserved=reserved)]
    for q, fn in zip(queries, (engine.lib.tbgpu_query_transfers, engine.lib.tbgpu_query_accounts)):
        got, matched, _ = q(raw_filter().tobytes())
        assert matched > 10 and len(got) == 10
        got, matched, _ = q(raw_filter(ledger=0, flags=1).tobytes())  # every field zero is valid
        assert matched > 10 and len(got) == 10
        for fields in invalid:
            got, matched, complete = q(raw_filter(**fields).tobytes())
            assert len(got) == 0 and matched == 0 and complete, fields
        # NULL arguments are a status, nothing else is.
        f = ctypes.create_string_buffer(raw_filter().tobytes(), 64)
        out = ctypes.create_string_buffer(128 * 10)
        res = _lib.tbgpu_query_result()
        assert fn(engine.h, None, out, 10, ctypes.byref(res)) == _lib.STATUS_INVALID
        assert fn(engine.h, f, None, 10, ctypes.byref(res)) == _lib.STATUS_INVALID
        assert fn(engine.h, f, out, 10, None) == _lib.STATUS_INVALID
        assert fn(engine.h, f, out, 10, ctypes.byref(res)) == _lib.STATUS_OK and res.count == 10
    # tbgpu_commit keeps refusing operations outside 128-131
    with pytest.raises(_lib.EngineError):
        engine.commit(132, small_world["steps"][3][1] + 10, raw_filter().tobytes() + bytes(64))


def test_read_only_and_allocation_free(small_world, gpu_engine_factory):
    w = small_world
    steps = w["steps"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    twin = gpu_engine_factory(transfers_max=1 << 14)
    run(steps[:-1], engine, twin)
    resident, held = engine.export_transfers(), engine.export_accounts()
    before = (engine.commit_timestamp, held.tobytes(), resident.tobytes(), engine.export_posted().tobytes())
    rng = random.Random(3)
    allocations = engine.lib.tbgpu_debug_allocations()
    stats = engine.stats()
    third = int(resident["timestamp"][len(resident) // 3])
    for i in range(50):
        flt = {f: rng.choice(values_of(held, f)) for f in rng.sample(FIELDS, rng.randrange(3))}
        kw = dict(reversed=rng.random() < 0.5, limit=rng.choice((1, 5, 8190)), timestamp_min=rng.choice((0, third)))
        if i % 2:
            check(engine.query_accounts, held, flt, **kw)
        else:
            check(engine.query_transfers, resident, flt, **kw)
    assert engine.lib.tbgpu_debug_allocations() == allocations
    after = engine.stats()
    assert all(after[k] == stats[k] for k in ("passes", "events", "transfers", "accounts", "log_used"))
    assert before == (engine.commit_timestamp, engine.export_accounts().tobytes(), engine.export_transfers().tobytes(),
                      engine.export_posted().tobytes())
    # One query of each kind between an asynchronous write-back's start and its wait leaves the delta alone.
    caps = (1 << 14, 1 << 14, 1 << 14)
    engine.checkpoint_delta_async(caps)
    check(engine.query_transfers, resident, dict(ledger=1), reversed=True, limit=5)
    check(engine.query_accounts, held, dict(ledger=1), limit=5)
    delta = engine.checkpoint_delta_wait()
    sync = twin.checkpoint_delta(caps)
    assert len(delta.transfers) == len(resident)
    assert delta.transfers.tobytes() == sync.transfers.tobytes() and delta.posted.tobytes() == sync.posted.tobytes()
    assert by_id(delta.accounts) == by_id(sync.accounts) and delta.created_after == sync.created_after
    # ... and the next commit still answers as the oracle did.
    op, ts, body = steps[-1]
    assert engine.commit(op, ts, body) == w["replies"][-1]
    assert engine.commit_timestamp == w["commit_timestamp"]
    assert engine.export_transfers().tobytes() == w["transfers"].tobytes()
    assert engine.export_accounts().tobytes() == w["accounts"].tobytes()
    check(engine.query_accounts, w["accounts"], {})
