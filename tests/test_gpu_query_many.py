"""get_account_transfers_many (include/tbgpu.h tbgpu_get_account_transfers_many, csrc/k_query_many.h): up
to 64 account filters over one read of the HBM transfer log.  Its specification is one sentence —
answer i is what the single call gives for filter i — so every answer is compared byte for byte with
the single call's and with the brute-force numpy filter of tests/test_gpu_query.py, with `matched` and
`complete`.  The chunk of the scan is shrunk through tbgpu_bench_query_many_tiles so that a small log
spans many chunks."""
import ctypes
import itertools
import random

import numpy as np
import pytest

from tests.harness.oracle import OracleEngine
from tests.harness.workload import account_id, make_scenario
from tests.test_gpu_query import SCENARIO, brute, by_id, commit_all, ids_of, posted_states, raw_filter
from tigerbeetle_amd import _lib
from tigerbeetle_amd.state_machine import Engine, Options
from tigerbeetle_amd.types import ACCOUNT_FILTER_DTYPE, TRANSFER_DTYPE, U64_MAX, pack_account, pack_transfer

pytestmark = pytest.mark.gpu

LIMITS = (1, 2, 63, 64, 65, 255, 256, 257, 8190)
SIDES = ((True, False), (False, True), (True, True))


def spec(account, debits=True, credits=True, reversed=False, limit=8190, **window):
    return account, dict(debits=debits, credits=credits, reversed=reversed, limit=limit, **window)


def check_batch(engine, transfers, specs, cap=None, complete=True, single=True):
    """Every answer of one batched call against the brute force and (single) the single call."""
    filters = [Engine.account_filter(a, **kw) for a, kw in specs]
    answers = engine.get_account_transfers_many(filters, cap)
    assert len(answers) == len(specs)
    for (account, kw), f, (got, matched, got_complete) in zip(specs, filters, answers):
        want, want_matched = brute(transfers, account, out_cap_records=cap, **kw)
        assert got.tobytes() == want.tobytes(), (hex(account), kw, len(got), len(want))
        assert (matched, got_complete) == (want_matched, complete), (hex(account), kw)
        if single:
            one, one_matched, one_complete = engine.get_account_transfers_raw(f, cap)
            assert (one.tobytes(), one_matched, one_complete) == (got.tobytes(), matched, got_complete), (hex(account), kw)
    return answers


def own_windows(transfers, account):
    """open, and each edge of the account's own timestamps: on it and one past it."""
    ts = np.sort(brute(transfers, account)[0]["timestamp"]).tolist()
    mid = ts[len(ts) // 2]
    return [dict(), dict(timestamp_min=ts[0]), dict(timestamp_min=ts[0] + 1), dict(timestamp_max=ts[-1]),
            dict(timestamp_max=ts[-1] - 1), dict(timestamp_min=mid, timestamp_max=mid), dict(timestamp_min=ts[1], timestamp_max=ts[-2])]


@pytest.fixture(scope="module")
def ledger():
    """The 6,652-position scenario of tests/test_gpu_query.py in one engine that is only ever read, with
    the oracle's exports (never changed)."""
    sc = make_scenario(2025, **SCENARIO)
    oracle = OracleEngine(4096, 1 << 15)
    engine = Engine(Options(accounts_max=4096, transfers_max=1 << 14, pass_events_max=8192 * 4, pass_batches_max=64))
    replies = commit_all(sc, oracle, engine)
    transfers = oracle.export_transfers()
    assert len(transfers) >= 1500 and engine.stats()["log_used"] == 6652
    yield dict(sc=sc, engine=engine, transfers=transfers, replies=replies, posted=oracle.export_posted(),
               accounts=oracle.export_accounts(), commit_timestamp=oracle.commit_timestamp)
    engine.close()


@pytest.mark.parametrize("tiles", [1, 3], ids=["26chunks", "9chunks"])
def test_batches_equal_single_and_brute(tiles, ledger):
    engine, transfers = ledger["engine"], ledger["transfers"]
    engine.query_many_tiles(tiles)
    accounts = ids_of(transfers)
    rng = random.Random(tiles)
    # Every account x sides x direction once, each with a limit and a window of its own drawn so that
    # every limit and every window shape occurs with every side and direction.
    combos = list(itertools.product(accounts, SIDES, (False, True)))
    rng.shuffle(combos)
    specs, seen = [], set()
    for i, (account, (d, c), rev) in enumerate(combos):
        wins = own_windows(transfers, account)
        limit, w = LIMITS[i % len(LIMITS)], (i // len(LIMITS)) % len(wins)
        specs.append(spec(account, d, c, rev, limit, **wins[w]))
        seen.add((limit, w, d, c, rev))
    assert {s[0] for s in seen} == set(LIMITS) and {s[1] for s in seen} == set(range(7))
    cut = False
    for at in range(0, len(specs), 64):
        batch = specs[at:at + 64]
        for (a, kw), (got, matched, _) in zip(batch, check_batch(engine, transfers, batch)):
            cut |= matched > len(got) == kw["limit"]
    assert cut and len(specs) == len(accounts) * 6 > 5 * 64
    engine.query_many_tiles(0)


def test_batch_shapes(ledger):
    engine, transfers = ledger["engine"], ledger["transfers"]
    engine.query_many_tiles(1)
    accounts = ids_of(transfers)
    hot = max(accounts, key=lambda a: brute(transfers, a)[1])
    for n in (1, 2, 63):
        check_batch(engine, transfers, [spec(accounts[i % len(accounts)], reversed=i % 2 == 1, limit=LIMITS[i % 9]) for i in range(n)])
    check_batch(engine, transfers, [spec(hot, reversed=True, limit=65)] * 64)                       # the same filter 64 times
    ts = np.sort(brute(transfers, hot)[0]["timestamp"]).tolist()
    assert len(ts) > 64
    check_batch(engine, transfers, [spec(hot, reversed=i % 3 == 0, limit=256, timestamp_min=ts[i], timestamp_max=ts[-1 - i // 2])
                                    for i in range(64)])                                            # one account, 64 windows
    got = check_batch(engine, transfers, [spec(hot, credits=False), spec(hot, debits=False), spec(hot)])
    assert got[0][1] > 0 and got[1][1] > 0 and got[0][1] + got[1][1] == got[2][1]                  # the two sides of one account
    check_batch(engine, transfers, [spec(account_id(5000)), spec(hot, limit=2), spec(account_id(5001), reversed=True)])
    engine.query_many_tiles(0)
    check_batch(engine, transfers, [spec(a, reversed=i % 2 == 0) for i, a in enumerate(accounts)])  # the default chunk: one


def call_raw(engine, filters, cap, fill=0xA5):
    """The C call itself on a pre-filled `out`: (status, out bytes per slot, results)."""
    n = len(filters)
    src = ctypes.create_string_buffer(b"".join(filters), 64 * max(n, 1))
    out = np.full((max(n, 1), max(cap, 1) * 128), fill, dtype=np.uint8)
    res = (_lib.tbgpu_query_result * max(n, 1))()
    st = engine.lib.tbgpu_get_account_transfers_many(engine.h, src, n, out.ctypes.data, cap, res)
    return st, out, res


def test_output_slots(ledger):
    engine, transfers = ledger["engine"], ledger["transfers"]
    engine.query_many_tiles(3)
    accounts = ids_of(transfers)
    hot = max(accounts, key=lambda a: brute(transfers, a)[1])
    specs = [spec(hot, limit=25), spec(accounts[0], limit=3, reversed=True), spec(account_id(5000)), spec(accounts[1], limit=8190)]
    cap = 10  # below two of the limits: it caps those answers
    st, out, res = call_raw(engine, [Engine.account_filter(a, **kw) for a, kw in specs], cap)
    assert st == _lib.STATUS_OK
    for i, (account, kw) in enumerate(specs):
        want, matched = brute(transfers, account, out_cap_records=cap, **kw)
        assert (res[i].count, res[i].matched, res[i].complete) == (len(want), matched, 1)
        assert out[i, :128 * len(want)].tobytes() == want.tobytes()
        assert (out[i, 128 * len(want):] == 0xA5).all()  # past `count` the slot is untouched
    assert res[0].count == 10 and res[0].matched > 25 and res[1].count == 3 and res[2].count == 0 and res[3].count == 10
    check_batch(engine, transfers, specs, cap=cap)
    engine.query_many_tiles(0)


def test_boundaries_inplace_log(gpu_engine_factory):
    """One 900-event prepare committed in place, so event i sits at log position i.  Failing events that
    name a queried account sit on both sides of the wave, tile and chunk boundaries (chunks of 1 and of
    2 tiles) and never match; matches of two different filters sit in neighbouring lanes, in one
    record, and in the first and the last lane of a chunk.  The batch also drains the pending commit."""
    engine = gpu_engine_factory(transfers_max=1 << 12)
    oracle = OracleEngine(64, 1 << 12)
    n_acc, A, B = 8, account_id(0), account_id(1)
    body = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(n_acc))
    assert engine.commit(128, 10**12, body) == oracle.commit(128, 10**12, body) == b""
    rng = random.Random(11)
    bad = {63: "zero", 64: "dup", 255: "dup", 256: "zero", 511: "dup", 512: "zero"}
    planted = {0: (A, 2), 100: (A, 3), 101: (B, 4), 254: (B, 5), 257: (A, 6), 510: (B, 7), 513: (A, B), 767: (A, B), 768: (B, A),
               899: (B, 2)}
    events = []
    for i in range(900):
        dr = rng.randrange(n_acc)
        cr = (dr + 1 + rng.randrange(n_acc - 1)) % n_acc
        ev = dict(id=1000 + i, debit_account_id=account_id(dr), credit_account_id=account_id(cr), amount=1 + i, ledger=1, code=1)
        if i in planted:
            d, c = planted[i]
            ev.update(debit_account_id=d, credit_account_id=c if c > 64 else account_id(c))
        if i in bad:
            ev.update(debit_account_id=A, credit_account_id=B, id=0 if bad[i] == "zero" else 1000 + i - 40)
        events.append(pack_transfer(**ev))
    body = b"".join(events)
    ts = 10**12 + 1000
    expected = oracle.commit(129, ts, body)
    assert np.frombuffer(expected, dtype=np.uint32)[0::2].tolist() == sorted(bad)  # exactly the planted events failed
    window = engine.log_window(900)
    engine.to_device(window, np.frombuffer(body, dtype=np.uint8))
    res, rb = engine.alloc(900 * 8), engine.alloc(4)
    engine.commit_device_async(129, [ts], [900], window, res, rb)
    transfers = oracle.export_transfers()
    specs = [spec(A, credits=False), spec(B, credits=False), spec(A), spec(B, reversed=True), spec(B, debits=False, limit=2),
             spec(A, reversed=True, limit=1), spec(account_id(2)), spec(A, debits=False, reversed=True, limit=3)]
    engine.query_many_tiles(1)
    first = check_batch(engine, transfers, specs, single=False)  # the call drains the pending commit itself
    t = np.frombuffer(body, dtype=TRANSFER_DTYPE)
    named = int(((t["debit_account_id_lo"] == A & U64_MAX) & (t["debit_account_id_hi"] == A >> 64)).sum())
    assert first[0][1] == named - len(bad) > 0  # the dead positions naming A as debit matched nothing
    for tiles in (1, 2, 0):
        engine.query_many_tiles(tiles)
        check_batch(engine, transfers, specs)
        check_batch(engine, transfers, [spec(account_id(i % n_acc), reversed=i % 2 == 0, debits=i % 3 != 0, limit=LIMITS[i % 9])
                                        for i in range(64)])
    n_reply = int(engine.to_host(rb, 4).view(np.uint32)[0])
    assert bytes(engine.to_host(res, n_reply)) == expected
    engine.free(res)
    engine.free(rb)


def test_unordered_union(gpu_engine_factory):
    """The log of test_unordered_log: half B committed, then half A (earlier timestamps) loaded in
    shuffled order.  The union of the hits is out of timestamp order, so the batch is answered through
    the single query's keyed rounds — with the whole key buffer and with one of 256 keys."""
    kw = dict(n_accounts=8, n_transfer_batches=40, batch_len=(100, 400), p_pending=0.3, p_dup=0.05, p_linked=0.05,
              p_limit=0.0, p_balancing=0.0, p_invalid=0.05, id_space=1 << 40)
    sa = make_scenario(31, p_post_void=0.25, **kw)
    last = sa.steps[-1][2]
    sb = make_scenario(32, p_post_void=0.25, start_ts=last + 10**9, **kw)
    acct_steps = [s for s in sa.steps if s[1] == 128]
    oracle = OracleEngine(64, 1 << 15)
    engine1 = gpu_engine_factory(transfers_max=1 << 15)
    engine2 = gpu_engine_factory(transfers_max=1 << 15)
    commit_all(sa, oracle, engine1, engine2, steps=acct_steps)
    commit_all(sa, oracle, engine1, steps=[s for s in sa.steps if s[1] == 129])
    half_a = engine1.export_transfers()
    states = posted_states(half_a, engine1.export_posted())
    commit_all(sb, oracle, engine2, steps=[s for s in sb.steps if s[1] == 129])
    order = np.random.default_rng(5).permutation(len(half_a))
    engine2.load_transfers(half_a[order], states[order])
    transfers = oracle.export_transfers()
    assert engine2.export_transfers().tobytes() == transfers.tobytes()
    accounts = ids_of(transfers)
    seam = int(half_a["timestamp"].max()) + 1  # every record of B is at or above it
    specs = []
    for account in accounts:
        in_a, total = brute(half_a, account)[1], brute(transfers, account)[1]
        assert 3 < in_a < total - 3
        for rev, limit in itertools.product((False, True), (3, in_a + 3, total - 3, 8190)):
            specs.append(spec(account, reversed=rev, limit=limit))
    specs += [spec(a, credits=False, reversed=r, timestamp_min=last - 10**9, timestamp_max=last + 2 * 10**9)
              for a in accounts for r in (False, True)]  # windows across the seam
    specs = specs[:64]
    assert len(specs) == 64 and max(brute(transfers, a)[1] for a in accounts) > 3 * 256
    # Only the first filter's account touches the records out of order: the others' windows hold B alone.
    one = [spec(accounts[0], limit=8190)] + [spec(a, reversed=i % 2 == 0, limit=40 * i + 1, timestamp_min=seam)
                                             for i, a in enumerate(accounts[1:])]
    ordered = [spec(a, reversed=i % 2 == 1, timestamp_min=seam) for i, a in enumerate(accounts)]  # an ordered union
    for keys_max, tiles in ((0, 0), (256, 2)):
        engine2.query_keys_max(keys_max)
        engine2.query_many_tiles(tiles)
        check_batch(engine2, transfers, specs, single=keys_max == 256)
        check_batch(engine2, transfers, one)
        check_batch(engine2, transfers, ordered)


def test_eviction_and_reload(gpu_engine_factory):
    sc = make_scenario(2025, **SCENARIO)
    engine = gpu_engine_factory(transfers_max=1 << 14)
    oracle = OracleEngine(4096, 1 << 15)
    commit_all(sc, oracle, engine)
    transfers, posted = oracle.export_transfers(), oracle.export_posted()
    engine.query_many_tiles(3)
    accounts = ids_of(transfers)
    hot = max(accounts, key=lambda a: brute(transfers, a)[1])
    engine.checkpoint_delta()
    assert engine.evict_transfers(2500) > 0
    resident = engine.export_transfers()
    assert 0 < len(resident) < len(transfers)
    specs = [spec(a, reversed=i % 2 == 0, limit=(1, 25, 8190)[i % 3]) for i, a in enumerate(accounts[:63])]
    answers = check_batch(engine, resident, specs + [spec(0)], complete=False)
    assert answers[-1][0].size == 0 and answers[-1][1:] == (0, False)  # the invalid entry: the same `complete`
    # Two evicted records of the account come back at the log's end, out of timestamp order.
    here = set(resident["timestamp"].tolist())
    mine, _ = brute(transfers, hot)
    gone = mine[[int(t) not in here for t in mine["timestamp"]]]
    assert len(gone) >= 2
    back = gone[[len(gone) // 2, 0]]
    engine.load_transfers(back, posted_states(back, posted))
    resident = engine.export_transfers()
    got = check_batch(engine, resident, [spec(hot, reversed=r, limit=l) for r in (False, True) for l in (1, 2, 25, 8190)] + specs[:40],
                      complete=False)
    assert set(back["timestamp"].tolist()) <= set(got[3][0]["timestamp"].tolist())


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=["node2", "node3"])
def test_node(devices, gpu_engine_factory):
    sc = make_scenario(2026, **dict(SCENARIO, n_accounts=16, n_transfer_batches=6))
    oracle = OracleEngine(4096, 1 << 14)
    engine = gpu_engine_factory(accounts_max=4096, transfers_max=1 << 14, pass_events_max=2048, pass_batches_max=16, devices=devices)
    commit_all(sc, oracle, engine)
    transfers = oracle.export_transfers()
    accounts = ids_of(transfers)
    engine.query_many_tiles(1)
    specs = [spec(accounts[i % len(accounts)], *SIDES[i % 3], reversed=i % 2 == 1, limit=LIMITS[(i // 2) % 9]) for i in range(63)]
    answers = check_batch(engine, transfers, specs + [spec(account_id(5000))])
    assert answers[-1][1] == 0 and any(m > len(g) for g, m, _ in answers)
    wins = own_windows(transfers, accounts[0])
    check_batch(engine, transfers, [spec(accounts[0], reversed=i % 2 == 0, limit=7, **wins[i % 7]) for i in range(14)])


def test_invalid_filters(ledger):
    engine, transfers = ledger["engine"], ledger["transfers"]
    engine.query_many_tiles(3)
    accounts = ids_of(transfers)
    good = [dict(account_id_lo=a & U64_MAX, account_id_hi=a >> 64) for a in accounts[:3]]
    reserved = np.zeros(24, dtype=np.uint8)
    reserved[23] = 1
    invalid = [dict(account_id_lo=0, account_id_hi=0), dict(account_id_lo=U64_MAX, account_id_hi=U64_MAX),
               dict(timestamp_min=U64_MAX), dict(timestamp_max=U64_MAX), dict(timestamp_min=10**12, timestamp_max=10**12 - 1),
               dict(limit=0), dict(flags=0), dict(flags=4), dict(flags=3 | 8), dict(flags=3 | (1 << 31)), dict(reserved=reserved)]
    want = [engine.get_account_transfers_raw(raw_filter(**g).tobytes()) for g in good]
    assert all(m > 0 and len(g) == 10 for g, m, _ in want)
    for fields in invalid:
        batch = [raw_filter(**good[0]), raw_filter(**good[1]), raw_filter(**dict(good[1], **fields)), raw_filter(**good[2])]
        got = engine.get_account_transfers_many([f.tobytes() for f in batch])
        assert len(got[2][0]) == 0 and got[2][1:] == (0, True), fields  # that entry answers nothing ...
        for g, w in zip((got[0], got[1], got[3]), want):                 # ... and its neighbours are intact
            assert (g[0].tobytes(), g[1], g[2]) == (w[0].tobytes(), w[1], w[2]), fields
    every = engine.get_account_transfers_many([raw_filter(**dict(good[0], **f)).tobytes() for f in invalid])
    assert all(len(g) == 0 and (m, c) == (0, True) for g, m, c in every)
    # n_filters = 0 and 65, and NULL arguments.
    f = [raw_filter(**good[0]).tobytes()]
    fn = engine.lib.tbgpu_get_account_transfers_many
    assert engine.get_account_transfers_many([]) == []
    assert fn(engine.h, None, 0, None, 10, None) == _lib.STATUS_OK
    st, out, res = call_raw(engine, f * 65, 10)
    assert st == _lib.STATUS_INVALID and (out == 0xA5).all()
    assert all((r.count, r.complete, r.matched) == (0, 0, 0) for r in res)  # nothing was touched
    src = ctypes.create_string_buffer(f[0], 64)
    out = ctypes.create_string_buffer(128 * 10)
    res = (_lib.tbgpu_query_result * 1)()
    assert fn(engine.h, None, 1, out, 10, res) == _lib.STATUS_INVALID
    assert fn(engine.h, src, 1, None, 10, res) == _lib.STATUS_INVALID
    assert fn(engine.h, src, 1, out, 10, None) == _lib.STATUS_INVALID
    assert res[0].count == 0
    assert fn(engine.h, src, 1, out, 10, res) == _lib.STATUS_OK and res[0].count == 10
    engine.query_many_tiles(0)


def test_read_only_and_allocation_free(gpu_engine_factory):
    sc = make_scenario(2025, **SCENARIO)
    oracle = OracleEngine(4096, 1 << 15)
    engine = gpu_engine_factory(transfers_max=1 << 14)
    twin = gpu_engine_factory(transfers_max=1 << 14)
    replies = commit_all(sc, oracle, engine, twin, steps=sc.steps[:-1])
    assert replies
    engine.query_many_tiles(2)
    resident = engine.export_transfers()
    before = (engine.commit_timestamp, engine.export_accounts().tobytes(), resident.tobytes(), engine.export_posted().tobytes())
    rng = random.Random(3)
    accounts = ids_of(resident)
    third = int(resident["timestamp"][len(resident) // 3])

    def draw(n):
        return [spec(rng.choice(accounts), debits=rng.random() < 0.7, reversed=rng.random() < 0.5, limit=rng.choice((1, 5, 8190)),
                     timestamp_min=rng.choice((0, third))) for _ in range(n)]

    allocations = engine.lib.tbgpu_debug_allocations()
    stats = engine.stats()
    for i in range(20):
        check_batch(engine, resident, draw(rng.choice((1, 7, 64))), single=i < 3)
    assert engine.lib.tbgpu_debug_allocations() == allocations
    after = engine.stats()
    assert all(after[k] == stats[k] for k in ("passes", "events", "transfers", "accounts", "log_used"))
    assert before == (engine.commit_timestamp, engine.export_accounts().tobytes(), engine.export_transfers().tobytes(),
                      engine.export_posted().tobytes())
    # A batch between an asynchronous write-back's start and its wait leaves the delta alone.
    caps = (1 << 14, 1 << 14, 1 << 14)
    engine.checkpoint_delta_async(caps)
    check_batch(engine, resident, draw(64), single=False)
    delta = engine.checkpoint_delta_wait()
    sync = twin.checkpoint_delta(caps)
    assert len(delta.transfers) == len(resident)
    assert delta.transfers.tobytes() == sync.transfers.tobytes() and delta.posted.tobytes() == sync.posted.tobytes()
    assert by_id(delta.accounts) == by_id(sync.accounts) and delta.created_after == sync.created_after
    # ... and the next commit still answers as the oracle did; a batch then sees its records.
    _, op, ts, events = sc.steps[-1]
    assert engine.commit(op, ts, b"".join(events)) == oracle.commit(op, ts, b"".join(events))
    assert engine.commit_timestamp == oracle.commit_timestamp
    transfers = oracle.export_transfers()
    assert engine.export_transfers().tobytes() == transfers.tobytes()
    check_batch(engine, transfers, draw(64), single=False)
