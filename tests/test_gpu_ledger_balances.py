"""get_ledger_balances (include/tbgpu.h tbgpu_get_ledger_balances, csrc/k_ledgers.h): a trial balance
per ledger as of a timestamp, from one scan of the account table and one of the HBM log.  Rows,
`matched` and `complete` are compared byte for byte with the checker of tests/harness/ledgers.py
(itself held to the oracle in tests/test_ledger_checkers.py), with lookup_accounts_at and with
ledger_summary."""
import ctypes
import random

import numpy as np
import pytest

from tests.harness.balances import COLUMNS, balances_of, u128
from tests.harness.ledgers import LedgerBalances, ledgers_body, sums_by_ledger
from tests.harness.oracle import OracleEngine
from tests.harness.workload import account_id, make_scenario
from tests.test_gpu_query import SCENARIO, by_id, commit_all, posted_states
from tigerbeetle_amd import _lib
from tigerbeetle_amd._lib import EnginePanic
from tigerbeetle_amd.types import U64_MAX, TransferFlags, pack_account, pack_transfer

pytestmark = pytest.mark.gpu

PENDING = int(TransferFlags.pending)
POST = int(TransferFlags.post_pending_transfer)
VOID = int(TransferFlags.void_pending_transfer)
LEDGERS = (1, 2, 7, 2**32 - 1)
REQUEST = list(LEDGERS[::-1]) + [0, 5, 1]
LEDGERS_MAX = 1024
# k_ledgers.h: LEDGER_THREADS positions a tile, LEDGER_LOG_TILES tiles a workgroup of the log scan.
LOG_TILE = 512
LOG_WORKGROUP = 512 * 16


def check(engine, checker, ledgers, T, evicted=False, cap=None):
    """One request: rows, matched and complete as the checker has them."""
    want, matched, orphan = checker.at(ledgers, T, cap)
    got, got_matched, got_complete = engine.get_ledger_balances(ledgers, T, cap)
    assert len(got) == len(want), (T, len(got), len(want))
    assert got.tobytes() == want.tobytes(), T
    assert (got_matched, got_complete) == (matched, not evicted and not orphan), T
    return got


def sweep_timestamps(sc, transfers, commit_timestamp):
    stamps = np.sort(transfers["timestamp"])
    boundaries = [ts for _, _, ts, _ in sc.steps]
    inside = [int(t) for t in stamps[::23] if int(t) not in boundaries]
    assert len(inside) > 20
    return boundaries + inside + [0, 1, commit_timestamp, commit_timestamp + 1]


@pytest.fixture(scope="module")
def ledger():
    """The four-ledger scenario, the oracle that committed all of it, its exports and the checker over
    them (never changed)."""
    sc = make_scenario(2031, ledgers=LEDGERS, **SCENARIO)
    oracle = OracleEngine(4096, 1 << 15)
    replies = commit_all(sc, oracle)
    transfers, accounts = oracle.export_transfers(), oracle.export_accounts()
    return dict(sc=sc, replies=replies, transfers=transfers, accounts=accounts, commit_timestamp=oracle.commit_timestamp,
                posted=oracle.export_posted(), checker=LedgerBalances(transfers, accounts),
                stamps=sweep_timestamps(sc, transfers, oracle.commit_timestamp))


def test_single_engine_sweep(ledger, gpu_engine_factory):
    sc, checker = ledger["sc"], ledger["checker"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    assert commit_all(sc, engine) == ledger["replies"]
    assert engine.commit_timestamp == ledger["commit_timestamp"]
    answers = {T: check(engine, checker, REQUEST, T) for T in ledger["stamps"]}
    assert len({a.tobytes() for a in answers.values()}) > len(sc.steps)
    assert answers[0].tobytes() == answers[ledger["commit_timestamp"]].tobytes() == answers[ledger["commit_timestamp"] + 1].tobytes()
    for rows in answers.values():  # nothing but commits happened: every ledger balances at every T
        for c in ("pending", "posted"):
            for w in ("_lo", "_hi"):
                assert (rows["debits_" + c + w] == rows["credits_" + c + w]).all()
    assert not answers[1]["accounts"].any() and answers[0]["accounts"].tolist()[4] == len(ledger["accounts"])
    # The ledger-0 row at T = 0 is ledger_summary.
    summary = engine.ledger_summary()
    every = answers[0][4]
    assert balances_of(every) == tuple(summary[c] for c in COLUMNS) and int(every["accounts"]) == summary["accounts"]
    # out_cap_rows cuts in request order and writes nothing past it.
    T = sc.steps[len(sc.steps) // 2][2]
    n = len(REQUEST)
    for cap in (0, 1, 3, n - 1, n, n + 3):
        check(engine, checker, REQUEST, T, cap=cap)
    body = ledgers_body(REQUEST)
    out = ctypes.create_string_buffer(b"\xAB" * (128 * n), 128 * n)
    res = _lib.tbgpu_query_result()
    src = ctypes.create_string_buffer(body, len(body))
    assert engine.lib.tbgpu_get_ledger_balances(engine.h, T, src, n, out, 3, ctypes.byref(res)) == _lib.STATUS_OK
    assert (res.count, res.matched, res.complete) == (3, n, 1)
    assert out.raw[:3 * 128] == answers[T][:3].tobytes() and out.raw[3 * 128:] == b"\xAB" * (128 * (n - 3))
    assert engine.get_ledger_balances_raw(body, T)[0].tobytes() == answers[T].tobytes()


def test_against_lookup_accounts_at(ledger, gpu_engine_factory):
    sc, transfers = ledger["sc"], ledger["transfers"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, engine)
    ids = [u128(a, "id") for a in ledger["accounts"]]
    stamps = np.sort(transfers["timestamp"])
    seen = set()
    for T in [sc.steps[0][2]] + [int(stamps[i]) for i in (0, 5, len(stamps) // 3, len(stamps) // 2, len(stamps) - 1)]:
        records, _, complete = engine.lookup_accounts_at(ids, T)
        assert complete
        want = sums_by_ledger(records)
        rows, matched, complete = engine.get_ledger_balances(REQUEST, T)
        assert matched == len(REQUEST) and complete
        for row, L in zip(rows, REQUEST):
            sums, count = want.get(L, ([0, 0, 0, 0], 0))
            assert (balances_of(row), int(row["accounts"]), int(row["ledger"])) == (tuple(sums), count, L), (T, L)
        seen.add(rows.tobytes())
    assert len(seen) == 6


def test_wave_tile_and_word_edges(gpu_engine_factory):
    """One 600-event prepare committed in place (tbgpu_log_window), so log position = event index.
    Ledger 1's transfers sit on both sides of every wave and tile edge of the log scan, ledger 2's are
    interleaved so that a wave holds two groups, a pending transfer and its partial post straddle a wave
    edge and another pair the tile edge, two events fail, and the amounts carry across the 64-bit word.
    T at the positions around each edge holds "strictly above".  The first call follows
    tbgpu_commit_device_async without a sync."""
    engine = gpu_engine_factory(transfers_max=1 << 12)
    oracle = OracleEngine(64, 1 << 12)
    accounts = b"".join(pack_account(id=account_id(i), ledger=1 + (i & 1), code=1) for i in range(8))
    assert engine.commit(128, 10**12, accounts) == oracle.commit(128, 10**12, accounts) == b""
    amounts = [(1 << 64) - 1, 1 << 64, 1 << 100, 1]
    edges = (0, 63, 64, 127, 128, 255, 256, LOG_TILE - 1, LOG_TILE, 599)
    batch = []
    for i in range(600):
        L = 1 if i in edges or i % 3 == 0 else 2  # even accounts carry ledger 1, odd ones ledger 2
        dr = 2 * (i % 4) + (L - 1)
        cr = (dr + 2 + 2 * (i % 3)) % 8
        ev = dict(id=1000 + i, debit_account_id=account_id(dr), credit_account_id=account_id(cr), amount=1 + i, ledger=L, code=1)
        if i in edges:
            ev.update(amount=amounts[edges.index(i) % 4])
        elif i == 62:
            ev.update(amount=1 << 64, flags=PENDING)
        elif i == 65:
            ev.update(debit_account_id=0, credit_account_id=0, amount=(1 << 64) - 1, ledger=0, code=0, pending_id=1062, flags=POST)
        elif i == LOG_TILE - 2:
            ev.update(amount=1 << 100, flags=PENDING)
        elif i == LOG_TILE + 1:
            ev.update(debit_account_id=0, credit_account_id=0, amount=1 << 64, ledger=0, code=0, pending_id=1000 + LOG_TILE - 2,
                      flags=POST)
        elif i == 300:
            ev.update(amount=5, flags=PENDING)
        elif i == 320:
            ev.update(debit_account_id=0, credit_account_id=0, amount=0, ledger=0, code=0, pending_id=1300, flags=VOID)
        elif i == 66:
            ev.update(id=0)
        elif i == 254:
            ev.update(id=1000 + 64, amount=77)
        batch.append(pack_transfer(**ev))
    body = b"".join(batch)
    ts = 10**12 + 1000
    expected = oracle.commit(129, ts, body)
    assert np.frombuffer(expected, dtype=np.uint32)[0::2].tolist() == [66, 254]  # exactly the planted events failed
    checker = LedgerBalances(oracle.export_transfers(), oracle.export_accounts())
    window = engine.log_window(600)
    engine.to_device(window, np.frombuffer(body, dtype=np.uint8))
    res, rb = engine.alloc(600 * 8), engine.alloc(4)
    engine.commit_device_async(129, [ts], [600], window, res, rb)
    # The query drains the pending call itself.
    first = ts - 600 + 1
    request = [1, 2, 0, 1]
    seen = set()
    around = sorted({e + d for e in edges for d in (-2, -1, 0, 1, 2) if 0 <= e + d < 600})
    for pos in around + [-1]:
        got = check(engine, checker, request, first + pos)
        assert got[0].tobytes()[:72] == got[3].tobytes()[:72]
        seen.add(balances_of(got[0]))
    assert len(seen) >= 20  # ledger 1's balances differ at nearly every position around an edge
    assert max(b[0] for b in seen) >> 64 and max(b[1] for b in seen) >> 64
    assert (0, 0, 0, 0) in seen
    assert engine.export_accounts().tobytes() == oracle.export_accounts().tobytes()
    n_reply = int(engine.to_host(rb, 4).view(np.uint32)[0])
    assert bytes(engine.to_host(res, n_reply)) == expected
    engine.free(res)
    engine.free(rb)


def test_set_and_bins_at_their_limit(gpu_engine_factory):
    """5,000 accounts over 1,024 ledgers spread over 32 bits, 2^32-1 among them, and 2,048 transfers
    after T that touch every ledger: more distinct ledgers in one workgroup than it has LDS bins.  A
    request is at most 1,024 positions, so the ledgers are asked once all 1,024, once 1,023 and ledger 0.
    2^127 on two accounts of one ledger wraps its sum out of 128 bits.  Then every account in one
    ledger: every lane of a wave in the same group."""
    rng = random.Random(9)
    ledgers = rng.sample(range(1, 2**32 - 1), LEDGERS_MAX - 1) + [2**32 - 1]
    n = 5000
    engine = gpu_engine_factory(accounts_max=1 << 14, transfers_max=1 << 12)
    one = gpu_engine_factory(accounts_max=1 << 14, transfers_max=1 << 12)
    for e, ledger_of in ((engine, lambda i: ledgers[i % LEDGERS_MAX]), (one, lambda i: 77)):
        body = b"".join(pack_account(id=account_id(i), ledger=ledger_of(i), code=1) for i in range(n))
        assert e.commit(128, 10**12, body) == b""
        T = 10**12 + 5
        body = b"".join(pack_transfer(id=10**6 + j, debit_account_id=account_id(j), credit_account_id=account_id(j + LEDGERS_MAX),
                                      amount=(1 << 64) - 1 - j, ledger=ledger_of(j), code=1, flags=PENDING if j % 3 == 0 else 0)
                        for j in range(2 * LEDGERS_MAX))
        assert e.commit(129, 2 * 10**12, body) == b""
    wrapped = ledgers[17]
    engine.set_balances(account_id(17), 1 << 127, 5, 0, 0)
    engine.set_balances(account_id(17 + LEDGERS_MAX), (1 << 127) + 3, 0, 0, 9)
    checker = LedgerBalances(engine.export_transfers(), engine.export_accounts())
    shuffled = ledgers[:]
    rng.shuffle(shuffled)
    with_all = [x for x in shuffled if x != ledgers[3]]
    with_all.insert(500, 0)
    for request in (shuffled, with_all):
        assert len(request) == LEDGERS_MAX
        for t in (0, T, 10**12 - 2000, 2 * 10**12 - 1000):
            rows = check(engine, checker, request, t)
            assert len(rows) == LEDGERS_MAX
        now = check(engine, checker, request, 0)
        assert {c for c, x in zip(now["accounts"].tolist(), request) if x} == {4, 5}
        assert int(now[request.index(wrapped)]["debits_pending_hi"]) == 0  # 2^127 + 2^127 + 3 wrapped
    assert int(check(engine, checker, with_all, 0)[500]["accounts"]) == n
    # One ledger: a single group in every wave, with and without the every-ledger bin, and a miss.
    checker = LedgerBalances(one.export_transfers(), one.export_accounts())
    for request in ([77], [0], [78, 77, 0, 77]):
        for t in (0, T, 2 * 10**12 - 1000):
            rows = check(one, checker, request, t)
        assert int(rows[-1]["accounts"]) == n
    # One ledger more is invalid, and nothing is written.
    src = ctypes.create_string_buffer(ledgers_body(ledgers + [5]), 4 * (LEDGERS_MAX + 1))
    out = ctypes.create_string_buffer(b"\xAB" * 1024, 1024)
    res = _lib.tbgpu_query_result(count=77, complete=77, matched=77)
    assert engine.lib.tbgpu_get_ledger_balances(engine.h, T, src, LEDGERS_MAX + 1, out, 8, ctypes.byref(res)) == _lib.STATUS_INVALID
    assert out.raw == b"\xAB" * 1024 and (res.count, res.complete, res.matched) == (77, 77, 77)


def test_hot_ledger_over_several_workgroups(gpu_engine_factory):
    """One ledger and 24,570 transfers in three prepares: three workgroups of the log scan
    (LOG_WORKGROUP positions each) add into one bin, with sums that carry across the 64-bit word."""
    engine = gpu_engine_factory(transfers_max=1 << 15)
    body = b"".join(pack_account(id=account_id(i), ledger=3, code=1) for i in range(6))
    assert engine.commit(128, 10**12, body) == b""
    per = 8190
    assert 3 * per > 2 * LOG_WORKGROUP + LOG_TILE
    for k in range(3):
        body = b"".join(pack_transfer(id=10**6 + k * per + j, debit_account_id=account_id(j % 6), credit_account_id=account_id((j + 1 + k) % 6),
                                      amount=(1 << 63) + j, ledger=3, code=1, flags=PENDING if j % 5 == 0 else 0)
                        for j in range(per))
        assert engine.commit(129, 10**12 + 10**6 * (k + 1), body) == b""
    transfers = engine.export_transfers()
    assert len(transfers) == 3 * per
    checker = LedgerBalances(transfers, engine.export_accounts())
    stamps = np.sort(transfers["timestamp"])
    answers = set()
    for pos in (3 * per // 2, 100, LOG_WORKGROUP - 1, LOG_WORKGROUP, 2 * LOG_WORKGROUP + 700, 3 * per - 1):
        for request in ([3], [0, 3, 4]):
            rows = check(engine, checker, request, int(stamps[pos]))
        answers.add(rows[1].tobytes())
        assert int(rows[1]["debits_posted_hi"]) or pos >= 3 * per - 2
    assert len(answers) == 6
    check(engine, checker, [0, 3, 4], 0)


def test_eviction_and_orphan_posts(ledger, gpu_engine_factory):
    """After eviction of an old prefix `complete` is 0 and the rows still equal the checker over the
    resident export.  With nothing evicted (transfers loaded without some pending transfers), an
    orphan post drops `complete` only when its ledger or 0 is requested and T is below it."""
    sc, transfers, accounts = ledger["sc"], ledger["transfers"], ledger["accounts"]
    evicted = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, evicted)
    evicted.checkpoint_delta()
    assert evicted.evict_transfers(300) > 0
    resident = evicted.export_transfers()
    checker = LedgerBalances(resident, evicted.export_accounts())
    stamps = np.sort(resident["timestamp"])
    for T in (0, int(stamps[0]) - 1, int(stamps[0]), int(stamps[len(stamps) // 2]), int(stamps[-1]), int(stamps[-1]) + 1):
        check(evicted, checker, REQUEST, T, evicted=True)
    # Orphans without an eviction.
    states = posted_states(transfers, ledger["posted"])
    pending = {u128(t, "id"): t for t in transfers if int(t["flags"]) & PENDING}
    posts = [t for t in transfers if int(t["flags"]) & POST and not int(t["flags"]) & PENDING
             and u128(t, "amount") < u128(pending[u128(t, "pending_id")], "amount")]
    assert len(posts) > 3
    orphan = posts[-1]
    L = int(orphan["ledger"])
    others = [x for x in LEDGERS if x != L]
    keep = np.array([u128(t, "id") != u128(orphan, "pending_id") for t in transfers])
    engine = gpu_engine_factory(transfers_max=1 << 14)
    engine.load_accounts(accounts)
    engine.load_transfers(transfers[keep], states[keep])
    engine.set_commit_timestamp(ledger["commit_timestamp"])
    checker = LedgerBalances(engine.export_transfers(), engine.export_accounts())
    at = int(orphan["timestamp"])
    assert checker.at([L], at - 1)[2] and checker.at([0], at - 1)[2] and not checker.at(others + [5], at - 1)[2]
    assert not checker.at([L, 0], at)[2]
    for request in ([L], [0], others + [5], REQUEST):
        for T in (at - 1, at, 1, 0):
            check(engine, checker, request, T)
    assert checker.at(REQUEST, at - 1)[0].tobytes() != ledger["checker"].at(REQUEST, at - 1)[0].tobytes()


CHAIN_FREE = dict(n_accounts=8, n_transfer_batches=4, batch_len=(100, 200), p_linked=0, p_limit=0, p_balancing=0,
                  p_pending=0.3, p_post_void=0.25)


def test_anchor_setup_action(gpu_engine_factory):
    """tbgpu_test_set_balances between two runs of commits: the rows follow the definition, anchored at
    the current balances; debits and credits need not agree then."""
    sc = make_scenario(17, ledgers=(1, 7), **CHAIN_FREE)
    half = len(sc.steps) - 2
    big = [(1 << 100) + 5, (1 << 64) + 1, (1 << 90) + 9, (1 << 64) - 1]
    oracle = OracleEngine(64, 1 << 12)
    engine = gpu_engine_factory(transfers_max=1 << 12)
    commit_all(sc, oracle, engine, steps=sc.steps[:half])
    for i, a in enumerate(oracle.export_accounts()):
        oracle.set_balances(u128(a, "id"), *[b + i for b in big])
        engine.set_balances(u128(a, "id"), *[b + i for b in big])
    at_setup = sums_by_ledger(oracle.export_accounts())
    commit_all(sc, oracle, engine, steps=sc.steps[half:])
    checker = LedgerBalances(engine.export_transfers(), engine.export_accounts())
    assert engine.export_accounts().tobytes() == oracle.export_accounts().tobytes()
    request = [7, 0, 1, 2]
    for step in sc.steps:
        check(engine, checker, request, step[2])
        check(engine, checker, request, step[2] - 3)
    rows = check(engine, checker, request, sc.steps[half - 1][2])
    for row, L in zip(rows, request):  # every T after the setup is the oracle's own past
        sums, count = at_setup.get(L, ([0, 0, 0, 0], 0))
        assert (balances_of(row), int(row["accounts"])) == (tuple(sums), count)
    assert balances_of(rows[0])[0] != balances_of(rows[0])[2]


def test_restart_and_unordered_log(gpu_engine_factory):
    """The accounts loaded (tbgpu_load_accounts), the newer half committed, then the older half loaded
    shuffled (tbgpu_load_transfers): records newer than T sit at lower log positions than older ones,
    and the T sweep still equals the checker."""
    kw = dict(n_accounts=8, n_transfer_batches=20, batch_len=(100, 300), p_pending=0.3, p_dup=0.05, p_linked=0.05,
              p_limit=0.0, p_balancing=0.0, p_invalid=0.05, id_space=1 << 40, ledgers=(1, 7))
    sa = make_scenario(31, p_post_void=0.25, **kw)
    last = sa.steps[-1][2]
    sb = make_scenario(32, p_post_void=0.25, start_ts=last + 10**9, **kw)
    acct_steps = [s for s in sa.steps if s[1] == 128]
    a_steps = [s for s in sa.steps if s[1] == 129]
    b_steps = [s for s in sb.steps if s[1] == 129]
    oracle = OracleEngine(64, 1 << 15)
    engine1 = gpu_engine_factory(transfers_max=1 << 15)
    engine2 = gpu_engine_factory(transfers_max=1 << 15)
    commit_all(sa, oracle, engine1, steps=acct_steps + a_steps)
    half_a = engine1.export_transfers()
    states = posted_states(half_a, engine1.export_posted())
    at_restart = sums_by_ledger(oracle.export_accounts())
    engine2.load_accounts(engine1.export_accounts())
    engine2.set_commit_timestamp(last)
    request = [7, 1, 0, 3]
    loaded = LedgerBalances(engine2.export_transfers(), engine2.export_accounts())
    assert check(engine2, loaded, request, last).tobytes() == check(engine2, loaded, request, 0).tobytes()
    commit_all(sb, oracle, engine2, steps=b_steps)
    order = np.random.default_rng(5).permutation(len(half_a))
    engine2.load_transfers(half_a[order], states[order])
    transfers = oracle.export_transfers()
    assert engine2.export_transfers().tobytes() == transfers.tobytes()
    assert len(half_a) > 500 and len(transfers) - len(half_a) > 500
    checker = LedgerBalances(engine2.export_transfers(), engine2.export_accounts())
    stamps = np.sort(transfers["timestamp"])
    answers = set()
    for T in [int(stamps[0]) - 1, int(stamps[0]), int(stamps[len(half_a) // 2]), int(half_a["timestamp"].max()), last, last + 1,
              int(stamps[len(half_a) + 50]), int(stamps[-1])] + [int(t) for t in stamps[::501]]:
        answers.add(check(engine2, checker, request, T).tobytes())
    assert len(answers) > 8
    rows = check(engine2, checker, request, last)  # at the restart point: what the oracle's accounts were then
    for row, L in zip(rows, request):
        sums, count = at_restart.get(L, ([0, 0, 0, 0], 0))
        assert (balances_of(row), int(row["accounts"])) == (tuple(sums), count)


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=["node2", "node3"])
def test_node(devices, ledger, gpu_engine_factory):
    sc, checker = ledger["sc"], ledger["checker"]
    single = gpu_engine_factory(transfers_max=1 << 14)
    engine = gpu_engine_factory(accounts_max=4096, transfers_max=1 << 14, pass_events_max=2048, pass_batches_max=16,
                                devices=devices)
    assert commit_all(sc, engine, single) == ledger["replies"]
    for T in ledger["stamps"]:
        got = check(engine, checker, REQUEST, T)
        assert got.tobytes() == single.get_ledger_balances(REQUEST, T)[0].tobytes()
    # `accounts` counts each account on its owner only, never a home's imported copies.
    now = check(engine, checker, REQUEST, 0)
    assert int(now[4]["accounts"]) == len(ledger["accounts"]) == engine.ledger_summary()["accounts"]
    T = sc.steps[len(sc.steps) // 2][2]
    for cap in (0, 3, len(REQUEST)):
        check(engine, checker, REQUEST, T, cap=cap)


def test_read_only_and_allocation_free(ledger, gpu_engine_factory):
    """40 calls around which the allocation counts, commit_timestamp, the exports and the commit-path
    counters stand still; one more inside an asynchronous write-back; then the next commit answers as
    the twin's.  (test_wave_tile_and_word_edges calls right after a tbgpu_commit_device_async.)"""
    sc, transfers = ledger["sc"], ledger["transfers"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    twin = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, engine, twin, steps=sc.steps[:-1])
    resident = engine.export_transfers()
    checker = LedgerBalances(resident, engine.export_accounts())
    before = (engine.commit_timestamp, engine.export_accounts().tobytes(), resident.tobytes(),
              engine.export_posted().tobytes())
    rng = random.Random(3)
    allocations, live = engine.lib.tbgpu_debug_allocations(), engine.lib.tbgpu_debug_live()
    stats = engine.stats()
    stamps = np.sort(resident["timestamp"])
    for _ in range(40):
        T = int(rng.choice((0, 1, stamps[len(stamps) // 3], stamps[-5], stamps[-1] + 7)))
        engine.get_ledger_balances(rng.sample(REQUEST, rng.choice((1, 3, len(REQUEST)))), T)
    assert (engine.lib.tbgpu_debug_allocations(), engine.lib.tbgpu_debug_live()) == (allocations, live)
    after = engine.stats()
    assert all(after[k] == stats[k] for k in ("passes", "events", "transfers", "accounts", "log_used"))
    assert before == (engine.commit_timestamp, engine.export_accounts().tobytes(), engine.export_transfers().tobytes(),
                      engine.export_posted().tobytes())
    # One between an asynchronous write-back's start and its wait leaves the delta alone.
    caps = (1 << 14, 1 << 14, 1 << 14)
    engine.checkpoint_delta_async(caps)
    allocations = engine.lib.tbgpu_debug_allocations()
    check(engine, checker, REQUEST, int(stamps[len(stamps) // 2]))
    assert engine.lib.tbgpu_debug_allocations() == allocations
    delta = engine.checkpoint_delta_wait()
    sync = twin.checkpoint_delta(caps)
    assert len(delta.transfers) == len(resident)
    assert delta.transfers.tobytes() == sync.transfers.tobytes() and delta.posted.tobytes() == sync.posted.tobytes()
    assert by_id(delta.accounts) == by_id(sync.accounts) and delta.created_after == sync.created_after
    # ... and the next commit still answers as the twin and the oracle did.
    _, op, ts, batch = sc.steps[-1]
    assert engine.commit(op, ts, b"".join(batch)) == twin.commit(op, ts, b"".join(batch)) == ledger["replies"][-1]
    check(engine, ledger["checker"], REQUEST, int(stamps[-1]))
    assert engine.commit_timestamp == ledger["commit_timestamp"]
    assert engine.export_transfers().tobytes() == transfers.tobytes()
    assert engine.export_accounts().tobytes() == ledger["accounts"].tobytes()


def test_on_an_engine_a_device_panic_stopped(gpu_engine_factory):
    """tests/test_gpu_alloc.py's way to a device panic (a post whose checked `-=` traps after the setup
    action zeroed the pending balance).  The stopped engine still answers."""
    engine = gpu_engine_factory()
    accounts = b"".join(pack_account(id=i, ledger=1 + (i > 2), code=1) for i in (1, 2, 3))
    assert engine.commit(128, 10, accounts) == b""
    assert engine.commit(129, 20, pack_transfer(id=10, debit_account_id=1, credit_account_id=2, amount=100, ledger=1, code=1,
                                                flags=PENDING)) == b""
    assert engine.commit(129, 25, pack_transfer(id=12, debit_account_id=2, credit_account_id=1, amount=7, ledger=1, code=1)) == b""
    healthy, matched, complete = engine.get_ledger_balances([1, 2], 20)
    assert matched == 2 and complete
    assert balances_of(healthy[0]) == (100, 0, 100, 0) and balances_of(healthy[1]) == (0, 0, 0, 0)
    assert healthy["accounts"].tolist() == [2, 1]
    engine.set_balances(1, 0, 0, 0, 0)
    with pytest.raises(EnginePanic):
        engine.commit(129, 30, pack_transfer(id=11, pending_id=10, flags=POST))
    with pytest.raises(EnginePanic, match="stopped"):
        engine.commit(129, 40, pack_transfer(id=13, debit_account_id=1, credit_account_id=2, amount=1, ledger=1, code=1))
    checker = LedgerBalances(engine.export_transfers(), engine.export_accounts())
    allocations = engine.lib.tbgpu_debug_allocations()
    for T in (0, 9, 10, 20, 24, 25):
        want, matched, _ = checker.at([2, 1, 0, 1], T)
        got, got_matched, _ = engine.get_ledger_balances([2, 1, 0, 1], T)
        assert got.tobytes() == want.tobytes() and got_matched == matched == 4
    assert engine.lib.tbgpu_debug_allocations() == allocations


def test_invalid_input(ledger, gpu_engine_factory):
    sc = ledger["sc"]
    engine = gpu_engine_factory(transfers_max=1 << 12)
    n = len(REQUEST)
    empty, matched, complete = engine.get_ledger_balances(REQUEST, 5)  # an empty engine: zero rows, one per position
    assert len(empty) == matched == n and complete and empty["ledger"].tolist() == REQUEST and not empty["accounts"].any()
    commit_all(sc, engine, steps=sc.steps[:4])
    T = sc.steps[2][2]
    valid, matched, complete = engine.get_ledger_balances(REQUEST, T)
    assert matched == len(valid) == n and complete and valid["accounts"].any()
    got, matched, complete = engine.get_ledger_balances(REQUEST, U64_MAX)
    assert len(got) == 0 and matched == 0 and complete
    got, matched, complete = engine.get_ledger_balances([], T)
    assert len(got) == 0 and matched == 0 and complete
    got, matched, complete = engine.get_ledger_balances(REQUEST, T, 0)  # cap = 0: nothing written, matched stays
    assert len(got) == 0 and matched == n and complete
    fn = engine.lib.tbgpu_get_ledger_balances
    src = ctypes.create_string_buffer(ledgers_body(REQUEST), 4 * n)
    sentinel = b"\xAB" * (128 * n)
    out = ctypes.create_string_buffer(sentinel, len(sentinel))
    res = _lib.tbgpu_query_result(count=77, complete=77, matched=77)
    untouched = lambda: out.raw == sentinel and (res.count, res.complete, res.matched) == (77, 77, 77)
    assert fn(engine.h, T, src, 0, out, n, ctypes.byref(res)) == _lib.STATUS_OK and untouched()
    assert fn(engine.h, T, None, 0, None, 0, None) == _lib.STATUS_OK
    assert fn(engine.h, T, None, n, out, n, ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, T, src, n, None, n, ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, T, src, n, out, n, None) == _lib.STATUS_INVALID and out.raw == sentinel
    assert fn(engine.h, T, src, LEDGERS_MAX + 1, out, n, ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, U64_MAX, src, n, out, n, ctypes.byref(res)) == _lib.STATUS_OK
    assert out.raw == sentinel and (res.count, res.matched, res.complete) == (0, 0, 1)
    assert fn(engine.h, T, src, n, out, 0, ctypes.byref(res)) == _lib.STATUS_OK
    assert out.raw == sentinel and (res.count, res.matched, res.complete) == (0, n, 1)
    assert fn(engine.h, T, src, n, out, n, ctypes.byref(res)) == _lib.STATUS_OK
    assert res.count == n and out.raw == valid.tobytes()
