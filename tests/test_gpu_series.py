"""get_account_statement_series (include/tbgpu.h tbgpu_get_account_statement_series, csrc/k_series.h):
for the accounts a caller names and consecutive buckets (bounds[k], bounds[k+1]], one statement row per
(account, bucket) from one scan of the HBM log.  Rows, `matched` and `complete` are compared byte for
byte with the checker of tests/harness/series.py (itself held to get_account_statements' checker in
tests/test_series_checkers.py) and with the engine's own single calls."""
import ctypes
import random

import numpy as np
import pytest

from tests.harness.balances import balances_of, u128
from tests.harness.oracle import OracleEngine
from tests.harness.series import Series, bounds_sweep
from tests.harness.shard_double import homes_of
from tests.harness.statements import SIDES, balances, ids_body, request_of, sums
from tests.harness.workload import account_id, make_scenario
from tests.test_gpu_query import SCENARIO, by_id, commit_all, posted_states
from tigerbeetle_amd import _lib
from tigerbeetle_amd._lib import EnginePanic
from tigerbeetle_amd.types import STATEMENT_DTYPE, U64_MAX, TransferFlags, pack_account, pack_transfer

pytestmark = pytest.mark.gpu

PENDING = int(TransferFlags.pending)
POST = int(TransferFlags.post_pending_transfer)
VOID = int(TransferFlags.void_pending_transfer)
MAX = 4095
ROW = 256
ABSENT = (account_id(5000), account_id(5001))
NOTHING = ((0, 0, 0, 0), (0, 0, 0, 0))


def fitting(ids, bounds):
    """The request, thinned where ids x buckets would pass 4,095 rows: absent ids, reserved ids and
    repeats stay in it."""
    return ids if len(ids) * (len(bounds) - 1) <= MAX else ids[::3] + ids[-10:]


def check(engine, checker, ids, bounds, evicted=False, cap=None):
    """One request: rows, matched and complete as the checker has them."""
    want, matched, orphan = checker.of(ids, bounds, cap)
    got, got_matched, got_complete = engine.get_account_statement_series(ids, bounds, cap)
    assert len(got) == len(want), (bounds, len(got), len(want))
    if got.tobytes() != want.tobytes():
        bad = [n for n in range(len(got)) if got[n].tobytes() != want[n].tobytes()]
        raise AssertionError("rows differ: %d of %d, the first %s, %d buckets" % (len(bad), len(got), bad[:8], len(bounds) - 1))
    assert (got_matched, got_complete) == (matched, not evicted and not orphan), bounds
    return got


def check_single_calls(engine, ids, bounds, got):
    """Every bucket's rows are the engine's own get_account_statements over that bucket, wherever that
    call yields a row; with one bucket the whole answer is."""
    n_buckets = len(bounds) - 1
    found = len(got) // n_buckets
    for k in range(n_buckets):
        single, matched, complete = engine.get_account_statements(ids, bounds[k], bounds[k + 1])
        mine = {}
        for r in range(found):
            mine.setdefault(u128(got[r * n_buckets + k], "id"), got[r * n_buckets + k].tobytes())
        assert all(mine[u128(row, "id")] == row.tobytes() for row in single), (bounds, k)
        if k == n_buckets - 1:
            assert matched == found
        if n_buckets == 1:
            assert single.tobytes() == got.tobytes()
            assert (matched, complete) == engine.get_account_statement_series(ids, bounds)[1:]


def raw_call(engine, bounds, ids, n, cap, n_buckets=None, fill=b"\xAB"):
    """The C call into a sentinel-filled buffer: (status, result, the buffer's bytes)."""
    n_buckets = len(bounds) - 1 if n_buckets is None else n_buckets
    rows = max(len(ids) * max(n_buckets, 1), 1)
    src = ctypes.create_string_buffer(ids_body(ids), 16 * len(ids))
    out = ctypes.create_string_buffer(fill * (ROW * rows), ROW * rows)
    edges = (ctypes.c_uint64 * max(len(bounds), 1))(*bounds)
    res = _lib.tbgpu_query_result(count=77, complete=77, matched=77)
    status = engine.lib.tbgpu_get_account_statement_series(engine.h, edges, n_buckets, src, n, out, cap, ctypes.byref(res))
    return status, (res.count, res.complete, res.matched), out.raw


@pytest.fixture(scope="module")
def ledger():
    """test_gpu_query.py's scenario, the oracle that committed all of it, its exports and the checker
    over them (never changed)."""
    sc = make_scenario(2025, **SCENARIO)
    oracle = OracleEngine(4096, 1 << 15)
    replies = commit_all(sc, oracle)
    transfers, accounts = oracle.export_transfers(), oracle.export_accounts()
    return dict(sc=sc, replies=replies, transfers=transfers, accounts=accounts, commit_timestamp=oracle.commit_timestamp,
                posted=oracle.export_posted(), checker=Series(transfers, accounts), ids=request_of(accounts, ABSENT),
                sweep=bounds_sweep(sc.steps, transfers, oracle.commit_timestamp))


def test_single_engine_sweep(ledger, gpu_engine_factory):
    sc, checker, ids = ledger["sc"], ledger["checker"], ledger["ids"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    assert commit_all(sc, engine) == ledger["replies"]
    assert engine.commit_timestamp == ledger["commit_timestamp"]
    assert {1, 2, 3, 7, 64} <= {len(b) - 1 for b in ledger["sweep"]}
    partial = empty = 0
    for bounds in ledger["sweep"]:
        request = fitting(ids, bounds)
        got = check(engine, checker, request, bounds)
        check_single_calls(engine, request, bounds, got)
        n_buckets = len(bounds) - 1
        assert len(got) > 0 and len(got) % n_buckets == 0
        for n, row in enumerate(got):
            k = n % n_buckets
            if k + 1 < n_buckets:
                assert balances(row, "closing") == balances(got[n + 1], "opening")
            empty += bounds[k] == bounds[k + 1] != 0 and sums(row) == NOTHING
            partial += any(u128(row, s + "_pending_out") and u128(row, s + "_posted_in")
                           and u128(row, s + "_pending_out") != u128(row, s + "_posted_in") for s in SIDES)
        # The last bucket's closing is lookup_accounts_at at the last bound.
        at_last = engine.lookup_accounts_at(request, bounds[-1])[0]
        assert [balances(r, "closing") for r in got[n_buckets - 1::n_buckets]] == [balances_of(a) for a in at_last]
    assert partial > 0 and empty > 0
    # out_cap_rows cuts the answer in row order, inside an account too, and nothing past count rows is written.
    bounds = ledger["sweep"][7]
    whole = check(engine, checker, ids, bounds)
    matched = len(whole)
    assert len(bounds) == 4 and matched > 30
    for cap in (0, 1, 4, 3 * 5 + 2, matched, matched + 3):
        check(engine, checker, ids, bounds, cap=cap)
        status, (count, complete, m), raw = raw_call(engine, bounds, ids, len(ids), cap)
        assert status == _lib.STATUS_OK and (count, complete, m) == (min(cap, matched), 1, matched)
        assert raw[:ROW * count] == whole[:count].tobytes() and raw[ROW * count:] == b"\xAB" * (len(raw) - ROW * count)


def test_tile_wave_and_workgroup_edges(gpu_engine_factory):
    """tests/test_gpu_statements.py's construction: two prepares of 4,200 events committed in place, so
    log position = event index and timestamp = first + position.  Account A's records sit around the
    scan's wave edge (63/64), tile edge (511/512) and workgroup edge (8191/8192), and in every lane of
    the wave at 1024-1087; with a pending transfer and its partial post, another and its void, failing
    events that name A, and amounts whose sums carry across the 64-bit word.  Bounds sit at, one below
    and one above every planted edge; one request cuts the wave of A alone into six buckets with
    bounds[0] and the last bound inside it, so that wave holds records below bounds[0], six buckets
    and the tail of one account."""
    engine = gpu_engine_factory(transfers_max=1 << 14)
    oracle = OracleEngine(64, 1 << 14)
    n_acc, A, half = 8, account_id(0), 4200
    accounts = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(n_acc))
    assert engine.commit(128, 10**12, accounts) == oracle.commit(128, 10**12, accounts) == b""
    rng = random.Random(11)
    amounts = [(1 << 64) - 1, 1 << 64, 1 << 100, 1, (1 << 64) - 7]
    planted = [62, 63, 64, 65, 255, 256, 510, 511, 512, 513, 4199, 4200, 8190, 8191, 8192, 8193, 8399] + list(range(1024, 1088))
    batch = []
    for i in range(2 * half):
        dr = 1 + rng.randrange(n_acc - 1)
        cr = 1 + (dr + rng.randrange(n_acc - 2)) % (n_acc - 1)  # another account, never A
        ev = dict(id=1000 + i, debit_account_id=account_id(dr), credit_account_id=account_id(cr), amount=1 + i, ledger=1, code=1)
        other = account_id(1 + i % (n_acc - 1))
        if i in planted:
            ev.update(amount=amounts[i % len(amounts)], flags=PENDING if i % 7 == 3 else 0)
            ev.update(debit_account_id=A, credit_account_id=other) if i % 2 == 0 else ev.update(debit_account_id=other, credit_account_id=A)
        elif i == 10:
            ev.update(debit_account_id=A, credit_account_id=other, amount=1 << 100, flags=PENDING)
        elif i == 514:
            ev.update(debit_account_id=0, credit_account_id=0, amount=(1 << 64) - 1, pending_id=1010, flags=POST)
        elif i == 61:
            ev.update(debit_account_id=other, credit_account_id=A, amount=1 << 64, flags=PENDING)
        elif i == 8189:
            ev.update(debit_account_id=0, credit_account_id=0, amount=0, pending_id=1061, flags=VOID)
        elif i == 66:
            ev.update(debit_account_id=A, credit_account_id=other, id=0)
        elif i == 8194:
            ev.update(debit_account_id=A, credit_account_id=other, id=1000 + 64)
        batch.append(pack_transfer(**ev))
    bodies = [b"".join(batch[:half]), b"".join(batch[half:])]
    stamps = [10**12 + 10**6, 10**12 + 10**6 + half]
    expected = b"".join(oracle.commit(129, ts, body) for ts, body in zip(stamps, bodies))
    failed = np.frombuffer(expected, dtype=np.uint32)[0::2].tolist()
    assert failed == [66, 8194 - half]  # exactly the planted events failed
    exported = oracle.export_transfers()
    first = stamps[0] - half + 1
    at = lambda pos: first + pos
    assert len(exported) == 2 * half - 2 and int(exported["timestamp"].max()) == at(2 * half - 1)
    checker = Series(exported, oracle.export_accounts())
    window = engine.log_window(2 * half)
    engine.to_device(window, np.frombuffer(bodies[0] + bodies[1], dtype=np.uint8))
    res, rb = engine.alloc(2 * half * 8), engine.alloc(8)
    engine.commit_device_async(129, stamps, [half, half], window, res, rb)
    # The query drains the pending call itself.
    ids = [account_id(i) for i in range(n_acc)] + [A, account_id(3)]
    edges = [62, 63, 64, 65, 255, 256, 510, 511, 512, 513, 4199, 4200, 8190, 8191, 8192, 8193]
    marks = sorted({e + d for e in edges for d in (-1, 0, 1)})
    in_wave = [at(p) for p in (1030, 1035, 1040, 1041, 1050, 1070, 1080)]
    requests = [[at(p) for p in marks], [0] + [at(p) for p in marks] + [0], in_wave, [at(10)] + in_wave + [at(8189), at(8194), 0],
                [at(p) for p in (9, 10, 61, 513, 514, 8188, 8189, 8399)]]
    seen = set()
    for bounds in requests:
        got = check(engine, checker, ids, bounds)
        n_buckets = len(bounds) - 1
        assert got[:n_buckets].tobytes() == got[n_acc * n_buckets:(n_acc + 1) * n_buckets].tobytes()  # A, and A again
        seen.update(row.tobytes() for row in got[:n_buckets])
    assert len(seen) > 25  # A's rows move with the buckets
    got = check(engine, checker, ids, in_wave)
    check_single_calls(engine, ids, in_wave, got)
    check_single_calls(engine, ids, requests[3], check(engine, checker, ids, requests[3]))
    a_rows = got[:6]
    counts = [int(r["debit_transfers"]) + int(r["credit_transfers"]) for r in a_rows]
    assert counts == [5, 5, 1, 9, 20, 10]  # every record of the wave between the first and the last bound, A's alone
    assert any(u128(r, "debits_posted_in") >> 64 for r in a_rows) and any(u128(r, "credits_posted_in") >> 64 for r in a_rows)
    a_rows = check(engine, checker, [A], requests[4])
    assert u128(a_rows[3], "debits_pending_out") == 1 << 100 and u128(a_rows[3], "debits_posted_in") == (1 << 64) - 1  # the partial post
    assert sums(a_rows[3]) == ((0, 1 << 100, (1 << 64) - 1, 1), (0, 0, 0, 0))
    assert sums(a_rows[5]) == ((0, 0, 0, 0), (0, 1 << 64, 0, 1))  # the void
    assert engine.export_accounts().tobytes() == oracle.export_accounts().tobytes()
    assert engine.export_transfers().tobytes() == exported.tobytes()
    engine.free(res)
    engine.free(rb)


def test_more_keys_than_lds_bins(gpu_engine_factory):
    """8 accounts and 511 buckets over one 4,088-transfer prepare in which every account debits and
    credits in every bucket: 4,088 distinct keys inside one workgroup's 8,192 records, far more than
    its claimed LDS bins — bins are claimed, handed over at the workgroup's end and, once both of a
    key's slots are taken, bypassed for HBM."""
    n_acc, n_buckets = 8, 511
    engine = gpu_engine_factory(transfers_max=1 << 13)
    body = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(n_acc))
    assert engine.commit(128, 10**12, body) == b""
    body = b"".join(pack_transfer(id=10**6 + j, debit_account_id=account_id(j % n_acc),
                                  credit_account_id=account_id((j + 1 + (j // n_acc) % (n_acc - 1)) % n_acc), amount=(1 << 63) + j,
                                  ledger=1, code=1, flags=PENDING if (j // n_acc) % 3 == 0 else 0) for j in range(n_acc * n_buckets))
    assert engine.commit(129, 2 * 10**12, body) == b""
    transfers = engine.export_transfers()
    assert len(transfers) == n_acc * n_buckets
    checker = Series(transfers, engine.export_accounts())
    stamps = np.sort(transfers["timestamp"])
    bounds = [int(stamps[0]) - 1] + [int(t) for t in stamps[n_acc - 1::n_acc]]
    assert len(bounds) == n_buckets + 1
    ids = [account_id(i) for i in range(n_acc - 1, -1, -1)]
    got = check(engine, checker, ids, bounds)
    assert len(got) == n_acc * n_buckets == 4088
    assert (got["debit_transfers"] == 1).all() and (got["credit_transfers"] == 1).all()
    # The same with the first and the last 100 buckets cut off: records below bounds[0] and a tail.
    check(engine, checker, ids, bounds[100:-100])


@pytest.fixture(scope="module")
def wide():
    """4,200 accounts and two 4,000-transfer prepares in which 600 accounts debit again and again
    (tests/test_gpu_statements.py's shape): the transfers as packed, shared by the tests below."""
    n_acc, hot = 4200, 600
    accounts = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(n_acc))
    bodies = [b"".join(pack_transfer(id=10**6 + 4000 * k + j, debit_account_id=account_id((7 * j) % hot),
                                     credit_account_id=account_id(hot + (j * 13 + k) % (n_acc - hot)), amount=(1 << 63) + j, ledger=1,
                                     code=1, flags=PENDING if (j // hot) % 3 == 0 else 0) for j in range(4000)) for k in range(2)]
    return dict(n_acc=n_acc, hot=hot, accounts=accounts, bodies=bodies)


def test_hot_accounts_and_capacity_shapes(wide, gpu_engine_factory):
    """600 hot accounts x 6 buckets, more active accounts than LDS bins in one workgroup; then the four
    shapes with ids x buckets = 4,095 exactly: 4,095 x 1, 1 x 4,095 (a bound per record over part of
    the log: the emit's suffix sum crosses 16 workgroups), 63 x 65 (it crosses waves) and 585 x 7.
    4,096 rows and no bucket are invalid and write nothing."""
    n_acc, hot = wide["n_acc"], wide["hot"]
    engine = gpu_engine_factory(accounts_max=1 << 13, transfers_max=1 << 14)
    assert engine.commit(128, 10**12, wide["accounts"]) == b""
    for k, body in enumerate(wide["bodies"]):
        assert engine.commit(129, 2 * 10**12 + k * 10**6, body) == b""
    transfers = engine.export_transfers()
    assert len(transfers) == 8000
    checker = Series(transfers, engine.export_accounts())
    stamps = [int(t) for t in np.sort(transfers["timestamp"])]
    hot_ids = [account_id(i) for i in range(hot - 1, -1, -1)]
    six = [stamps[900], stamps[1700], stamps[3100], stamps[3999], stamps[4000], stamps[6100], stamps[7300]]
    got = check(engine, checker, hot_ids, six)
    assert len(got) == 6 * hot
    assert ((got["debit_transfers"].reshape(hot, 6) > 0).sum(axis=0) == hot).sum() >= 5  # every hot account is active in the buckets
    assert (got["closing_debits_posted_hi"] > 0).any()
    check(engine, checker, hot_ids, [0] + six[1:4] + [0])
    rng = random.Random(9)
    exact = [account_id(i) for i in range(MAX)]
    rng.shuffle(exact)
    shapes = [(exact, [stamps[1700], stamps[6100]]),                                          # 4,095 x 1
              ([account_id(7)], stamps[2000:2000 + MAX + 1]),                                 # 1 x 4,095
              (exact[:40] + hot_ids[:23], stamps[300:300 + 66 * 100:100]),                    # 63 x 65
              (hot_ids[:300] + exact[:285], [0] + stamps[1000:7000:1000] + [0])]              # 585 x 7
    for ids, bounds in shapes:
        assert len(ids) * (len(bounds) - 1) == MAX
        got = check(engine, checker, ids, bounds)
        assert len(got) == MAX
    one = check(engine, checker, [account_id(7)], stamps[2000:2000 + MAX + 1])
    assert int(one["debit_transfers"].sum()) >= 6 and balances(one[0], "opening") != balances(one[-1], "closing")
    check_single_calls(engine, exact, shapes[0][1], check(engine, checker, exact, shapes[0][1]))
    # One row too many, and no bucket.
    ids64 = exact[:64]
    status, result, raw = raw_call(engine, stamps[100:165], ids64, 64, 4096)
    assert status == _lib.STATUS_INVALID and result == (77, 77, 77) and raw == b"\xAB" * len(raw)
    status, result, raw = raw_call(engine, stamps[100:101], ids64, 64, 64, n_buckets=0)
    assert status == _lib.STATUS_INVALID and result == (77, 77, 77) and raw == b"\xAB" * len(raw)
    status, result, raw = raw_call(engine, stamps[100:102], exact + [account_id(MAX)], MAX + 1, 8)
    assert status == _lib.STATUS_INVALID and result == (77, 77, 77) and raw == b"\xAB" * len(raw)


def test_eviction_and_orphaned_posts(ledger, gpu_engine_factory):
    """After tbgpu_evict_transfers of an old prefix `complete` is 0 and the rows are the checker's over
    the resident export, an orphan post among them.  And posts whose pending transfers were never
    loaded, with nothing evicted: `complete` drops exactly when one lies above bounds[0], in whatever
    bucket, or in the tail."""
    transfers, accounts, ids = ledger["transfers"], ledger["accounts"], ledger["ids"]
    evicted = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(ledger["sc"], evicted)
    evicted.checkpoint_delta()
    assert evicted.evict_transfers(700) > 0
    resident = evicted.export_transfers()
    checker = Series(resident, evicted.export_accounts())
    stamps = [int(t) for t in np.sort(resident["timestamp"])]
    third, half = stamps[len(stamps) // 3], stamps[len(stamps) // 2]
    assert checker.of(ids, [stamps[0], 0])[2] and len(stamps) > 100  # an orphan post is resident
    for bounds in ([0, third, 0], [stamps[0] - 1, third, half, stamps[-1]], [half, stamps[-5], 0], [1, stamps[0] - 1, third]):
        check(evicted, checker, ids, bounds, evicted=True)
    # Loaded without some pending transfers: nothing was evicted, the orphans alone drop `complete`.
    states = posted_states(transfers, ledger["posted"])
    pending = {u128(t, "id"): t for t in transfers if int(t["flags"]) & PENDING}
    posts = [t for t in transfers if int(t["flags"]) & POST and not int(t["flags"]) & PENDING
             and u128(t, "amount") < u128(pending[u128(t, "pending_id")], "amount")]
    assert len(posts) > 3
    lost = {u128(p, "pending_id") for p in posts[len(posts) // 2:]}
    keep = np.array([u128(t, "id") not in lost for t in transfers])
    engine = gpu_engine_factory(transfers_max=1 << 14)
    engine.load_accounts(accounts)
    engine.load_transfers(transfers[keep], states[keep])
    engine.set_commit_timestamp(ledger["commit_timestamp"])
    checker = Series(engine.export_transfers(), engine.export_accounts())
    first_orphan = min(int(p["timestamp"]) for p in posts[len(posts) // 2:])
    newest_orphan = max(int(p["timestamp"]) for p in posts[len(posts) // 2:])
    verdicts = []
    for bounds in ([1, first_orphan - 1], [1, first_orphan - 1, first_orphan], [first_orphan - 1, first_orphan, newest_orphan - 1],
                   [newest_orphan - 2, newest_orphan - 1], [newest_orphan, 0], [0, first_orphan, 0]):
        check(engine, checker, ids, bounds)
        verdicts.append(checker.of(ids, bounds)[2])
    # The first request's tail holds every orphan, the fourth's the newest: one value for the whole answer.
    assert verdicts == [True, True, True, True, False, True]
    narrow = engine.get_account_statements(ids, newest_orphan - 2, newest_orphan - 1)
    assert narrow[2] is False  # (the single call counts its tail too)


CHAIN_FREE = dict(n_accounts=8, n_transfer_batches=4, batch_len=(100, 200), p_linked=0, p_limit=0, p_balancing=0,
                  p_pending=0.3, p_post_void=0.25)


def test_anchor_setup_action(gpu_engine_factory):
    """tbgpu_test_set_balances between two runs of commits: the answers are anchored at the engine's
    current balances, and a bucket after the setup is the oracle's own past."""
    sc = make_scenario(17, **CHAIN_FREE)
    half = len(sc.steps) - 2
    big = [(1 << 100) + 5, (1 << 64) + 1, (1 << 90) + 9, (1 << 64) - 1]
    oracle = OracleEngine(64, 1 << 12)
    engine = gpu_engine_factory(transfers_max=1 << 12)
    commit_all(sc, oracle, engine, steps=sc.steps[:half])
    ids = request_of(oracle.export_accounts(), ABSENT)
    for i, a in enumerate(oracle.export_accounts()):
        oracle.set_balances(u128(a, "id"), *[b + i for b in big])
        engine.set_balances(u128(a, "id"), *[b + i for b in big])
    at_setup = {u128(a, "id"): balances_of(a) for a in oracle.export_accounts()}
    commit_all(sc, oracle, engine, steps=sc.steps[half:half + 1])
    after_one = {u128(a, "id"): balances_of(a) for a in oracle.export_accounts()}
    commit_all(sc, oracle, engine, steps=sc.steps[half + 1:])
    checker = Series(engine.export_transfers(), engine.export_accounts())
    assert engine.export_accounts().tobytes() == oracle.export_accounts().tobytes()
    boundaries = [s[2] for s in sc.steps]
    n_buckets = len(boundaries) - 1
    rows = check(engine, checker, ids, boundaries)
    check(engine, checker, ids, [b - 3 for b in boundaries] + [0])
    check(engine, checker, ids, [0] + boundaries[2:])
    mine = rows[half - 1::n_buckets]  # the bucket of the prepare right after the setup
    assert len(mine) == len(at_setup) + 6
    assert all(balances(r, "opening") == at_setup[u128(r, "id")] and balances(r, "closing") == after_one[u128(r, "id")] for r in mine)
    assert at_setup != after_one


def test_restart_and_unordered_log(gpu_engine_factory):
    """The accounts loaded, the newer half committed, then the older half loaded shuffled: older
    timestamps sit behind newer ones in the log, records of every bucket share tiles, accounts are
    younger than the early buckets, and the answers still equal the checker."""
    kw = dict(n_accounts=8, n_transfer_batches=20, batch_len=(100, 300), p_pending=0.3, p_dup=0.05, p_linked=0.05,
              p_limit=0.0, p_balancing=0.0, p_invalid=0.05, id_space=1 << 40)
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
    at_restart = {u128(a, "id"): balances_of(a) for a in oracle.export_accounts()}
    engine2.load_accounts(engine1.export_accounts())
    engine2.set_commit_timestamp(last)
    ids = request_of(oracle.export_accounts(), ABSENT)
    # Restarted from the balances alone, an empty log: every bucket opens and closes on the loaded balances.
    loaded = Series(engine2.export_transfers(), engine2.export_accounts())
    rows = check(engine2, loaded, ids, [0, last // 2, last])
    assert len(rows) == 2 * (len(ids) - 4) and all(balances(r, "opening") == balances(r, "closing") == at_restart[u128(r, "id")] for r in rows)
    commit_all(sb, oracle, engine2, steps=b_steps)
    order = np.random.default_rng(5).permutation(len(half_a))
    engine2.load_transfers(half_a[order], states[order])
    transfers = oracle.export_transfers()
    assert engine2.export_transfers().tobytes() == transfers.tobytes()
    assert len(half_a) > 500 and len(transfers) - len(half_a) > 500
    checker = Series(engine2.export_transfers(), engine2.export_accounts())
    stamps = [int(t) for t in np.sort(transfers["timestamp"])]
    created = sorted(int(a["timestamp"]) for a in oracle.export_accounts())
    marks = [0, created[0] - 1, created[0], created[-1], stamps[0], stamps[len(half_a) // 2], int(half_a["timestamp"].max()), last,
             last + 1, stamps[len(half_a) + 50], stamps[-1], 0]
    rows = check(engine2, checker, ids, marks)
    young = [r for r in rows[0::len(marks) - 1] if sums(r) == NOTHING]
    assert len(young) == len(ids) - 4  # nobody existed in the first bucket, and everybody has its row
    check_single_calls(engine2, ids, marks, rows)
    oldest = check(engine2, checker, ids, marks[:3])  # only the oldest account, as often as it is named
    assert 0 < len(oldest) <= 2 * 3 and len({u128(r, "id") for r in oldest}) == 1
    check(engine2, checker, ids[:8], stamps[200:-200:37])
    # A bucket that ends at the restart point closes on what the oracle's accounts were then.
    rows = check(engine2, checker, ids, [stamps[100], last, stamps[-1]])
    assert all(balances(r, "closing") == at_restart[u128(r, "id")] for r in rows[0::2])


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=["node2", "node3"])
def test_node(devices, ledger, gpu_engine_factory):
    sc, checker, ids, transfers = ledger["sc"], ledger["checker"], ledger["ids"], ledger["transfers"]
    world = len(devices)
    posts = transfers[(transfers["flags"] & POST) != 0]
    home = homes_of(np.stack([posts["id_lo"], posts["id_hi"]], axis=1), world)
    pending_home = homes_of(np.stack([posts["pending_id_lo"], posts["pending_id_hi"]], axis=1), world)
    assert np.any(home != pending_home)  # a post reads its pending transfer on another shard
    single = gpu_engine_factory(transfers_max=1 << 14)
    engine = gpu_engine_factory(accounts_max=4096, transfers_max=1 << 14, pass_events_max=2048, pass_batches_max=16,
                                devices=devices)
    assert commit_all(sc, engine, single) == ledger["replies"]
    for bounds in ledger["sweep"]:
        request = fitting(ids, bounds)
        got = check(engine, checker, request, bounds)
        assert got.tobytes() == single.get_account_statement_series(request, bounds)[0].tobytes()
    bounds = ledger["sweep"][7]
    for cap in (0, 4, 3 * 5 + 2, 3 * len(ids)):
        check(engine, checker, ids, bounds, cap=cap)
    status, result, raw = raw_call(engine, bounds, ids, len(ids), 5)
    assert status == _lib.STATUS_OK and result[0] == 5 and raw[5 * ROW:] == b"\xAB" * (len(raw) - 5 * ROW)
    one = ledger["sweep"][1]
    assert engine.get_account_statement_series(ids, one)[0].tobytes() == engine.get_account_statements(ids, *one)[0].tobytes()


def test_read_only_and_allocation_free(ledger, gpu_engine_factory):
    """50 calls around which the allocation count, commit_timestamp, the exports and the commit-path
    counters of tbgpu_get_stats stand still; one more inside an asynchronous write-back; then the
    next commit answers as the oracle did."""
    sc, transfers, ids = ledger["sc"], ledger["transfers"], ledger["ids"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    twin = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, engine, twin, steps=sc.steps[:-1])
    resident = engine.export_transfers()
    checker = Series(resident, engine.export_accounts())
    before = (engine.commit_timestamp, engine.export_accounts().tobytes(), resident.tobytes(), engine.export_posted().tobytes())
    rng = random.Random(3)
    allocations = engine.lib.tbgpu_debug_allocations()
    stats = engine.stats()
    stamps = [int(t) for t in np.sort(resident["timestamp"])]
    marks = [1, stamps[len(stamps) // 3], stamps[-5], stamps[-1] + 7]
    for _ in range(50):
        inner = sorted(rng.sample(marks, rng.choice((0, 1, 3))))
        bounds = [rng.choice((0, 1))] + inner + [rng.choice((0, stamps[-1] + 7))]
        engine.get_account_statement_series(rng.sample(ids, rng.choice((1, 5, len(ids)))), bounds)
    assert engine.lib.tbgpu_debug_allocations() == allocations
    after = engine.stats()
    assert all(after[k] == stats[k] for k in ("passes", "events", "transfers", "accounts", "log_used"))
    assert before == (engine.commit_timestamp, engine.export_accounts().tobytes(), engine.export_transfers().tobytes(),
                      engine.export_posted().tobytes())
    # One between an asynchronous write-back's start and its wait leaves the delta alone.
    caps = (1 << 14, 1 << 14, 1 << 14)
    engine.checkpoint_delta_async(caps)
    allocations = engine.lib.tbgpu_debug_allocations()
    check(engine, checker, ids, [stamps[len(stamps) // 3], stamps[len(stamps) // 2], stamps[-5]])
    assert engine.lib.tbgpu_debug_allocations() == allocations
    delta = engine.checkpoint_delta_wait()
    sync = twin.checkpoint_delta(caps)
    assert len(delta.transfers) == len(resident)
    assert delta.transfers.tobytes() == sync.transfers.tobytes() and delta.posted.tobytes() == sync.posted.tobytes()
    assert by_id(delta.accounts) == by_id(sync.accounts) and delta.created_after == sync.created_after
    # ... and the next commit still answers as the oracle did.
    _, op, ts, batch = sc.steps[-1]
    assert engine.commit(op, ts, b"".join(batch)) == ledger["replies"][-1]
    assert engine.commit_timestamp == ledger["commit_timestamp"]
    assert engine.export_transfers().tobytes() == transfers.tobytes()
    assert engine.export_accounts().tobytes() == ledger["accounts"].tobytes()


def test_on_an_engine_a_device_panic_stopped(gpu_engine_factory):
    """tests/test_gpu_alloc.py's way to a device panic (a post whose checked `-=` traps after the setup
    action zeroed the pending balance).  The stopped engine still answers."""
    engine = gpu_engine_factory()
    accounts = b"".join(pack_account(id=i, ledger=1, code=1) for i in (1, 2))
    assert engine.commit(128, 10, accounts) == b""
    assert engine.commit(129, 20, pack_transfer(id=10, debit_account_id=1, credit_account_id=2, amount=100, ledger=1, code=1,
                                                flags=PENDING)) == b""
    assert engine.commit(129, 25, pack_transfer(id=12, debit_account_id=2, credit_account_id=1, amount=7, ledger=1, code=1)) == b""
    healthy, matched, complete = engine.get_account_statement_series([1, 2], [10, 20, 25])
    assert matched == 4 and complete
    assert [balances(r, "closing") for r in healthy[:2]] == [(100, 0, 0, 0), (100, 0, 0, 7)]
    assert sums(healthy[3]) == ((0, 0, 7, 1), (0, 0, 0, 0))
    engine.set_balances(1, 0, 0, 0, 0)
    with pytest.raises(EnginePanic):
        engine.commit(129, 30, pack_transfer(id=11, pending_id=10, flags=POST))
    with pytest.raises(EnginePanic, match="stopped"):
        engine.commit(129, 40, pack_transfer(id=13, debit_account_id=1, credit_account_id=2, amount=1, ledger=1, code=1))
    checker = Series(engine.export_transfers(), engine.export_accounts())
    allocations = engine.lib.tbgpu_debug_allocations()
    for bounds in ([0, 0], [10, 20, 24], [0, 19, 20, 25, 0], [19, 24, 0]):
        want, matched, _ = checker.of([2, 1, 2], bounds)
        got, got_matched, _ = engine.get_account_statement_series([2, 1, 2], bounds)
        assert got.tobytes() == want.tobytes() and got_matched == matched == 3 * (len(bounds) - 1)
    assert engine.lib.tbgpu_debug_allocations() == allocations


def test_invalid_input(ledger, gpu_engine_factory):
    sc, ids = ledger["sc"], ledger["ids"]
    engine = gpu_engine_factory(transfers_max=1 << 12)
    empty = engine.get_account_statement_series(ids, [0, 5, 9])
    assert len(empty[0]) == 0 and empty[0].dtype == STATEMENT_DTYPE and empty[1:] == (0, True)  # an empty engine
    commit_all(sc, engine, steps=sc.steps[:4])
    t0, t1, t2 = sc.steps[1][2], sc.steps[2][2], sc.steps[3][2]
    bounds = [t0, t1, t2]
    valid, matched, complete = engine.get_account_statement_series(ids, bounds)
    assert matched == len(valid) == 2 * (len(ids) - 4) and complete
    assert any(sums(r) != NOTHING for r in valid)
    # Invalid bounds are answered OK with zeros and write nothing.
    for bad in ([U64_MAX, 0], [0, U64_MAX], [t0, U64_MAX, 0], [U64_MAX, t0, t1], [t0, 0, t1], [0, 0, 0], [t1, t0], [t0, t2, t1],
                [t2, t0, 0], [t0, t1 + 1, t1]):
        got, m, complete = engine.get_account_statement_series(ids, bad)
        assert len(got) == 0 and m == 0 and complete
        status, result, raw = raw_call(engine, bad, ids, len(ids), 2 * len(ids))
        assert status == _lib.STATUS_OK and result == (0, 1, 0) and raw == b"\xAB" * len(raw)
    got, m, complete = engine.get_account_statement_series([], bounds)
    assert len(got) == 0 and m == 0 and complete
    fn = engine.lib.tbgpu_get_account_statement_series
    src = ctypes.create_string_buffer(ids_body(ids), 16 * len(ids))
    edges = (ctypes.c_uint64 * 3)(*bounds)
    rows = 2 * len(ids)
    sentinel = b"\xAB" * (ROW * rows)
    out = ctypes.create_string_buffer(sentinel, len(sentinel))
    res = _lib.tbgpu_query_result(count=77, complete=77, matched=77)
    untouched = lambda: out.raw == sentinel and (res.count, res.complete, res.matched) == (77, 77, 77)
    assert fn(engine.h, edges, 2, src, 0, out, rows, ctypes.byref(res)) == _lib.STATUS_OK and untouched()
    assert fn(engine.h, edges, 2, None, 0, None, 0, None) == _lib.STATUS_OK
    assert fn(engine.h, None, 2, src, len(ids), out, rows, ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, None, 2, None, 0, None, 0, None) == _lib.STATUS_INVALID
    assert fn(engine.h, edges, 0, src, len(ids), out, rows, ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, edges, 2, None, len(ids), out, rows, ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, edges, 2, src, len(ids), None, rows, ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, edges, 2, src, len(ids), out, rows, None) == _lib.STATUS_INVALID and out.raw == sentinel
    assert fn(engine.h, edges, 2, src, 2048, out, rows, ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, edges, 0xFFFFFFFF, src, 0xFFFFFFFF, out, rows, ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, edges, 2, src, len(ids), out, rows, ctypes.byref(res)) == _lib.STATUS_OK
    assert res.count == len(valid) and out.raw[:ROW * len(valid)] == valid.tobytes()
    assert out.raw[ROW * len(valid):] == sentinel[ROW * len(valid):]
