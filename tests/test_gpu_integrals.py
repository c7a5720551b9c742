"""get_account_balance_integrals (include/tbgpu.h tbgpu_get_account_balance_integrals,
csrc/k_integral.h): for the accounts a caller names and a period (t_open, t_end], the balances at its
start and at its end and each balance summed over every nanosecond of the period, modulo 2^192, from one
scan of the HBM log.  Rows, `matched` and `complete` are compared byte for byte with the checker of
tests/harness/integrals.py (itself held to lookup_accounts_at's checker tick by tick in
tests/test_integral_checkers.py), with lookup_accounts_at summed tick by tick on the device and with
get_account_statements at both ends."""
import ctypes
import random

import numpy as np
import pytest

from tests.harness.balances import balances_of, u128
from tests.harness.integrals import MOD192, Integrals, balances, ids_body, integrals
from tests.harness.oracle import OracleEngine
from tests.harness.shard_double import homes_of
from tests.harness.statements import request_of, sweep_pairs
from tests.harness.workload import account_id, make_scenario
from tests.test_gpu_query import SCENARIO, by_id, commit_all, posted_states
from tigerbeetle_amd import _lib
from tigerbeetle_amd._lib import EnginePanic
from tigerbeetle_amd.state_machine import average_balances
from tigerbeetle_amd.types import INTEGRAL_DTYPE, U64_MAX, TransferFlags, pack_account, pack_transfer

pytestmark = pytest.mark.gpu

PENDING = int(TransferFlags.pending)
POST = int(TransferFlags.post_pending_transfer)
VOID = int(TransferFlags.void_pending_transfer)
MAX = 4095
ROW = 256
ABSENT = (account_id(5000), account_id(5001))
ENDS = [when + "_" + c + w for when in ("opening", "closing")
        for c in ("debits_pending", "debits_posted", "credits_pending", "credits_posted") for w in ("_lo", "_hi")]


def check(engine, checker, ids, t_open, t_close, evicted=False, cap=None):
    """One request: rows, matched and complete as the checker has them."""
    want, matched, orphan = checker.of(ids, t_open, t_close, cap)
    got, got_matched, got_complete = engine.get_account_balance_integrals(ids, t_open, t_close, cap)
    assert len(got) == len(want), (t_open, t_close, len(got), len(want))
    if got.tobytes() != want.tobytes():
        bad = next(k for k in range(len(got)) if got[k].tobytes() != want[k].tobytes())
        assert False, (t_open, t_close, bad, got[bad], want[bad])
    assert (got_matched, got_complete) == (matched, not evicted and not orphan), (t_open, t_close)
    return got


def raw_call(engine, t_open, t_close, ids, n, cap, fill=b"\xAB"):
    """The C call into a sentinel-filled buffer: (status, result, the buffer's bytes)."""
    src = ctypes.create_string_buffer(ids_body(ids), 16 * len(ids))
    out = ctypes.create_string_buffer(fill * (ROW * max(len(ids), 1)), ROW * max(len(ids), 1))
    res = _lib.tbgpu_query_result(count=77, complete=77, matched=77)
    status = engine.lib.tbgpu_get_account_balance_integrals(engine.h, t_open, t_close, src, n, out, cap, ctypes.byref(res))
    return status, (res.count, res.complete, res.matched), out.raw


def same_ends_as_statements(engine, rows, ids, t_open, t_end):
    """opening and closing, byte for byte get_account_statements' for the same period."""
    held = engine.get_account_statements(ids, t_open, t_end)[0]
    assert len(held) == len(rows)
    for f in ("id_lo", "id_hi") + tuple(ENDS):
        assert rows[f].tobytes() == held[f].tobytes(), (f, t_open, t_end)


def additive(engine, ids, t0, t1, t2):
    """I(t0, t2) = I(t0, t1) + I(t1, t2) modulo 2^192, on the engine's own answers."""
    whole, first, second = (engine.get_account_balance_integrals(ids, a, b)[0] for a, b in ((t0, t2), (t0, t1), (t1, t2)))
    earlier = {u128(r, "id"): integrals(r) for r in first}  # (an account created after t1 has no first part: zero)
    assert len(whole) == len(second) > 0
    for w, s in zip(whole, second):
        parts = tuple((a + b) % MOD192 for a, b in zip(earlier.get(u128(w, "id"), (0, 0, 0, 0)), integrals(s)))
        assert parts == integrals(w), (t0, t1, t2, hex(u128(w, "id")))


@pytest.fixture(scope="module")
def ledger():
    """test_gpu_query.py's scenario, the oracle that committed all of it, its exports and the checker
    over them (never changed)."""
    sc = make_scenario(2025, **SCENARIO)
    oracle = OracleEngine(4096, 1 << 15)
    replies = commit_all(sc, oracle)
    transfers, accounts = oracle.export_transfers(), oracle.export_accounts()
    return dict(sc=sc, replies=replies, transfers=transfers, accounts=accounts, commit_timestamp=oracle.commit_timestamp,
                posted=oracle.export_posted(), checker=Integrals(transfers, accounts, oracle.commit_timestamp),
                ids=request_of(accounts, ABSENT), pairs=sweep_pairs(sc.steps, transfers, oracle.commit_timestamp))


def test_single_engine_sweep(ledger, gpu_engine_factory):
    sc, checker, ids = ledger["sc"], ledger["checker"], ledger["ids"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    assert commit_all(sc, engine) == ledger["replies"]
    now = ledger["commit_timestamp"]
    assert engine.commit_timestamp == now
    answers = {pair: check(engine, checker, ids, *pair) for pair in ledger["pairs"]}
    assert len({rows.tobytes() for rows in answers.values()}) > 20
    empty = [pair for pair in answers if pair[0] == pair[1] != 0 and len(answers[pair])]
    assert empty and all(integrals(r) == (0, 0, 0, 0) and balances(r, "opening") == balances(r, "closing") and average_balances(r) is None
                         for pair in empty for r in answers[pair])
    whole = answers[(0, 0)]
    assert len(whole) == len(ids) - 4 and all(balances(r, "opening") == (0, 0, 0, 0) and int(r["t_end"]) == now for r in whole)
    assert any(w >> 64 for r in whole for w in integrals(r))
    assert len(answers[(0, 1)]) == 0 and 0 < len(answers[(0, sc.steps[0][2])]) < len(whole)
    # t_close == 0 is t_close == commit_timestamp; an end below the start has no rows.
    assert len(answers[(now + 1, 0)]) == 0
    for t_open in (0, 1, sc.steps[5][2], now):
        assert engine.get_account_balance_integrals(ids, t_open, 0)[0].tobytes() == check(engine, checker, ids, t_open, now).tobytes()
    # An average lies between the least and the greatest balance of a column that only grows.
    row = answers[(sc.steps[5][2], sc.steps[12][2])][0]
    assert balances(row, "opening")[1] <= average_balances(row)[1] <= balances(row, "closing")[1]
    # out_cap_rows cuts the answer in request order, and nothing past count rows is written.
    pair = ledger["pairs"][len(ledger["pairs"]) // 2]
    matched = len(answers[pair])
    assert matched > 8
    for cap in (0, 1, matched - 1, matched, matched + 3):
        check(engine, checker, ids, *pair, cap=cap)
        status, (count, complete, m), raw = raw_call(engine, pair[0], pair[1], ids, len(ids), cap)
        assert status == _lib.STATUS_OK and (count, complete, m) == (min(cap, matched), 1, matched)
        assert raw[:ROW * count] == answers[pair][:count].tobytes() and raw[ROW * count:] == b"\xAB" * (ROW * (len(ids) - count))


def test_against_the_engines_own_calls(ledger, gpu_engine_factory):
    """opening and closing are get_account_statements' bytes for the same period, and the integrals add
    over three split points."""
    sc, ids = ledger["sc"], ledger["ids"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, engine)
    b = [ts for _, _, ts, _ in sc.steps]
    stamps = np.sort(ledger["transfers"]["timestamp"])
    for t_open, t_end in ((b[2], b[9]), (int(stamps[300]), int(stamps[1500])), (b[5], ledger["commit_timestamp"]), (int(stamps[40]), b[-1]),
                          (0, b[4]), (b[7], b[7])):
        rows, matched, complete = engine.get_account_balance_integrals(ids, t_open, t_end)
        assert complete and matched == len(rows) > 0
        same_ends_as_statements(engine, rows, ids, t_open, t_end)
    t0, t2 = int(stamps[100]), int(stamps[1800])
    for t1 in (t0 + 1, int(stamps[900]), b[10], t2 - 1):
        additive(engine, ids, t0, t1, t2)
    additive(engine, ids, 0, b[3], ledger["commit_timestamp"])


def test_tile_wave_and_workgroup_edges(gpu_engine_factory):
    """Two prepares of 4,200 events committed in place (tbgpu_log_window), so log position = event
    index and timestamp = first + position.  Account A's records sit around the scan's wave edge
    (63/64), tile edge (511/512) and workgroup edge (8191/8192), and in every lane of the wave at
    1024-1087; with a pending transfer and its partial post, another and its void, failing events that
    name A, and amounts whose sums carry across the 64-bit word.  t_open and t_end at, one below and
    one above those records put both zone borders on every edge and inside the wave that holds only A;
    further periods end 2^40 past the last record, so that an amount of 2^100 times its weight carries
    across both word borders of a 192-bit sum.  The first call follows tbgpu_commit_device_async
    without a sync."""
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
    last = at(2 * half - 1)
    assert len(exported) == 2 * half - 2 and int(exported["timestamp"].max()) == last == oracle.commit_timestamp
    checker = Integrals(exported, oracle.export_accounts(), last)
    window = engine.log_window(2 * half)
    engine.to_device(window, np.frombuffer(bodies[0] + bodies[1], dtype=np.uint8))
    res, rb = engine.alloc(2 * half * 8), engine.alloc(8)
    engine.commit_device_async(129, stamps, [half, half], window, res, rb)
    # The query drains the pending call itself.
    ids = [account_id(i) for i in range(n_acc)] + [A, account_id(3)]
    far = last + (1 << 40)
    edges = [61, 62, 63, 64, 65, 66, 510, 511, 512, 513, 514, 1023, 1024, 1050, 1087, 1088, 4199, 4200, 8189, 8190, 8191, 8192, 8193,
             8194, 8399]
    pairs = [(at(a), at(b)) for a, b in zip(edges, edges[1:])] + [(at(a), at(b)) for a, b in zip(edges, edges[2:])]
    pairs += [(0, at(e)) for e in (63, 64, 511, 512, 8191, 8192)]
    pairs += [(at(e), 0) for e in (63, 64, 511, 512, 8191, 8192)] + [(at(1030), at(1060)), (at(100), at(8300)), (0, 0)]
    pairs += [(at(e), far) for e in (0, 61, 63, 64, 511, 512, 1050, 8191, 8192, 8399)] + [(last + 5, far), (0, far)]
    seen, in_both = set(), 0
    for t_open, t_close in pairs:
        got = check(engine, checker, ids, t_open, t_close)
        assert got[0].tobytes() == got[n_acc].tobytes()
        seen.add(got[0].tobytes())
        in_both += at(1024) <= t_open < t_close < at(1087)  # the wave of A alone holds both zones and records below t_open
    assert len(set(pairs)) == len(pairs) and len(seen) > len(pairs) // 2 and in_both >= 2
    # Non-vacuity.  A far end: every column's integral of A has a third word, and so has the weighted
    # part alone (the sums, not just opening * L, carried across both word borders).
    a_row = check(engine, checker, [A], at(100), far)[0]
    length = far - at(100)
    weighted = [(total - opening * length) % MOD192 for total, opening in zip(integrals(a_row), balances(a_row, "opening"))]
    assert all(v >> 128 for v in integrals(a_row)) and weighted[1] >> 128 and weighted[3] >> 128
    assert weighted[1] < 1 << 191 and weighted[3] < 1 << 191  # the posted columns only grow
    # A released hold in the period and none placed: the pending column's weighted part is negative —
    # it wraps modulo 2^192 — and the integral itself is the true, smaller, sum.
    for t_open, t_end, column, held in ((at(513), at(1023), 0, 1 << 100), (at(8188), at(8190), 2, 1 << 64)):
        row = check(engine, checker, [A], t_open, t_end)[0]
        opening, closing, length = balances(row, "opening")[column], balances(row, "closing")[column], t_end - t_open
        assert opening - closing == held
        part = (integrals(row)[column] - opening * length) % MOD192
        assert part >> 191 and MOD192 - part == held * (length - 1)  # released one tick into the period
        assert integrals(row)[column] == opening + closing * (length - 1)
    # From first principles on the device: the integral is lookup_accounts_at summed over every t.
    for t_open, t_end in ((at(1020), at(1090)), (at(1040), at(1041)), (at(1023), at(1088))):
        rows = check(engine, checker, [A, account_id(3)], t_open, t_end)
        total = {u128(r, "id"): [0, 0, 0, 0] for r in rows}
        for t in range(t_open, t_end):
            for rec in engine.lookup_accounts_at([A, account_id(3)], t)[0]:
                for c, v in enumerate(balances_of(rec)):
                    total[u128(rec, "id")][c] += v
        assert t_end - t_open <= 70 and all(integrals(r) == tuple(total[u128(r, "id")]) for r in rows)
        assert all(any(integrals(r)) for r in rows)
    # Against the engine's own calls: the statements' ends, and additivity over three split points.
    for t_open, t_end in ((at(63), at(8192)), (at(511), far), (0, at(512))):
        same_ends_as_statements(engine, check(engine, checker, ids, t_open, t_end), ids, t_open, t_end)
    for t1 in (at(64), at(1050), at(8192)):
        additive(engine, ids, at(10), t1, far)
    assert engine.get_account_balance_integrals(ids, at(511), 0)[0].tobytes() == check(engine, checker, ids, at(511), last).tobytes()
    assert engine.export_accounts().tobytes() == oracle.export_accounts().tobytes()
    assert engine.export_transfers().tobytes() == exported.tobytes()
    engine.free(res)
    engine.free(rb)


def test_more_active_accounts_than_lds_bins(gpu_engine_factory):
    """4,200 accounts; two 4,000-transfer prepares in which 600 accounts debit again and again, more
    than a workgroup's claimed LDS bins, all inside one workgroup's 8,192 records: bins are claimed,
    handed over at the workgroup's end and, once both of an index's slots are taken, bypassed for HBM.
    Amounts of 2^63 + j: two of them carry out of the low word.  A request of exactly 4,095 ids; one
    more is invalid and writes nothing."""
    n_acc, hot = 4200, 600
    engine = gpu_engine_factory(accounts_max=1 << 13, transfers_max=1 << 14)
    body = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(n_acc))
    assert engine.commit(128, 10**12, body) == b""
    for k in range(2):
        body = b"".join(pack_transfer(id=10**6 + 4000 * k + j, debit_account_id=account_id((7 * j) % hot),
                                      credit_account_id=account_id(hot + (j * 13 + k) % (n_acc - hot)), amount=(1 << 63) + j, ledger=1,
                                      code=1, flags=PENDING if (j // hot) % 3 == 0 else 0) for j in range(4000))
        assert engine.commit(129, 2 * 10**12 + k * 10**6, body) == b""
    transfers = engine.export_transfers()
    assert len(transfers) == 8000
    checker = Integrals(transfers, engine.export_accounts(), engine.commit_timestamp)
    stamps = np.sort(transfers["timestamp"])
    inside_first, inside_second = int(stamps[1700]), int(stamps[6100])
    hot_ids = [account_id(i) for i in range(hot - 1, -1, -1)]
    exact = [account_id(i) for i in range(MAX)]
    rng = random.Random(9)
    rng.shuffle(exact)
    for ids in (hot_ids, exact):
        for t_open, t_close in ((0, 0), (10**12, inside_first), (inside_first, inside_second), (inside_second, 0)):
            got = check(engine, checker, ids, t_open, t_close)
            assert len(got) == len(ids)
        got = check(engine, checker, ids, inside_first, inside_second)
        active = got[got["closing_debits_posted_lo"] != got["opening_debits_posted_lo"]]
        assert len(active) == hot
        assert (active["integral_debits_posted_w1"] > 0).all() and (active["closing_debits_posted_hi"] > 0).all()
    assert len(exact) == MAX
    status, result, raw = raw_call(engine, 0, 0, exact + [account_id(MAX)], MAX + 1, 8)
    assert status == _lib.STATUS_INVALID and result == (77, 77, 77) and raw == b"\xAB" * len(raw)


def test_eviction_and_orphaned_posts(ledger, gpu_engine_factory):
    """After tbgpu_evict_transfers of an old prefix `complete` is 0 and the rows are the checker's over
    the resident export, an orphan post among them (P = its own amount).  And posts whose pending
    transfers were never loaded, with nothing evicted: only a period or a tail that holds one drops
    `complete`."""
    transfers, accounts, ids = ledger["transfers"], ledger["accounts"], ledger["ids"]
    evicted = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(ledger["sc"], evicted)
    evicted.checkpoint_delta()
    assert evicted.evict_transfers(700) > 0
    resident = evicted.export_transfers()
    checker = Integrals(resident, evicted.export_accounts(), evicted.commit_timestamp)
    stamps = np.sort(resident["timestamp"])
    assert checker.of(ids, int(stamps[0]), 0)[2]  # an orphan post is resident
    third, half = int(stamps[len(stamps) // 3]), int(stamps[len(stamps) // 2])
    assert len(stamps) > 100
    for t_open, t_close in ((0, 0), (int(stamps[0]) - 1, third), (int(stamps[0]), int(stamps[-1])), (half, 0), (third, half),
                            (1, int(stamps[0]) - 1)):
        got = check(evicted, checker, ids, t_open, t_close, evicted=True)
        if t_open >= int(stamps[0]) - 1 and not checker.of(ids, t_open, t_close)[2]:  # the ledger's own past
            assert got.tobytes() == ledger["checker"].of(ids, t_open, t_close)[0].tobytes()
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
    checker = Integrals(engine.export_transfers(), engine.export_accounts(), ledger["commit_timestamp"])
    first_orphan = min(int(p["timestamp"]) for p in posts[len(posts) // 2:])
    newest_orphan = max(int(p["timestamp"]) for p in posts[len(posts) // 2:])
    incomplete = 0
    for t_open, t_close in ((first_orphan - 1, first_orphan), (first_orphan, newest_orphan - 1), (newest_orphan - 1, newest_orphan),
                            (newest_orphan, 0), (1, first_orphan - 1), (0, 0)):
        check(engine, checker, ids, t_open, t_close)
        incomplete += checker.of(ids, t_open, t_close)[2]
    assert 3 <= incomplete < 6
    post = posts[-1]
    ts = int(post["timestamp"])
    row = check(engine, checker, [u128(post, "debit_account_id")], ts - 1, ts)[0]
    assert balances(row, "opening")[0] - balances(row, "closing")[0] == u128(post, "amount")  # P is the post's own amount


CHAIN_FREE = dict(n_accounts=8, n_transfer_batches=4, batch_len=(100, 200), p_linked=0, p_limit=0, p_balancing=0,
                  p_pending=0.3, p_post_void=0.25)


def test_anchor_setup_action(gpu_engine_factory):
    """tbgpu_test_set_balances between two runs of commits: the answers are anchored at the engine's
    current balances, and a period after the setup is the oracle's own past."""
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
    checker = Integrals(engine.export_transfers(), engine.export_accounts(), engine.commit_timestamp)
    assert engine.export_accounts().tobytes() == oracle.export_accounts().tobytes()
    for lo, hi in zip(sc.steps, sc.steps[1:]):
        check(engine, checker, ids, lo[2], hi[2])
        check(engine, checker, ids, lo[2] - 3, hi[2] - 3)
    t_open, t_end = sc.steps[half - 1][2], sc.steps[half][2]
    rows = check(engine, checker, ids, t_open, t_end)
    assert all(balances(r, "opening") == at_setup[u128(r, "id")] and balances(r, "closing") == after_one[u128(r, "id")] for r in rows)
    assert at_setup != after_one
    # Up to now, with a third word: 2^100 held for more than 2^28 ns.
    assert engine.commit_timestamp - t_open > 1 << 28 and all(integrals(r)[0] >> 128 for r in check(engine, checker, ids, t_open, 0))
    check(engine, checker, ids, 0, 0)


def test_restart_and_unordered_log(gpu_engine_factory):
    """The accounts loaded (tbgpu_load_accounts), the newer half committed, then the older half loaded
    shuffled (tbgpu_load_transfers): older timestamps sit behind newer ones in the log, records of all
    three kinds (below t_open, in the period, above t_end) share tiles, and the answers still equal
    the checker anchored at the engine's current balances."""
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
    # Restarted from the balances alone, an empty log: the loaded balances held for the whole period.
    loaded = Integrals(engine2.export_transfers(), engine2.export_accounts(), last)
    rows = check(engine2, loaded, ids, 5, 0)
    assert len(rows) == len(ids) - 4
    assert all(balances(r, "opening") == balances(r, "closing") == at_restart[u128(r, "id")] == average_balances(r) for r in rows)
    commit_all(sb, oracle, engine2, steps=b_steps)
    order = np.random.default_rng(5).permutation(len(half_a))
    engine2.load_transfers(half_a[order], states[order])
    transfers = oracle.export_transfers()
    assert engine2.export_transfers().tobytes() == transfers.tobytes()
    assert len(half_a) > 500 and len(transfers) - len(half_a) > 500
    checker = Integrals(engine2.export_transfers(), engine2.export_accounts(), engine2.commit_timestamp)
    stamps = np.sort(transfers["timestamp"])
    created = sorted(int(a["timestamp"]) for a in oracle.export_accounts())
    marks = [0, created[0] - 1, created[0], created[-1], int(stamps[0]), int(stamps[len(half_a) // 2]), int(half_a["timestamp"].max()),
             last, last + 1, int(stamps[len(half_a) + 50]), int(stamps[-1]), 0]
    lengths = set()
    for t_open, t_close in list(zip(marks, marks[1:])) + [(int(stamps[200]), int(stamps[-200])), (created[0], int(stamps[len(half_a) + 50]))]:
        lengths.add(len(check(engine2, checker, ids, t_open, t_close)))
    assert 0 in lengths and len(lengths) >= 3  # accounts loaded with a timestamp above t_end are skipped
    # A period that ends at the restart point closes on what the oracle's accounts were then.
    rows = check(engine2, checker, ids, int(stamps[100]), last)
    assert all(balances(r, "closing") == at_restart[u128(r, "id")] for r in rows)


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
    assert engine.commit_timestamp == ledger["commit_timestamp"]
    for pair in ledger["pairs"]:
        got = check(engine, checker, ids, *pair)
        assert got.tobytes() == single.get_account_balance_integrals(ids, *pair)[0].tobytes()
    # A far end: sums beyond one word.  A shard that holds a post but not its pending transfer has a
    # negative partial sum — all ones in its upper words — so the host's add carries across both borders.
    far = ledger["commit_timestamp"] + (1 << 62)
    got = check(engine, checker, ids, sc.steps[3][2], far)
    assert all(any(w >> 64 for w in integrals(r)) for r in got)
    pair = ledger["pairs"][len(ledger["pairs"]) // 2]
    for cap in (0, 3, len(ids)):
        check(engine, checker, ids, *pair, cap=cap)
    status, result, raw = raw_call(engine, pair[0], pair[1], ids, len(ids), 3)
    assert status == _lib.STATUS_OK and result[0] == 3 and raw[3 * ROW:] == b"\xAB" * (len(raw) - 3 * ROW)


def test_read_only_and_allocation_free(ledger, gpu_engine_factory):
    """50 calls around which the allocation count, commit_timestamp, the exports and the commit-path
    counters of tbgpu_get_stats stand still; one more inside an asynchronous write-back; then the
    next commit answers as the oracle did."""
    sc, transfers, ids = ledger["sc"], ledger["transfers"], ledger["ids"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    twin = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, engine, twin, steps=sc.steps[:-1])
    resident = engine.export_transfers()
    checker = Integrals(resident, engine.export_accounts(), engine.commit_timestamp)
    before = (engine.commit_timestamp, engine.export_accounts().tobytes(), resident.tobytes(), engine.export_posted().tobytes())
    rng = random.Random(3)
    allocations = engine.lib.tbgpu_debug_allocations()
    stats = engine.stats()
    stamps = np.sort(resident["timestamp"])
    marks = (0, 1, int(stamps[len(stamps) // 3]), int(stamps[-5]), int(stamps[-1]) + 7)
    for _ in range(50):
        t_open = rng.choice(marks)
        t_close = rng.choice([0] + [m for m in marks if m >= t_open])
        engine.get_account_balance_integrals(rng.sample(ids, rng.choice((1, 5, len(ids)))), t_open, t_close)
    assert engine.lib.tbgpu_debug_allocations() == allocations
    after = engine.stats()
    assert all(after[k] == stats[k] for k in ("passes", "events", "transfers", "accounts", "log_used"))
    assert before == (engine.commit_timestamp, engine.export_accounts().tobytes(), engine.export_transfers().tobytes(),
                      engine.export_posted().tobytes())
    # One between an asynchronous write-back's start and its wait leaves the delta alone.
    caps = (1 << 14, 1 << 14, 1 << 14)
    engine.checkpoint_delta_async(caps)
    allocations = engine.lib.tbgpu_debug_allocations()
    check(engine, checker, ids, int(stamps[len(stamps) // 3]), int(stamps[-5]))
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
    action zeroed the pending balance).  The stopped engine still answers.  The panic left the post in
    the log and its accounts' balances short of it, so before the post the definition walks through
    balances below zero: there the header's order-free form is the specification (a balance below zero
    counts as that negative number); from the post on the rows are the checker's byte for byte."""
    engine = gpu_engine_factory()
    accounts = b"".join(pack_account(id=i, ledger=1, code=1) for i in (1, 2))
    assert engine.commit(128, 10, accounts) == b""
    assert engine.commit(129, 20, pack_transfer(id=10, debit_account_id=1, credit_account_id=2, amount=100, ledger=1, code=1,
                                                flags=PENDING)) == b""
    assert engine.commit(129, 25, pack_transfer(id=12, debit_account_id=2, credit_account_id=1, amount=7, ledger=1, code=1)) == b""
    healthy, matched, complete = engine.get_account_balance_integrals([1, 2], 18, 27)
    assert matched == 2 and complete
    assert balances(healthy[0], "opening") == (0, 0, 0, 0) and balances(healthy[0], "closing") == (100, 0, 0, 7)
    assert integrals(healthy[0]) == (700, 0, 0, 14) and integrals(healthy[1]) == (0, 14, 700, 0)
    assert average_balances(healthy[0]) == (77, 0, 0, 1)
    engine.set_balances(1, 0, 0, 0, 0)
    with pytest.raises(EnginePanic):
        engine.commit(129, 30, pack_transfer(id=11, pending_id=10, flags=POST))
    with pytest.raises(EnginePanic, match="stopped"):
        engine.commit(129, 40, pack_transfer(id=13, debit_account_id=1, credit_account_id=2, amount=1, ledger=1, code=1))
    checker = Integrals(engine.export_transfers(), engine.export_accounts(), engine.commit_timestamp)
    last = int(engine.export_transfers()["timestamp"].max())
    allocations = engine.lib.tbgpu_debug_allocations()
    for t_open, t_close in ((engine.commit_timestamp, 0), (last, last + 1), (last + 3, 1000), (last, 1 << 63)):
        want, matched, _ = checker.of([2, 1, 2], t_open, t_close)
        got, got_matched, _ = engine.get_account_balance_integrals([2, 1, 2], t_open, t_close)
        assert got.tobytes() == want.tobytes() and got_matched == matched == 3
    for t_open, t_end in ((0, 1000), (10, 20), (20, 24), (19, 25), (24, 31)):
        got, got_matched, _ = engine.get_account_balance_integrals([2, 1, 2], t_open, t_end)
        assert got_matched == len(got) == 3 and got[0].tobytes() == got[2].tobytes()
        for row in got:
            i = u128(row, "id")
            assert balances(row, "opening") == checker.balance_at(i, t_open) and balances(row, "closing") == checker.balance_at(i, t_end)
            assert integrals(row) == checker.order_free(i, t_open, t_end), (t_open, t_end, i)
    assert engine.lib.tbgpu_debug_allocations() == allocations


def test_invalid_input(ledger, gpu_engine_factory):
    sc, ids = ledger["sc"], ledger["ids"]
    engine = gpu_engine_factory(transfers_max=1 << 12)
    for t_close in (0, 5):  # an empty engine: commit_timestamp is 0, nothing existed at 5
        empty = engine.get_account_balance_integrals(ids, 0, t_close)
        assert len(empty[0]) == 0 and empty[0].dtype == INTEGRAL_DTYPE and empty[1:] == (0, True)
    commit_all(sc, engine, steps=sc.steps[:4])
    now = engine.commit_timestamp
    t_open, t_close = sc.steps[1][2], sc.steps[3][2]
    valid, matched, complete = engine.get_account_balance_integrals(ids, t_open, t_close)
    assert matched == len(valid) == len(ids) - 4 and complete
    assert any(any(integrals(r)) for r in valid)
    # Invalid periods are answered OK with zeros and write nothing: an end at 2^64-1, t_end below
    # t_open, and t_close == 0 with commit_timestamp below t_open.
    for o, c in ((U64_MAX, 0), (0, U64_MAX), (U64_MAX, U64_MAX), (t_close, t_open), (t_close + 1, t_close), (now + 1, 0)):
        got, m, complete = engine.get_account_balance_integrals(ids, o, c)
        assert len(got) == 0 and m == 0 and complete
        status, result, raw = raw_call(engine, o, c, ids, len(ids), len(ids))
        assert status == _lib.STATUS_OK and result == (0, 1, 0) and raw == b"\xAB" * len(raw)
    assert len(engine.get_account_balance_integrals(ids, now, 0)[0]) == len(valid)  # L == 0 is a period
    got, m, complete = engine.get_account_balance_integrals([], t_open, t_close)
    assert len(got) == 0 and m == 0 and complete
    fn = engine.lib.tbgpu_get_account_balance_integrals
    src = ctypes.create_string_buffer(ids_body(ids), 16 * len(ids))
    sentinel = b"\xAB" * (ROW * len(ids))
    out = ctypes.create_string_buffer(sentinel, len(sentinel))
    res = _lib.tbgpu_query_result(count=77, complete=77, matched=77)
    untouched = lambda: out.raw == sentinel and (res.count, res.complete, res.matched) == (77, 77, 77)
    assert fn(engine.h, t_open, t_close, src, 0, out, len(ids), ctypes.byref(res)) == _lib.STATUS_OK and untouched()
    assert fn(engine.h, t_open, t_close, None, 0, None, 0, None) == _lib.STATUS_OK
    assert fn(engine.h, t_open, t_close, None, len(ids), out, len(ids), ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, t_open, t_close, src, len(ids), None, len(ids), ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, t_open, t_close, src, len(ids), out, len(ids), None) == _lib.STATUS_INVALID and out.raw == sentinel
    assert fn(engine.h, t_open, t_close, src, MAX + 1, out, len(ids), ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, t_open, t_close, src, len(ids), out, len(ids), ctypes.byref(res)) == _lib.STATUS_OK
    assert res.count == len(valid) and out.raw[:ROW * len(valid)] == valid.tobytes()
    assert out.raw[ROW * len(valid):] == sentinel[ROW * len(valid):]
