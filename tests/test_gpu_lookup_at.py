"""lookup_accounts_at (include/tbgpu.h tbgpu_lookup_accounts_at, csrc/k_asof.h): the accounts a caller
names as they stood at a timestamp it names, derived from the current balances and the HBM log in one
scan.  Records, `matched` and `complete` are compared byte for byte with the checker of
tests/harness/asof.py (itself held to the oracle in tests/test_asof_checkers.py), with lookup_accounts,
and with the account blocks and balance rows get_change_events and get_account_balances return."""
import ctypes
import random

import numpy as np
import pytest

from tests.harness.asof import AsOf, ids_body
from tests.harness.balances import COLUMNS, balances_of, u128
from tests.harness.oracle import OracleEngine
from tests.harness.workload import account_id, make_scenario
from tests.test_gpu_query import SCENARIO, by_id, commit_all, posted_states
from tigerbeetle_amd import _lib
from tigerbeetle_amd._lib import EnginePanic
from tigerbeetle_amd.types import CHANGE_EVENTS_MAX, U64_MAX, TransferFlags, pack_account, pack_transfer

pytestmark = pytest.mark.gpu

PENDING = int(TransferFlags.pending)
POST = int(TransferFlags.post_pending_transfer)
VOID = int(TransferFlags.void_pending_transfer)
U128_MAX = (1 << 128) - 1
AT_MAX = 8191


def check(engine, checker, ids, T, evicted=False, cap=None):
    """One request: records, matched and complete as the checker has them."""
    want, matched, orphan = checker.at(ids, T, cap)
    got, got_matched, got_complete = engine.lookup_accounts_at(ids, T, cap)
    assert len(got) == len(want), (T, len(got), len(want))
    assert got.tobytes() == want.tobytes(), T
    assert (got_matched, got_complete) == (matched, not evicted and not orphan), T
    return got


def request_of(accounts):
    """Every account, absent ids, the reserved ids and repeats."""
    ids = [u128(a, "id") for a in accounts]
    return ids[::-1] + [account_id(5000), 0, U128_MAX] + ids[:5] + [account_id(5001)] + ids[3:4]


def sweep_timestamps(sc, transfers, commit_timestamp):
    stamps = np.sort(transfers["timestamp"])
    boundaries = [ts for _, _, ts, _ in sc.steps]  # the two account prepares' among them
    inside = [int(t) for t in stamps[::37] if int(t) not in boundaries]
    assert len(inside) > 20
    return boundaries + inside + [0, commit_timestamp, commit_timestamp + 1, 1]


@pytest.fixture(scope="module")
def ledger():
    """test_gpu_query.py's scenario, the oracle that committed all of it, its exports and the checker
    over them (never changed)."""
    sc = make_scenario(2025, **SCENARIO)
    oracle = OracleEngine(4096, 1 << 15)
    replies = commit_all(sc, oracle)
    transfers, accounts = oracle.export_transfers(), oracle.export_accounts()
    return dict(sc=sc, replies=replies, transfers=transfers, accounts=accounts, commit_timestamp=oracle.commit_timestamp,
                posted=oracle.export_posted(), checker=AsOf(transfers, accounts), ids=request_of(accounts),
                stamps=sweep_timestamps(sc, transfers, oracle.commit_timestamp))


def test_single_engine_sweep(ledger, gpu_engine_factory):
    sc, checker, ids = ledger["sc"], ledger["checker"], ledger["ids"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    assert commit_all(sc, engine) == ledger["replies"]
    assert engine.commit_timestamp == ledger["commit_timestamp"]
    answers = {T: check(engine, checker, ids, T) for T in ledger["stamps"]}
    # Non-vacuity: the answers move with T, an account prepare's boundary skips the younger accounts,
    # and before everything there is nothing.
    first_accounts, second_accounts = sc.steps[0][2], sc.steps[1][2]
    assert 0 < len(answers[first_accounts]) < len(answers[second_accounts]) == len(ids) - 4
    assert len(answers[1]) == 0
    assert len({a.tobytes() for a in answers.values()}) > len(sc.steps)
    assert answers[ledger["commit_timestamp"]].tobytes() == answers[0].tobytes() == answers[ledger["commit_timestamp"] + 1].tobytes()
    # out_cap_records below matched cuts the answer in request order and writes nothing past it.
    T = sc.steps[len(sc.steps) // 2][2]
    whole = answers[T]
    for cap in (0, 1, 7, len(whole) - 1, len(whole), len(whole) + 3):
        check(engine, checker, ids, T, cap=cap)
    body = ids_body(ids)
    out = ctypes.create_string_buffer(b"\xAB" * (128 * len(ids)), 128 * len(ids))
    res = _lib.tbgpu_query_result()
    src = ctypes.create_string_buffer(body, len(body))
    assert engine.lib.tbgpu_lookup_accounts_at(engine.h, T, src, len(ids), out, 7, ctypes.byref(res)) == _lib.STATUS_OK
    assert (res.count, res.matched, res.complete) == (7, len(whole), 1)
    assert out.raw[:7 * 128] == whole[:7].tobytes() and out.raw[7 * 128:] == b"\xAB" * (128 * (len(ids) - 7))
    # T = 0 is lookup_accounts.
    assert answers[0].tobytes() == engine.commit(130, ledger["commit_timestamp"] + 1, body)


def test_against_change_events_and_account_balances(ledger, gpu_engine_factory):
    """The parent's own calls: an event's two account blocks are its accounts at the event's timestamp,
    and an account's newest balance row at or before T holds its balances at T."""
    sc, transfers = ledger["sc"], ledger["transfers"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, engine)
    after, events = 0, 0
    while True:
        page, _, complete = engine.get_change_events(timestamp_min=after, limit=CHANGE_EVENTS_MAX)
        assert complete
        if len(page) == 0:
            break
        for ev in page:
            T = int(ev["transfer"]["timestamp"])
            pair = [u128(ev["transfer"], "debit_account_id"), u128(ev["transfer"], "credit_account_id")]
            got, matched, complete = engine.lookup_accounts_at(pair, T)
            assert matched == 2 and complete
            assert got[0].tobytes() == ev["debit_account"].tobytes() and got[1].tobytes() == ev["credit_account"].tobytes(), T
        events += len(page)
        after = int(page["transfer"]["timestamp"][-1]) + 1
    assert events == len(transfers) > 1500
    stamps = np.sort(transfers["timestamp"])
    ids = [u128(a, "id") for a in ledger["accounts"]]
    rows_met = 0
    for T in [int(stamps[i]) for i in (0, 5, len(stamps) // 3, len(stamps) // 2, len(stamps) - 2, len(stamps) - 1)]:
        got, _, _ = engine.lookup_accounts_at(ids, T)
        assert len(got) == len(ids)
        for rec in got:
            rows, matched, _ = engine.get_account_balances(u128(rec, "id"), timestamp_max=T, reversed=True, limit=1)
            if matched:
                assert [rec[c + w] for c in COLUMNS for w in ("_lo", "_hi")] == [rows[0][c + w] for c in COLUMNS for w in ("_lo", "_hi")]
                rows_met += 1
            else:
                assert balances_of(rec) == (0, 0, 0, 0)
    assert rows_met > 100


def test_tile_and_wave_boundaries(gpu_engine_factory):
    """One 600-event prepare committed in place (tbgpu_log_window), so log position = event index.
    Account A's transfers sit at the scan's wave and tile boundaries, with a pending transfer and its
    partial post, another and its void, failing events that name A, and amounts whose sums carry
    across the 64-bit word.  T at the positions around every wave and tile edge puts the first record
    newer than T there.  The first call follows tbgpu_commit_device_async without a sync."""
    engine = gpu_engine_factory(transfers_max=1 << 12)
    oracle = OracleEngine(64, 1 << 12)
    n_acc, A = 8, account_id(0)
    accounts = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(n_acc))
    assert engine.commit(128, 10**12, accounts) == oracle.commit(128, 10**12, accounts) == b""
    rng = random.Random(11)
    amounts = [(1 << 64) - 1, 1 << 64, 1 << 100, 1]
    plain = {0: 0, 63: 1, 64: 2, 255: 3, 256: 0, 511: 1, 599: 2}   # position -> amounts index
    batch = []
    for i in range(600):
        dr = 1 + rng.randrange(n_acc - 1)
        cr = 1 + (dr + rng.randrange(n_acc - 2)) % (n_acc - 1)  # another account, never A
        ev = dict(id=1000 + i, debit_account_id=account_id(dr), credit_account_id=account_id(cr), amount=1 + i, ledger=1,
                  code=1)
        other = account_id(1 + i % (n_acc - 1))
        if i in plain and i % 2 == 0:
            ev.update(debit_account_id=A, credit_account_id=other, amount=amounts[plain[i]])
        elif i in plain:
            ev.update(debit_account_id=other, credit_account_id=A, amount=amounts[plain[i]])
        elif i == 10:
            ev.update(debit_account_id=A, credit_account_id=other, amount=1 << 100, flags=PENDING)
        elif i == 300:
            ev.update(debit_account_id=0, credit_account_id=0, amount=(1 << 64) - 1, pending_id=1010, flags=POST)
        elif i == 62:
            ev.update(debit_account_id=other, credit_account_id=A, amount=1 << 64, flags=PENDING)
        elif i == 257:
            ev.update(debit_account_id=0, credit_account_id=0, amount=0, pending_id=1062, flags=VOID)
        elif i == 65:
            ev.update(debit_account_id=A, credit_account_id=other, id=0)
        elif i == 254:
            ev.update(debit_account_id=A, credit_account_id=other, id=1000 + 64)
        batch.append(pack_transfer(**ev))
    body = b"".join(batch)
    ts = 10**12 + 1000
    expected = oracle.commit(129, ts, body)
    assert np.frombuffer(expected, dtype=np.uint32)[0::2].tolist() == [65, 254]  # exactly the planted events failed
    checker = AsOf(oracle.export_transfers(), oracle.export_accounts())
    window = engine.log_window(600)
    engine.to_device(window, np.frombuffer(body, dtype=np.uint8))
    res, rb = engine.alloc(600 * 8), engine.alloc(4)
    engine.commit_device_async(129, [ts], [600], window, res, rb)
    # The query drains the pending call itself.
    first = ts - 600 + 1
    ids = [account_id(i) for i in range(n_acc)] + [A, account_id(3)]
    seen = set()
    for pos in (62, 63, 64, 254, 255, 256, 257, 510, 511, 512, 599, -1):
        got = check(engine, checker, ids, first + pos)
        assert got[0].tobytes() == got[n_acc].tobytes()
        seen.add(balances_of(got[0]))
    assert len(seen) >= 9  # A's balances differ at nearly every edge
    assert max(b[0] for b in seen) >> 64 and max(b[1] for b in seen) >> 64 and max(b[3] for b in seen) >> 64
    assert (0, 0, 0, 0) in seen
    assert engine.export_accounts().tobytes() == oracle.export_accounts().tobytes()
    n_reply = int(engine.to_host(rb, 4).view(np.uint32)[0])
    assert bytes(engine.to_host(res, n_reply)) == expected
    engine.free(res)
    engine.free(rb)


def test_set_at_its_limit(gpu_engine_factory):
    """8,192 accounts and one 4,096-transfer prepare after T that names all of them, two fresh accounts
    per transfer: a request of 8,191 distinct ids fills the set to its limit and every bin takes adds;
    a request with 4,000 repeats resolves each repeated id to one bin."""
    n = 8192
    engine = gpu_engine_factory(accounts_max=1 << 14, transfers_max=1 << 13)
    for half in range(2):
        body = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(half * n // 2, (half + 1) * n // 2))
        assert engine.commit(128, 10**12 * (half + 1), body) == b""
    T = 2 * 10**12
    body = b"".join(pack_transfer(id=10**6 + j, debit_account_id=account_id(2 * j), credit_account_id=account_id(2 * j + 1),
                                  amount=(1 << 64) - 1 - j, ledger=1, code=1, flags=PENDING if j % 3 == 0 else 0)
                    for j in range(n // 2))
    assert engine.commit(129, 3 * 10**12, body) == b""
    checker = AsOf(engine.export_transfers(), engine.export_accounts())
    distinct = [account_id(i) for i in range(AT_MAX)]
    rng = random.Random(5)
    repeats = distinct[:AT_MAX - 4000] + [distinct[rng.randrange(AT_MAX - 4000)] for _ in range(4000)]
    rng.shuffle(repeats)
    for ids in (distinct, repeats):
        assert len(ids) == AT_MAX
        then = check(engine, checker, ids, T)
        now = check(engine, checker, ids, 0)
        assert len(then) == len(now) == AT_MAX
        for c in COLUMNS:
            assert not then[c + "_lo"].any() and not then[c + "_hi"].any()
        moved = now["debits_pending_lo"] | now["debits_posted_lo"] | now["credits_pending_lo"] | now["credits_posted_lo"]
        assert moved.all()
        check(engine, checker, ids, 10**12)  # the second prepare's accounts did not exist yet
    # One id more is invalid, and nothing is written.
    ids = distinct + [account_id(AT_MAX)]
    src = ctypes.create_string_buffer(ids_body(ids), 16 * len(ids))
    out = ctypes.create_string_buffer(b"\xAB" * 1024, 1024)
    res = _lib.tbgpu_query_result(count=77, complete=77, matched=77)
    assert engine.lib.tbgpu_lookup_accounts_at(engine.h, T, src, len(ids), out, 8, ctypes.byref(res)) == _lib.STATUS_INVALID
    assert out.raw == b"\xAB" * 1024 and (res.count, res.complete, res.matched) == (77, 77, 77)


def test_hot_account(gpu_engine_factory):
    """9,000 transfers between two accounts after T, in two prepares, with 100 other ids in the request:
    the two bins take every add, and their sums carry across the 64-bit word."""
    engine = gpu_engine_factory(transfers_max=1 << 14)
    body = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(102))
    assert engine.commit(128, 10**12, body) == b""
    warm = pack_transfer(id=5, debit_account_id=account_id(50), credit_account_id=account_id(0), amount=3, ledger=1, code=1)
    assert engine.commit(129, 10**12 + 10, warm) == b""
    T = 10**12 + 10
    for half in range(2):
        body = b"".join(pack_transfer(id=10**6 + half * 4500 + j, debit_account_id=account_id(j & 1), credit_account_id=account_id(1 - (j & 1)),
                                      amount=(1 << 63) + j, ledger=1, code=1, flags=PENDING if j % 5 == 0 else 0)
                        for j in range(4500))
        assert engine.commit(129, 10**12 + 10**6 * (half + 1), body) == b""
    checker = AsOf(engine.export_transfers(), engine.export_accounts())
    ids = [account_id(i) for i in range(101, -1, -1)]
    then = check(engine, checker, ids, T)
    now = check(engine, checker, ids, 0)
    by = {u128(r, "id"): balances_of(r) for r in then}
    assert by[account_id(0)] == (0, 0, 0, 3) and by[account_id(1)] == (0, 0, 0, 0) and by[account_id(50)] == (0, 3, 0, 0)
    hot = {u128(r, "id"): balances_of(r) for r in now}
    assert all(v >> 64 for v in hot[account_id(0)]) and all(v >> 64 for v in hot[account_id(1)])
    check(engine, checker, ids, 10**12 + 10**6)  # between the two prepares


def test_eviction_of_an_old_prefix(gpu_engine_factory):
    sc = make_scenario(61, n_accounts=16, n_transfer_batches=8, batch_len=(100, 300), p_pending=0, p_post_void=0)
    engine = gpu_engine_factory(transfers_max=1 << 14)
    oracle = OracleEngine(4096, 1 << 14)
    commit_all(sc, oracle, engine)
    whole = AsOf(oracle.export_transfers(), oracle.export_accounts())
    engine.checkpoint_delta()
    assert engine.evict_transfers(500) > 0
    resident = engine.export_transfers()
    checker = AsOf(resident, engine.export_accounts())
    ids = request_of(oracle.export_accounts())
    stamps = np.sort(resident["timestamp"])
    for T in (0, int(stamps[0]) - 1, int(stamps[0]), int(stamps[len(stamps) // 2]), int(stamps[-1]), int(stamps[-1]) + 1):
        got = check(engine, checker, ids, T, evicted=True)
        if T == 0 or T >= int(stamps[0]) - 1:  # every record newer than T is resident: the ledger's own past
            assert got.tobytes() == whole.at(ids, T)[0].tobytes()


def test_orphaned_posts(ledger, gpu_engine_factory):
    """Posts whose pending transfers are not resident, with nothing evicted (the transfers were loaded
    without them) and after an eviction: summed with P = their own amount, and complete is 0 for every
    T below such a post that names a requested account."""
    transfers, accounts, ids = ledger["transfers"], ledger["accounts"], ledger["ids"]
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
    checker = AsOf(engine.export_transfers(), engine.export_accounts())
    first_orphan = min(int(p["timestamp"]) for p in posts[len(posts) // 2:])
    newest_orphan = max(int(p["timestamp"]) for p in posts[len(posts) // 2:])
    incomplete = 0
    for T in (first_orphan - 1, first_orphan, newest_orphan - 1, newest_orphan, 1, 0):
        check(engine, checker, ids, T)
        incomplete += checker.at(ids, T)[2]
    assert 2 <= incomplete < 6
    assert checker.at(ids, first_orphan - 1)[0].tobytes() != ledger["checker"].at(ids, first_orphan - 1)[0].tobytes()
    # ... and after an eviction of the committed ledger.
    evicted = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(ledger["sc"], evicted)
    evicted.checkpoint_delta()
    assert evicted.evict_transfers(700) > 0
    checker = AsOf(evicted.export_transfers(), evicted.export_accounts())
    stamps = np.sort(evicted.export_transfers()["timestamp"])
    assert checker.at(ids, int(stamps[0]))[2]
    for T in (int(stamps[0]) - 1, int(stamps[0]), int(stamps[len(stamps) // 2]), int(stamps[-1])):
        check(evicted, checker, ids, T, evicted=True)


CHAIN_FREE = dict(n_accounts=8, n_transfer_batches=4, batch_len=(100, 200), p_linked=0, p_limit=0, p_balancing=0,
                  p_pending=0.3, p_post_void=0.25)


def test_anchor_setup_action(gpu_engine_factory):
    """tbgpu_test_set_balances between two runs of commits: the answers are anchored at the engine's
    current balances, and every T after the setup is the oracle's own past."""
    sc = make_scenario(17, **CHAIN_FREE)
    half = len(sc.steps) - 2
    big = [(1 << 100) + 5, (1 << 64) + 1, (1 << 90) + 9, (1 << 64) - 1]
    oracle = OracleEngine(64, 1 << 12)
    engine = gpu_engine_factory(transfers_max=1 << 12)
    commit_all(sc, oracle, engine, steps=sc.steps[:half])
    ids = request_of(oracle.export_accounts())
    for i, a in enumerate(oracle.export_accounts()):
        oracle.set_balances(u128(a, "id"), *[b + i for b in big])
        engine.set_balances(u128(a, "id"), *[b + i for b in big])
    at_setup = oracle.commit(130, sc.steps[half - 1][2] + 1, ids_body(ids))
    commit_all(sc, oracle, engine, steps=sc.steps[half:half + 1])
    after_one = oracle.commit(130, sc.steps[half][2] + 1, ids_body(ids))
    commit_all(sc, oracle, engine, steps=sc.steps[half + 1:])
    checker = AsOf(engine.export_transfers(), engine.export_accounts())
    assert engine.export_accounts().tobytes() == oracle.export_accounts().tobytes()
    for step in sc.steps:
        check(engine, checker, ids, step[2])
        check(engine, checker, ids, step[2] - 3)
    assert check(engine, checker, ids, sc.steps[half - 1][2]).tobytes() == at_setup
    assert check(engine, checker, ids, sc.steps[half][2]).tobytes() == after_one
    assert at_setup != after_one


def test_restart_and_unordered_log(gpu_engine_factory):
    """test_gpu_balances.py's unordered log through a restart: the accounts loaded
    (tbgpu_load_accounts), the newer half committed, then the older half loaded shuffled
    (tbgpu_load_transfers) — records newer than T sit at lower log positions than older ones, and the
    answers still equal the checker anchored at the engine's current balances.  An account loaded
    with a timestamp above T is skipped."""
    kw = dict(n_accounts=8, n_transfer_batches=40, batch_len=(100, 400), p_pending=0.3, p_dup=0.05, p_linked=0.05,
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
    at_restart = oracle.export_accounts()
    engine2.load_accounts(engine1.export_accounts())
    engine2.set_commit_timestamp(last)
    ids = request_of(at_restart)
    # Restarted from the balances alone, an empty log: every T answers the loaded balances.
    loaded = AsOf(engine2.export_transfers(), engine2.export_accounts())
    assert check(engine2, loaded, ids, last).tobytes() == check(engine2, loaded, ids, 0).tobytes()
    commit_all(sb, oracle, engine2, steps=b_steps)
    order = np.random.default_rng(5).permutation(len(half_a))
    engine2.load_transfers(half_a[order], states[order])
    transfers = oracle.export_transfers()
    assert engine2.export_transfers().tobytes() == transfers.tobytes()
    assert len(half_a) > 1000 and len(transfers) - len(half_a) > 1000
    assert engine2.export_accounts().tobytes() == oracle.export_accounts().tobytes()
    checker = AsOf(engine2.export_transfers(), engine2.export_accounts())
    stamps = np.sort(transfers["timestamp"])
    created = sorted(int(a["timestamp"]) for a in at_restart)
    lengths = set()
    for T in [created[0] - 1, created[0], created[len(created) // 2], created[-1], int(stamps[0]), int(stamps[len(half_a) // 2]),
              int(half_a["timestamp"].max()), last, last + 1, int(stamps[len(half_a) + 50]), int(stamps[-1])] + [int(t) for t in stamps[::501]]:
        lengths.add(len(check(engine2, checker, ids, T)))
    assert 0 in lengths and len(lengths) >= 3  # accounts loaded with a timestamp above T are skipped
    # At the restart point the ledger's own past: what the oracle's accounts were then.
    want = {u128(a, "id"): a.tobytes() for a in at_restart}
    assert [r.tobytes() for r in check(engine2, checker, ids, last)] == [want[i] for i in ids if i in want]


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=["node2", "node3"])
def test_node(devices, ledger, gpu_engine_factory):
    sc, checker, ids = ledger["sc"], ledger["checker"], ledger["ids"]
    single = gpu_engine_factory(transfers_max=1 << 14)
    engine = gpu_engine_factory(accounts_max=4096, transfers_max=1 << 14, pass_events_max=2048, pass_batches_max=16,
                                devices=devices)
    assert commit_all(sc, engine, single) == ledger["replies"]
    # First the commit path's own answer: the node's accounts are the oracle's.
    every = [u128(a, "id") for a in ledger["accounts"]]
    current = engine.commit(130, ledger["commit_timestamp"] + 1, ids_body(every))
    assert current == b"".join(a.tobytes() for a in ledger["accounts"])
    for T in ledger["stamps"]:
        got = check(engine, checker, ids, T)
        assert got.tobytes() == single.lookup_accounts_at(ids, T)[0].tobytes()
    T = sc.steps[len(sc.steps) // 2][2]
    for cap in (0, 3, len(ids)):
        check(engine, checker, ids, T, cap=cap)


def test_read_only_and_allocation_free(ledger, gpu_engine_factory):
    """50 calls around which the allocation count, commit_timestamp, the exports and the commit-path
    counters of tbgpu_get_stats (passes, events, transfers, accounts, log_used) stand still; one more
    inside an asynchronous write-back; then the next commit answers as the oracle did."""
    sc, transfers, ids = ledger["sc"], ledger["transfers"], ledger["ids"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    twin = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, engine, twin, steps=sc.steps[:-1])
    resident = engine.export_transfers()
    checker = AsOf(resident, engine.export_accounts())
    before = (engine.commit_timestamp, engine.export_accounts().tobytes(), resident.tobytes(),
              engine.export_posted().tobytes())
    rng = random.Random(3)
    allocations = engine.lib.tbgpu_debug_allocations()
    stats = engine.stats()
    stamps = np.sort(resident["timestamp"])
    for _ in range(50):
        T = int(rng.choice((0, 1, stamps[len(stamps) // 3], stamps[-5], stamps[-1] + 7)))
        engine.lookup_accounts_at(rng.sample(ids, rng.choice((1, 5, len(ids)))), T)
    assert engine.lib.tbgpu_debug_allocations() == allocations
    after = engine.stats()
    assert all(after[k] == stats[k] for k in ("passes", "events", "transfers", "accounts", "log_used"))
    assert before == (engine.commit_timestamp, engine.export_accounts().tobytes(), engine.export_transfers().tobytes(),
                      engine.export_posted().tobytes())
    # One between an asynchronous write-back's start and its wait leaves the delta alone.
    caps = (1 << 14, 1 << 14, 1 << 14)
    engine.checkpoint_delta_async(caps)
    allocations = engine.lib.tbgpu_debug_allocations()
    check(engine, checker, ids, int(stamps[len(stamps) // 2]))
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
    healthy, matched, complete = engine.lookup_accounts_at([1, 2], 20)
    assert matched == 2 and complete
    assert balances_of(healthy[0]) == (100, 0, 0, 0) and balances_of(healthy[1]) == (0, 0, 100, 0)
    engine.set_balances(1, 0, 0, 0, 0)
    with pytest.raises(EnginePanic):
        engine.commit(129, 30, pack_transfer(id=11, pending_id=10, flags=POST))
    with pytest.raises(EnginePanic, match="stopped"):
        engine.commit(129, 40, pack_transfer(id=13, debit_account_id=1, credit_account_id=2, amount=1, ledger=1, code=1))
    checker = AsOf(engine.export_transfers(), engine.export_accounts())
    allocations = engine.lib.tbgpu_debug_allocations()
    for T in (0, 10, 20, 24, 25):
        want, matched, _ = checker.at([2, 1, 2], T)
        got, got_matched, _ = engine.lookup_accounts_at([2, 1, 2], T)
        assert got.tobytes() == want.tobytes() and got_matched == matched == 3
    assert engine.lib.tbgpu_debug_allocations() == allocations


def test_invalid_input(ledger, gpu_engine_factory):
    sc, ids = ledger["sc"], ledger["ids"]
    engine = gpu_engine_factory(transfers_max=1 << 12)
    empty = engine.lookup_accounts_at(ids, 5)
    assert len(empty[0]) == 0 and empty[1:] == (0, True)  # an empty engine
    commit_all(sc, engine, steps=sc.steps[:4])
    T = sc.steps[2][2]
    valid, matched, complete = engine.lookup_accounts_at(ids, T)
    assert matched == len(valid) == len(ids) - 4 and complete
    got, matched, complete = engine.lookup_accounts_at(ids, U64_MAX)
    assert len(got) == 0 and matched == 0 and complete
    got, matched, complete = engine.lookup_accounts_at([], T)
    assert len(got) == 0 and matched == 0 and complete
    fn = engine.lib.tbgpu_lookup_accounts_at
    src = ctypes.create_string_buffer(ids_body(ids), 16 * len(ids))
    sentinel = b"\xAB" * (128 * len(ids))
    out = ctypes.create_string_buffer(sentinel, len(sentinel))
    res = _lib.tbgpu_query_result(count=77, complete=77, matched=77)
    untouched = lambda: out.raw == sentinel and (res.count, res.complete, res.matched) == (77, 77, 77)
    assert fn(engine.h, T, src, 0, out, len(ids), ctypes.byref(res)) == _lib.STATUS_OK and untouched()
    assert fn(engine.h, T, None, 0, None, 0, None) == _lib.STATUS_OK
    assert fn(engine.h, T, None, len(ids), out, len(ids), ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, T, src, len(ids), None, len(ids), ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, T, src, len(ids), out, len(ids), None) == _lib.STATUS_INVALID and out.raw == sentinel
    assert fn(engine.h, T, src, AT_MAX + 1, out, len(ids), ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, U64_MAX, src, len(ids), out, len(ids), ctypes.byref(res)) == _lib.STATUS_OK
    assert out.raw == sentinel and (res.count, res.matched, res.complete) == (0, 0, 1)
    assert fn(engine.h, T, src, len(ids), out, len(ids), ctypes.byref(res)) == _lib.STATUS_OK
    assert res.count == len(valid) and out.raw[:128 * len(valid)] == valid.tobytes()
    assert out.raw[128 * len(valid):] == sentinel[128 * len(valid):]
