"""get_account_balances (include/tbgpu.h tbgpu_get_account_balances, csrc/k_balances.h): an account's
balances after each of its transfers, derived from the current balances and the HBM log.  Rows are
compared byte for byte with the checkers of tests/harness/balances.py (themselves held to the
oracle in tests/test_balance_checkers.py), with `matched`, `complete` and the timestamps
get_account_transfers returns for the same filter."""
import ctypes
import itertools
import random

import numpy as np
import pytest

from tests.harness.balances import balances_of, oracle_rows, pack, replay_rows, select, spec_rows, u128
from tests.harness.oracle import OracleEngine
from tests.harness.shard_double import homes_of
from tests.harness.workload import account_id, make_scenario
from tests.test_gpu_query import SCENARIO, by_id, commit_all, ids_of, posted_states, raw_filter, windows
from tigerbeetle_amd import _lib
from tigerbeetle_amd.types import U64_MAX, TransferFlags, pack_account, pack_transfer

pytestmark = pytest.mark.gpu

PENDING = int(TransferFlags.pending)
POST = int(TransferFlags.post_pending_transfer)
VOID = int(TransferFlags.void_pending_transfer)
SIDES = ((True, False), (False, True), (True, True))


def packed(rows):
    return {account: pack(items) for account, items in rows.items()}


NOTHING = pack([])


def check(engine, tables, account, complete=True, **filter):
    """One filter: rows, matched and complete as expected, and the rows are get_account_transfers'."""
    want, matched = select(tables.get(account, NOTHING), **filter)
    got, got_matched, got_complete = engine.get_account_balances(account, **filter)
    assert got.tobytes() == want.tobytes(), (hex(account), filter, len(got), len(want))
    assert (got_matched, got_complete) == (matched, complete), (hex(account), filter)
    transfers, t_matched, _ = engine.get_account_transfers(account, **filter)
    assert t_matched == matched and np.array_equal(transfers["timestamp"], got["timestamp"]), (hex(account), filter)
    return got, matched


@pytest.fixture(scope="module")
def ledger():
    """test_gpu_query.py's scenario, the oracle that committed all of it, its exports and the
    replayed history (never changed)."""
    sc = make_scenario(2025, **SCENARIO)
    oracle = OracleEngine(4096, 1 << 15)
    replies = commit_all(sc, oracle)
    transfers = oracle.export_transfers()
    return dict(sc=sc, replies=replies, transfers=transfers, posted=oracle.export_posted(),
                accounts=oracle.export_accounts(), commit_timestamp=oracle.commit_timestamp,
                tables=packed(replay_rows(transfers)))


def test_single_engine_sweep(ledger, gpu_engine_factory):
    sc, transfers, tables = ledger["sc"], ledger["transfers"], ledger["tables"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    assert commit_all(sc, engine) == ledger["replies"]
    accounts = ids_of(transfers)
    cut = False
    for account in accounts:
        for (d, c), rev, limit, win in itertools.product(SIDES, (False, True), (1, 25, 8190), windows(transfers, account)):
            got, matched = check(engine, tables, account, debits=d, credits=c, reversed=rev, limit=limit, **win)
            cut |= matched > len(got) == limit
    hot = max(accounts, key=lambda a: len(tables[a][0]))
    last = int(transfers["timestamp"].max())
    got, matched = check(engine, tables, hot, timestamp_min=last + 1)     # a window with no match
    assert matched == 0 and len(got) == 0
    got, matched = check(engine, tables, account_id(5000))                # an account that does not exist
    assert matched == 0 and len(got) == 0
    got, matched = check(engine, tables, hot, limit=25, out_cap_records=10)
    assert len(got) == 10 and matched > 25
    # Non-vacuity: a limit cut an answer; some row follows a partial post; some row lies between a
    # pending transfer and its void.
    assert cut
    at = {u128(t, "id"): t for t in transfers if t["flags"] & PENDING}
    partial = [t for t in transfers if t["flags"] & POST and u128(t, "amount") < u128(at[u128(t, "pending_id")], "amount")]
    assert partial
    row, _, _ = engine.get_account_balances(u128(partial[0], "debit_account_id"),
                                            timestamp_min=int(partial[0]["timestamp"]), limit=1)
    assert int(row["timestamp"][0]) == int(partial[0]["timestamp"])
    between = 0
    for v in transfers[(transfers["flags"] & VOID) != 0]:
        p, account = at[u128(v, "pending_id")], u128(v, "debit_account_id")
        inside, _ = select(tables[account], timestamp_min=int(p["timestamp"]) + 1, timestamp_max=int(v["timestamp"]) - 1)
        between += len(inside)
    assert between > 0  # (the sweep's open windows returned every one of them)


def test_tile_and_wave_boundaries(gpu_engine_factory):
    """One 600-event prepare committed in place (tbgpu_log_window), so log position = event index.
    Account A's transfers sit at the scan's wave and tile boundaries, with a pending transfer and its
    partial post, another and its void, failing events that name A, and amounts whose sums carry
    across the 64-bit word."""
    engine = gpu_engine_factory(transfers_max=1 << 12)
    oracle = OracleEngine(64, 1 << 12)
    n_acc, A = 8, account_id(0)
    accounts = [pack_account(id=account_id(i), ledger=1, code=1) for i in range(n_acc)]
    body = b"".join(accounts)
    assert engine.commit(128, 10**12, body) == oracle.commit(128, 10**12, body) == b""
    rng = random.Random(11)
    amounts = [(1 << 64) - 1, 1 << 64, 1 << 100, 1]
    plain = {0: 0, 63: 1, 64: 2, 255: 3, 256: 0, 511: 1, 599: 2}   # position -> amounts index
    events = []
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
        events.append(pack_transfer(**ev))
    body = b"".join(events)
    ts = 10**12 + 1000
    expected = oracle.commit(129, ts, body)
    assert np.frombuffer(expected, dtype=np.uint32)[0::2].tolist() == [65, 254]  # exactly the planted events failed
    window = engine.log_window(600)
    engine.to_device(window, np.frombuffer(body, dtype=np.uint8))
    res, rb = engine.alloc(600 * 8), engine.alloc(4)
    engine.commit_device_async(129, [ts], [600], window, res, rb)
    # The query drains the pending call itself.
    tables = packed(oracle_rows([("commit", 128, 10**12, accounts), ("commit", 129, ts, events)], 64, 1 << 12))
    mine = tables[A][0]
    assert mine["timestamp"].tolist() == [ts - 600 + i + 1 for i in sorted(list(plain) + [10, 62, 257, 300])]
    assert mine["debits_pending_hi"].max() > 0 and mine["debits_posted_hi"].max() > 0 and mine["credits_posted_hi"].max() > 0
    for rev, limit in itertools.product((False, True), (1, 2, 3, 8190)):
        check(engine, tables, A, reversed=rev, limit=limit)
    for account in (account_id(1), account_id(7)):
        check(engine, tables, account)
    assert engine.export_accounts().tobytes() == oracle.export_accounts().tobytes()
    n_reply = int(engine.to_host(rb, 4).view(np.uint32)[0])
    assert bytes(engine.to_host(res, n_reply)) == expected
    engine.free(res)
    engine.free(rb)


def test_bins_at_capacity(gpu_engine_factory):
    """Two accounts and more transfers than one reply holds: every bin of the limit is in use."""
    sc = make_scenario(41, n_accounts=2, n_transfer_batches=3, batch_len=(4000, 4000), p_limit=0, p_linked=0,
                       p_balancing=0, p_pending=0.2, p_post_void=0.15, id_space=1 << 40, ledgers=(1,))
    oracle = OracleEngine(64, 1 << 15)
    engine = gpu_engine_factory(transfers_max=1 << 15)
    commit_all(sc, oracle, engine)
    tables = packed(replay_rows(oracle.export_transfers()))
    for account in (account_id(0), account_id(1)):
        for rev in (False, True):
            got, matched = check(engine, tables, account, reversed=rev, limit=8190)
            assert matched > len(got) == 8190
        newest, _, _ = engine.get_account_balances(account, reversed=True, limit=8190)
        current, found = engine.fetch_accounts([[account & U64_MAX, account >> 64]])
        assert found[0] and tuple(u128(newest[0], c) for c in
                                  ("debits_pending", "debits_posted", "credits_pending", "credits_posted")) == balances_of(current[0])


def test_unordered_log(gpu_engine_factory):
    """test_gpu_query.py's unordered log — half B committed, then half A (earlier timestamps) loaded
    shuffled: a record finds its bin by timestamp, never by position, with the whole key buffer and
    with one small enough that the rows take several rounds."""
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
    assert engine1.export_accounts().tobytes() == oracle.export_accounts().tobytes()
    # Loaded transfers leave balances alone: half A's effects reach engine2 as a restart's do, in the
    # checkpointed accounts it starts from.
    engine2.load_accounts(engine1.export_accounts())
    engine2.set_commit_timestamp(last)
    commit_all(sb, oracle, engine2, steps=b_steps)
    order = np.random.default_rng(5).permutation(len(half_a))
    engine2.load_transfers(half_a[order], states[order])
    transfers = oracle.export_transfers()
    assert engine2.export_transfers().tobytes() == transfers.tobytes()
    assert engine2.export_accounts().tobytes() == oracle.export_accounts().tobytes()
    assert len(half_a) > 1000 and len(transfers) - len(half_a) > 1000 and states.max() == 2
    tables = packed(replay_rows(transfers))
    for keys_max in (0, 256):
        engine2.query_keys_max(keys_max)
        rounds = False
        for account in ids_of(transfers):
            in_a = len(select(tables[account], timestamp_max=last)[0])
            total = len(tables[account][0])
            assert 3 < in_a < total - 3
            rounds |= total > 3 * 256
            for rev, limit in itertools.product((False, True), (3, in_a + 3, total - 3, 8190)):
                check(engine2, tables, account, reversed=rev, limit=limit)
            check(engine2, tables, account, credits=False, timestamp_min=last - 10**9, timestamp_max=last + 2 * 10**9)
        assert rounds


CHAIN_FREE = dict(n_accounts=8, n_transfer_batches=4, batch_len=(100, 200), p_linked=0, p_limit=0, p_balancing=0,
                  p_pending=0.3, p_post_void=0.25)


def test_anchor_setup_action(gpu_engine_factory):
    """tbgpu_test_set_balances between two runs of commits: the rows after it are anchored at the
    balances it set, as the oracle's are."""
    sc = make_scenario(17, **CHAIN_FREE)
    half = len(sc.steps) - 2
    big = [(1 << 100) + 5, (1 << 64) + 1, (1 << 90) + 9, (1 << 64) - 1]
    oracle = OracleEngine(64, 1 << 12)
    engine = gpu_engine_factory(transfers_max=1 << 12)
    commit_all(sc, oracle, engine, steps=sc.steps[:half])
    setups = [("setup", u128(a, "id"), *[b + i for b in big]) for i, a in enumerate(oracle.export_accounts())]
    assert len(setups) >= 6
    for _, account, *balances in setups:
        oracle.set_balances(account, *balances)
        engine.set_balances(account, *balances)
    commit_all(sc, oracle, engine, steps=sc.steps[half:])
    assert engine.export_accounts().tobytes() == oracle.export_accounts().tobytes()
    tables = packed(oracle_rows(sc.steps[:half] + setups + sc.steps[half:], 64, 1 << 12))
    first = sc.steps[half][2] - len(sc.steps[half][3]) + 1  # the first event after the setup
    rows = 0
    for account in ids_of(oracle.export_transfers()):
        for rev, limit in itertools.product((False, True), (2, 8190)):
            got, _ = check(engine, tables, account, reversed=rev, limit=limit, timestamp_min=first)
        rows += len(got)
        assert np.all(got["debits_posted_hi"] > 0)
    assert rows > 100


def test_anchor_restart_from_checkpointed_balances(gpu_engine_factory):
    """A fresh engine given the checkpointed accounts (tbgpu_load_accounts) and an empty log, then the
    next prepares: its rows are the ledger's, though it never saw the transfers behind the balances."""
    kw = dict(CHAIN_FREE, id_space=1 << 40)
    sa = make_scenario(51, **kw)
    sb = make_scenario(52, start_ts=sa.steps[-1][2] + 10**9, **kw)
    b_steps = [s for s in sb.steps if s[1] == 129]
    oracle = OracleEngine(64, 1 << 12)
    commit_all(sa, oracle)
    engine = gpu_engine_factory(transfers_max=1 << 12)
    engine.load_accounts(oracle.export_accounts())
    engine.set_commit_timestamp(oracle.commit_timestamp)
    assert oracle.export_accounts()["debits_posted_lo"].max() > 0
    commit_all(sb, oracle, engine, steps=b_steps)
    assert engine.export_accounts().tobytes() == oracle.export_accounts().tobytes()
    tables = packed(oracle_rows(sa.steps + b_steps, 64, 1 << 12))
    first = int(engine.export_transfers()["timestamp"].min())
    assert first > sa.steps[-1][2]
    for account in ids_of(engine.export_transfers()):
        for rev, limit in itertools.product((False, True), (1, 8190)):
            check(engine, tables, account, reversed=rev, limit=limit, timestamp_min=first)


def test_eviction_of_an_old_prefix(gpu_engine_factory):
    """No two-phase transfers: after eviction the rows over the resident suffix are still the whole
    ledger's, and complete says the older rows are elsewhere."""
    sc = make_scenario(61, n_accounts=16, n_transfer_batches=8, batch_len=(100, 300), p_pending=0, p_post_void=0)
    oracle = OracleEngine(4096, 1 << 14)
    engine = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, oracle, engine)
    transfers = oracle.export_transfers()
    tables = packed(replay_rows(transfers))
    engine.checkpoint_delta()
    assert engine.evict_transfers(500) > 0
    resident = engine.export_transfers()
    assert 0 < len(resident) < len(transfers)
    oldest = int(resident["timestamp"].min())
    assert set(resident["timestamp"].tolist()) == set(transfers["timestamp"][transfers["timestamp"] >= oldest].tolist())
    for account in ids_of(resident):
        for rev, limit in itertools.product((False, True), (1, 8190)):
            got, matched = select(tables[account], reversed=rev, limit=limit, timestamp_min=oldest)
            rows, got_matched, complete = engine.get_account_balances(account, reversed=rev, limit=limit)
            assert rows.tobytes() == got.tobytes() and got_matched == matched and not complete


def test_eviction_orphans_posts(ledger, gpu_engine_factory):
    """The two-phase ledger evicted: resident posts have lost their pending transfers, and the rows are
    the header's definition over what is resident (P = the post's own amount)."""
    sc = ledger["sc"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, engine)
    engine.checkpoint_delta()
    assert engine.evict_transfers(700) > 0
    resident = engine.export_transfers()
    rows, orphans = spec_rows(resident, engine.export_accounts())
    assert orphans and len(resident) < len(ledger["transfers"])
    tables = packed(rows)
    for account in ids_of(resident):
        for rev, limit in itertools.product((False, True), (1, 25, 8190)):
            check(engine, tables, account, complete=False, reversed=rev, limit=limit)


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=["node2", "node3"])
def test_node(devices, gpu_engine_factory):
    sc = make_scenario(2026, **dict(SCENARIO, n_accounts=16, n_transfer_batches=6))
    oracle = OracleEngine(4096, 1 << 14)
    engine = gpu_engine_factory(accounts_max=4096, transfers_max=1 << 14, pass_events_max=2048, pass_batches_max=16,
                                devices=devices)
    commit_all(sc, oracle, engine)
    transfers = oracle.export_transfers()
    posts = transfers[(transfers["flags"] & POST) != 0]
    home = homes_of(np.stack([posts["id_lo"], posts["id_hi"]], axis=1), len(devices))
    pending_home = homes_of(np.stack([posts["pending_id_lo"], posts["pending_id_hi"]], axis=1), len(devices))
    assert np.any(home != pending_home)  # a post reads its pending transfer on another shard
    tables = packed(replay_rows(transfers))
    cut = False
    for account in ids_of(transfers):
        for (d, c), rev, limit, win in itertools.product(SIDES, (False, True), (1, 7, 8190), windows(transfers, account)):
            got, matched = check(engine, tables, account, debits=d, credits=c, reversed=rev, limit=limit, **win)
            cut |= matched > len(got) == limit
    assert cut
    got, matched = check(engine, tables, account_id(5000))
    assert matched == 0


def test_invalid_filters(ledger, gpu_engine_factory):
    steps = ledger["sc"].steps[:4]
    engine = gpu_engine_factory(transfers_max=1 << 12)
    empty = engine.get_account_balances_raw(raw_filter().tobytes())
    assert len(empty[0]) == 0 and empty[1:] == (0, True)  # a valid filter on an empty engine
    commit_all(ledger["sc"], engine, steps=steps)
    account = ids_of(engine.export_transfers())[0]
    good = dict(account_id_lo=account & U64_MAX, account_id_hi=account >> 64)
    got, matched, _ = engine.get_account_balances_raw(raw_filter(**good).tobytes())
    assert matched > 0 and len(got) == min(matched, 10)
    reserved = np.zeros(24, dtype=np.uint8)
    reserved[23] = 1
    invalid = [dict(account_id_lo=0, account_id_hi=0), dict(account_id_lo=U64_MAX, account_id_hi=U64_MAX),
               dict(timestamp_min=U64_MAX), dict(timestamp_max=U64_MAX), dict(timestamp_min=10**12, timestamp_max=10**12 - 1),
               dict(limit=0), dict(flags=0), dict(flags=4), dict(flags=3 | 8), dict(flags=3 | (1 << 31)),
               dict(reserved=reserved)]
    for fields in invalid:
        got, matched, complete = engine.get_account_balances_raw(raw_filter(**dict(good, **fields)).tobytes())
        assert len(got) == 0 and matched == 0 and complete, fields
    # NULL arguments are a status, nothing else is.
    f = ctypes.create_string_buffer(raw_filter(**good).tobytes(), 64)
    out = ctypes.create_string_buffer(128 * 10)
    res = _lib.tbgpu_query_result()
    fn = engine.lib.tbgpu_get_account_balances
    assert fn(engine.h, None, out, 10, ctypes.byref(res)) == _lib.STATUS_INVALID
    assert fn(engine.h, f, None, 10, ctypes.byref(res)) == _lib.STATUS_INVALID
    assert fn(engine.h, f, out, 10, None) == _lib.STATUS_INVALID
    assert fn(engine.h, f, out, 10, ctypes.byref(res)) == _lib.STATUS_OK and res.count > 0
    assert np.frombuffer(out.raw, dtype=np.uint8).reshape(10, 128)[:res.count, 72:].max() == 0  # reserved bytes are zero


def test_read_only_and_allocation_free(ledger, gpu_engine_factory):
    sc, transfers = ledger["sc"], ledger["transfers"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    twin = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, engine, twin, steps=sc.steps[:-1])
    resident = engine.export_transfers()
    tables = packed(replay_rows(resident))
    before = (engine.commit_timestamp, engine.export_accounts().tobytes(), resident.tobytes(),
              engine.export_posted().tobytes())
    rng = random.Random(3)
    accounts = ids_of(resident)
    allocations = engine.lib.tbgpu_debug_allocations()
    stats = engine.stats()
    for _ in range(49):
        engine.get_account_balances(rng.choice(accounts), debits=rng.random() < 0.7, credits=True, reversed=rng.random() < 0.5,
                                    limit=rng.choice((1, 5, 8190)),
                                    timestamp_min=rng.choice((0, int(resident["timestamp"][len(resident) // 3]))))
    assert engine.lib.tbgpu_debug_allocations() == allocations
    after = engine.stats()
    assert all(after[k] == stats[k] for k in ("passes", "events", "transfers", "accounts", "log_used"))
    assert before == (engine.commit_timestamp, engine.export_accounts().tobytes(), engine.export_transfers().tobytes(),
                      engine.export_posted().tobytes())
    # The fiftieth between an asynchronous write-back's start and its wait leaves the delta alone.
    caps = (1 << 14, 1 << 14, 1 << 14)
    engine.checkpoint_delta_async(caps)
    allocations = engine.lib.tbgpu_debug_allocations()
    check(engine, tables, accounts[0], reversed=True, limit=5)
    assert engine.lib.tbgpu_debug_allocations() == allocations
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
