"""get_change_events (include/tbgpu.h tbgpu_get_change_events, csrc/k_change_events.h): the ledger's
transfers of a timestamp window, each with both accounts as they stood right after it, derived from
the current balances and the HBM log.  Events are compared byte for byte with the checkers of
tests/harness/change_events.py (themselves held to the oracle in tests/test_change_event_checkers.py),
with `matched`, `complete` and the records query_transfers returns for the same window."""
import ctypes
import random

import numpy as np
import pytest

from tests.harness.balances import u128
from tests.harness.change_events import oracle_events, select, spec_events
from tests.harness.oracle import OracleEngine
from tests.harness.shard_double import homes_of
from tests.harness.workload import account_id, make_scenario
from tests.test_gpu_query import SCENARIO, by_id, commit_all, posted_states
from tigerbeetle_amd import _lib
from tigerbeetle_amd._lib import EnginePanic
from tigerbeetle_amd.types import (CHANGE_EVENTS_FILTER_DTYPE, CHANGE_EVENTS_MAX, U64_MAX,
                                   TransferFlags, pack_account, pack_transfer)

pytestmark = pytest.mark.gpu

PENDING = int(TransferFlags.pending)
POST = int(TransferFlags.post_pending_transfer)
VOID = int(TransferFlags.void_pending_transfer)
MAX = CHANGE_EVENTS_MAX


def check(engine, events, complete=True, **filter):
    """One filter: events, matched and complete as expected."""
    want, matched = select(events, **filter)
    got, got_matched, got_complete = engine.get_change_events(**filter)
    assert len(got) == len(want), (filter, len(got), len(want))
    assert got.tobytes() == want.tobytes(), (filter, len(got))
    assert (got_matched, got_complete) == (matched, complete), filter
    return got, matched


@pytest.fixture(scope="module")
def ledger():
    """test_gpu_query.py's scenario, the oracle that committed all of it, its exports and the events
    of the backward definition over them (never changed)."""
    sc = make_scenario(2025, **SCENARIO)
    oracle = OracleEngine(4096, 1 << 15)
    replies = commit_all(sc, oracle)
    transfers, accounts = oracle.export_transfers(), oracle.export_accounts()
    events, incomplete = spec_events(transfers, accounts)
    assert not incomplete.any()
    return dict(sc=sc, replies=replies, transfers=transfers, accounts=accounts, commit_timestamp=oracle.commit_timestamp,
                events=events)


def test_single_engine_sweep(ledger, gpu_engine_factory):
    sc, transfers, events = ledger["sc"], ledger["transfers"], ledger["events"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    assert commit_all(sc, engine) == ledger["replies"]
    ts = np.sort(transfers["timestamp"])
    third, mid, last = int(ts[len(ts) // 3]), int(ts[len(ts) // 2]), int(ts[-1])
    windows = [dict(), dict(timestamp_min=mid), dict(timestamp_max=mid), dict(timestamp_min=third, timestamp_max=mid),
               dict(timestamp_min=third), dict(timestamp_min=third + 1), dict(timestamp_min=last + 1)]
    cut = False
    answers = []
    for win in windows:
        for limit in (1, 25, MAX):
            got, matched = check(engine, events, limit=limit, **win)
            cut |= matched > len(got) == limit
            recs, q_matched, _ = engine.query_transfers(limit=limit, **win)
            assert q_matched == matched and got["transfer"].tobytes() == recs.tobytes(), (win, limit)
            answers.append(got)
    got, matched = check(engine, events, timestamp_min=last + 1)
    assert matched == 0 and len(got) == 0
    got, matched = check(engine, events, limit=25, out_cap_events=10)
    assert len(got) == 10 and matched > 25
    first_at_third, _ = check(engine, events, timestamp_min=third, limit=1)
    past_third, _ = check(engine, events, timestamp_min=third + 1, limit=1)
    assert int(first_at_third["transfer"]["timestamp"][0]) == third < int(past_third["transfer"]["timestamp"][0])
    # Non-vacuity: a limit cut an answer; some event is a partial post; some event lies between a
    # pending transfer and its void on that transfer's debit account; some account is on the debit
    # side of one returned event and on the credit side of another.
    assert cut
    returned = np.concatenate(answers)
    at = {u128(t, "id"): t for t in transfers if t["flags"] & PENDING}
    rt = returned["transfer"]
    partial = [t for t in rt if t["flags"] & POST and u128(t, "amount") < u128(at[u128(t, "pending_id")], "amount")]
    assert partial
    between = 0
    for v in transfers[(transfers["flags"] & VOID) != 0]:
        p, account = at[u128(v, "pending_id")], u128(v, "debit_account_id")
        inside = rt[(rt["timestamp"] > p["timestamp"]) & (rt["timestamp"] < v["timestamp"])]
        between += sum(1 for t in inside if u128(t, "debit_account_id") == account)
    assert between > 0
    page = answers[2]  # the open start at limit MAX
    debit_side = {u128(t, "debit_account_id") for t in page["transfer"]}
    credit_side = {u128(t, "credit_account_id") for t in page["transfer"]}
    assert debit_side & credit_side


def test_tile_and_wave_boundaries(gpu_engine_factory):
    """One 600-event prepare committed in place (tbgpu_log_window), so log position = event index.
    Account A's transfers sit at the scan's wave and tile boundaries, with a pending transfer and its
    partial post, another and its void, failing events that name A, and amounts whose sums carry
    across the 64-bit word.  Pages that end at positions 62..64, 254..256 and 510..512 put the first
    record that is newer than the page at every wave and tile edge of k_query.h and k_change_events.h."""
    engine = gpu_engine_factory(transfers_max=1 << 12)
    n_acc, A = 8, account_id(0)
    accounts = [pack_account(id=account_id(i), ledger=1, code=1) for i in range(n_acc)]
    assert engine.commit(128, 10**12, b"".join(accounts)) == b""
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
    events = oracle_events([("commit", 128, 10**12, accounts), ("commit", 129, ts, batch)], 64, 1 << 12)
    first = ts - 600 + 1
    assert events["transfer"]["timestamp"].tolist() == [first + i for i in range(600) if i not in (65, 254)]
    window = engine.log_window(600)
    engine.to_device(window, np.frombuffer(body, dtype=np.uint8))
    res, rb = engine.alloc(600 * 8), engine.alloc(4)
    engine.commit_device_async(129, [ts], [600], window, res, rb)
    # The query drains the pending call itself.
    for limit in (1, 2, 63, 64, 65, 256):
        check(engine, events, limit=limit)
    for end in (62, 63, 64, 254, 255, 256, 510, 511, 512):
        got, _ = check(engine, events, timestamp_max=first + end)
        assert int(got["transfer"]["timestamp"][-1]) == first + (253 if end == 254 else end)
        check(engine, events, timestamp_min=first + end - 1, timestamp_max=first + end, limit=2)
    check(engine, events, timestamp_min=first + 599)
    mine = events[(events["transfer"]["debit_account_id_lo"] == A & U64_MAX) | (events["transfer"]["credit_account_id_lo"] == A & U64_MAX)]
    assert len(mine) == 11
    assert mine["debit_account"]["debits_pending_hi"].max() > 0 and mine["debit_account"]["debits_posted_hi"].max() > 0
    assert mine["credit_account"]["credits_posted_hi"].max() > 0
    engine.free(res)
    engine.free(rb)


def test_page_at_capacity(gpu_engine_factory):
    """Two accounts and more transfers than three pages hold: every page is full, each account's bin
    takes every newer record, and paging with timestamp_min = last + 1 returns the whole ledger."""
    sc = make_scenario(41, n_accounts=2, n_transfer_batches=3, batch_len=(4000, 4000), p_limit=0, p_linked=0,
                       p_balancing=0, p_pending=0.2, p_post_void=0.15, id_space=1 << 40, ledgers=(1,))
    oracle = OracleEngine(64, 1 << 15)
    engine = gpu_engine_factory(transfers_max=1 << 15)
    commit_all(sc, oracle, engine)
    events, incomplete = spec_events(oracle.export_transfers(), oracle.export_accounts())
    assert not incomplete.any() and len(events) > 3 * MAX
    got, matched = check(engine, events, limit=MAX)
    assert matched > len(got) == MAX
    pages, after = [], 0
    while True:
        got, matched, complete = engine.get_change_events(timestamp_min=after, limit=MAX)
        assert complete and matched == len(events) - sum(len(p) for p in pages)
        if len(got) == 0:
            break
        pages.append(got)
        after = int(got["transfer"]["timestamp"][-1]) + 1
    assert len(pages) == -(-len(events) // MAX)
    assert np.concatenate(pages).tobytes() == events.tobytes()
    newest = pages[-1][-1]
    ids = [[int(newest["transfer"][n + "_lo"]), int(newest["transfer"][n + "_hi"])] for n in ("debit_account_id", "credit_account_id")]
    current, found = engine.fetch_accounts(ids)
    assert found.all()
    assert newest["debit_account"].tobytes() == current[0].tobytes() and newest["credit_account"].tobytes() == current[1].tobytes()


def test_set_at_capacity(gpu_engine_factory):
    """A page of 2,730 events that names 5,460 distinct accounts — the set and the bins at their
    capacity — and a second prepare whose transfers all name accounts of that page, so every bin takes
    adds.  (Two accounts of their own per transfer need 6,000 accounts for 3,000 transfers.)  At limit
    2730 and at 2729, where the set is two accounts short of full."""
    n = 3000
    oracle = OracleEngine(8192, 1 << 14)
    engine = gpu_engine_factory(accounts_max=8192, transfers_max=1 << 14)
    accounts = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(2 * n))
    first = b"".join(pack_transfer(id=10**6 + j, debit_account_id=account_id(2 * j), credit_account_id=account_id(2 * j + 1),
                                   amount=1 + j, ledger=1, code=1) for j in range(n))
    second = b"".join(pack_transfer(id=2 * 10**6 + j, debit_account_id=account_id(2 * j + 1),
                                    credit_account_id=account_id((2 * j + 2) % (2 * n)), amount=(1 << 64) - 1 - j, ledger=1, code=1,
                                    flags=PENDING if j % 3 == 0 else 0) for j in range(n))
    for e in (oracle, engine):
        assert e.commit(128, 10**12, accounts) == b""
        assert e.commit(129, 2 * 10**12, first) == b""
        assert e.commit(129, 3 * 10**12, second) == b""
    events, incomplete = spec_events(oracle.export_transfers(), oracle.export_accounts())
    assert len(events) == 2 * n and not incomplete.any()
    for limit in (MAX, MAX - 1):
        got, matched = check(engine, events, limit=limit)
        assert matched == 2 * n and len(got) == limit
        t = got["transfer"]
        distinct = {u128(r, f) for r in t for f in ("debit_account_id", "credit_account_id")}
        assert len(distinct) == 2 * limit
        assert got["debit_account"]["debits_posted_lo"].min() > 0 and got["credit_account"]["debits_pending_lo"].max() == 0
    # A page of the second prepare: accounts on both sides of the page, the older prepare below it.
    check(engine, events, timestamp_min=int(events["transfer"]["timestamp"][n + 100]), limit=MAX)
    assert engine.export_accounts().tobytes() == oracle.export_accounts().tobytes()


def test_unordered_log(gpu_engine_factory):
    """test_gpu_balances.py's unordered log — half B committed, then half A (earlier timestamps, with
    the accounts that carry their effects) loaded shuffled: the newer records sit at LOWER log
    positions than every row of a page of loaded records, and the balances still subtract them.  With
    the whole key buffer and with one small enough that a page's rows take several rounds."""
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
    engine2.load_accounts(engine1.export_accounts())
    engine2.set_commit_timestamp(last)
    assert len(b_steps) >= 2
    commit_all(sb, oracle, engine2, steps=b_steps)
    order = np.random.default_rng(5).permutation(len(half_a))
    engine2.load_transfers(half_a[order], states[order])
    transfers = oracle.export_transfers()
    assert engine2.export_transfers().tobytes() == transfers.tobytes()
    assert len(half_a) > 1000 and len(transfers) - len(half_a) > 1000
    # The anchor is the current balances, and after plain commits those are the oracle's (a balance add
    # lost under tb_flow's sequential replay once made one differ: test_gpu_late_apply.py).
    assert engine2.export_accounts().tobytes() == oracle.export_accounts().tobytes()
    events, incomplete = spec_events(transfers, oracle.export_accounts())
    assert not incomplete.any()
    for keys_max in (0, 256):
        engine2.query_keys_max(keys_max)
        # Pages of loaded records only (every newer record is at a lower position), pages that
        # straddle the two halves, and pages of committed records only.
        got, _ = check(engine2, events, limit=700)
        assert int(got["transfer"]["timestamp"][-1]) <= last and len(got) == 700 > 2 * 256
        check(engine2, events, timestamp_max=last, limit=MAX)
        check(engine2, events, timestamp_min=int(half_a["timestamp"].max()) - 10**6, limit=600)
        check(engine2, events, timestamp_min=last - 10**9, timestamp_max=last + 2 * 10**9, limit=MAX)
        check(engine2, events, timestamp_min=last + 1, limit=300)
        check(engine2, events, limit=3)


CHAIN_FREE = dict(n_accounts=8, n_transfer_batches=4, batch_len=(100, 200), p_linked=0, p_limit=0, p_balancing=0,
                  p_pending=0.3, p_post_void=0.25)


def test_anchor_setup_action(gpu_engine_factory):
    """tbgpu_test_set_balances between two runs of commits: the events after it are the oracle's own,
    and the events before it follow the definition (anchored at the current balances)."""
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
    events, incomplete = spec_events(oracle.export_transfers(), oracle.export_accounts())
    assert not incomplete.any()
    first = sc.steps[half][2] - len(sc.steps[half][3]) + 1  # the first event after the setup
    forward = oracle_events(sc.steps[:half] + setups + sc.steps[half:], 64, 1 << 12)
    after = forward[forward["transfer"]["timestamp"] >= first]
    assert len(after) > 50 and after.tobytes() == select(events, timestamp_min=first)[0].tobytes()
    for limit in (2, 50, MAX):
        got, _ = check(engine, events, limit=limit, timestamp_min=first)
        check(engine, events, limit=limit)
    assert np.all(got["debit_account"]["debits_posted_hi"] > 0)


def test_anchor_restart_from_checkpointed_balances(gpu_engine_factory):
    """A fresh engine given the checkpointed accounts (tbgpu_load_accounts) and an empty log, then the
    next prepares: its events are the ledger's, though it never saw the transfers behind the balances."""
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
    resident = engine.export_transfers()
    events, incomplete = spec_events(resident, engine.export_accounts())
    assert not incomplete.any()
    forward = oracle_events(sa.steps + b_steps, 64, 1 << 12)
    assert forward[forward["transfer"]["timestamp"] > sa.steps[-1][2]].tobytes() == events.tobytes()
    for limit in (1, 100, MAX):
        check(engine, events, limit=limit)


def test_eviction_of_an_old_prefix(gpu_engine_factory):
    """No two-phase transfers: after eviction the resident events are still the whole ledger's, and
    complete says the older events are elsewhere."""
    sc = make_scenario(61, n_accounts=16, n_transfer_batches=8, batch_len=(100, 300), p_pending=0, p_post_void=0)
    oracle = OracleEngine(4096, 1 << 14)
    engine = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, oracle, engine)
    whole, incomplete = spec_events(oracle.export_transfers(), oracle.export_accounts())
    assert not incomplete.any()
    engine.checkpoint_delta()
    assert engine.evict_transfers(500) > 0
    resident = engine.export_transfers()
    assert 0 < len(resident) < len(whole)
    events = whole[whole["transfer"]["timestamp"] >= int(resident["timestamp"].min())]
    assert len(events) == len(resident)
    for limit in (1, 100, MAX):
        check(engine, events, complete=False, limit=limit)
    check(engine, events, complete=False, timestamp_min=int(np.sort(resident["timestamp"])[len(resident) // 2]), limit=50)


def test_eviction_orphans_posts(ledger, gpu_engine_factory):
    """The two-phase ledger evicted: resident posts have lost their pending transfers, and the events
    are the header's definition over what is resident (P = the post's own amount)."""
    sc = ledger["sc"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, engine)
    engine.checkpoint_delta()
    assert engine.evict_transfers(700) > 0
    resident = engine.export_transfers()
    events, incomplete = spec_events(resident, engine.export_accounts())
    assert incomplete.any() and len(resident) < len(ledger["transfers"])
    orphan_ts = np.sort(events["transfer"]["timestamp"][incomplete])
    for limit in (1, 25, MAX):
        check(engine, events, complete=False, limit=limit)
    check(engine, events, complete=False, timestamp_min=int(orphan_ts[0]), limit=1)       # the page is an orphan post
    check(engine, events, complete=False, timestamp_max=int(orphan_ts[0]) - 1, limit=MAX)  # orphans only above the page


def test_missing_accounts(ledger, gpu_engine_factory):
    """Transfers loaded without some of their accounts: those blocks are zero, the other side's block
    is right, and complete is 0."""
    transfers, accounts = ledger["transfers"], ledger["accounts"]
    oracle = OracleEngine(4096, 1 << 15)
    commit_all(ledger["sc"], oracle)
    states = posted_states(transfers, oracle.export_posted())
    kept = accounts[::2]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    engine.load_accounts(kept)
    engine.load_transfers(transfers, states)
    engine.set_commit_timestamp(ledger["commit_timestamp"])
    events, incomplete = spec_events(transfers, kept)
    assert incomplete.any() and not incomplete.all()
    zero = bytes(128)
    one_sided = [e for e in events if (e["debit_account"].tobytes() == zero) != (e["credit_account"].tobytes() == zero)]
    assert one_sided
    for limit in (1, 25, MAX):
        check(engine, events, complete=False, limit=limit)
    got, _ = check(engine, events, complete=False, timestamp_min=int(one_sided[0]["transfer"]["timestamp"]), limit=1)
    assert got[0].tobytes() == one_sided[0].tobytes()
    whole = np.flatnonzero(~incomplete)
    t = int(events["transfer"]["timestamp"][whole[0]])
    got, _, complete = engine.get_change_events(timestamp_min=t, timestamp_max=t)
    assert len(got) == 1 and complete  # a page whose accounts are all there


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=["node2", "node3"])
def test_node(devices, gpu_engine_factory):
    sc = make_scenario(2026, **dict(SCENARIO, n_accounts=16, n_transfer_batches=6))
    oracle = OracleEngine(4096, 1 << 14)
    single = gpu_engine_factory(transfers_max=1 << 14)
    engine = gpu_engine_factory(accounts_max=4096, transfers_max=1 << 14, pass_events_max=2048, pass_batches_max=16,
                                devices=devices)
    commit_all(sc, oracle, engine, single)
    transfers = oracle.export_transfers()
    world = len(devices)
    posts = transfers[(transfers["flags"] & POST) != 0]
    home = homes_of(np.stack([posts["id_lo"], posts["id_hi"]], axis=1), world)
    pending_home = homes_of(np.stack([posts["pending_id_lo"], posts["pending_id_hi"]], axis=1), world)
    assert np.any(home != pending_home)  # a post reads its pending transfer on another shard
    t_home = homes_of(np.stack([transfers["id_lo"], transfers["id_hi"]], axis=1), world)
    owner = homes_of(np.stack([transfers["debit_account_id_lo"], transfers["debit_account_id_hi"]], axis=1), world)
    assert np.any(t_home != owner)       # an account's record comes from a shard other than the transfer's home
    events, incomplete = spec_events(transfers, oracle.export_accounts())
    assert not incomplete.any()
    ts = np.sort(transfers["timestamp"])
    mid = int(ts[len(ts) // 2])
    cut = False
    for win in (dict(), dict(timestamp_min=mid), dict(timestamp_max=mid), dict(timestamp_min=int(ts[-1]) + 1)):
        for limit in (1, 7, MAX):
            got, matched = check(engine, events, limit=limit, **win)
            cut |= matched > len(got) == limit
            assert got.tobytes() == single.get_change_events(limit=limit, **win)[0].tobytes()
    assert cut


def raw_filter(**fields):
    f = np.zeros(1, dtype=CHANGE_EVENTS_FILTER_DTYPE)
    base = dict(limit=10)
    base.update(fields)
    for name, value in base.items():
        f[name] = value
    return f


def test_invalid_filters(ledger, gpu_engine_factory):
    steps = ledger["sc"].steps[:4]
    engine = gpu_engine_factory(transfers_max=1 << 12)
    empty = engine.get_change_events_raw(raw_filter().tobytes())
    assert len(empty[0]) == 0 and empty[1:] == (0, True)  # a valid filter on an empty engine
    commit_all(ledger["sc"], engine, steps=steps)
    valid, matched, _ = engine.get_change_events_raw(raw_filter().tobytes())
    assert matched > 10 and len(valid) == 10
    reserved = np.zeros(44, dtype=np.uint8)
    reserved[43] = 1
    first = np.zeros(44, dtype=np.uint8)
    first[0] = 1
    invalid = [dict(timestamp_min=U64_MAX), dict(timestamp_max=U64_MAX), dict(timestamp_min=10**12, timestamp_max=10**12 - 1),
               dict(limit=0), dict(reserved=reserved), dict(reserved=first)]
    for fields in invalid:
        got, matched, complete = engine.get_change_events_raw(raw_filter(**fields).tobytes())
        assert len(got) == 0 and matched == 0 and complete, fields
    # NULL arguments are a status, nothing else is.
    f = ctypes.create_string_buffer(raw_filter().tobytes(), 64)
    out = ctypes.create_string_buffer(384 * 10)
    res = _lib.tbgpu_query_result()
    fn = engine.lib.tbgpu_get_change_events
    assert fn(engine.h, None, out, 10, ctypes.byref(res)) == _lib.STATUS_INVALID
    assert fn(engine.h, f, None, 10, ctypes.byref(res)) == _lib.STATUS_INVALID
    assert fn(engine.h, f, out, 10, None) == _lib.STATUS_INVALID
    assert fn(engine.h, f, out, 10, ctypes.byref(res)) == _lib.STATUS_OK and res.count == 10
    assert out.raw == valid.tobytes()
    # limit above the cap and above out_cap_events: the smaller holds.
    got, matched, _ = engine.get_change_events(limit=U64_MAX >> 32, out_cap_events=3)
    assert len(got) == 3 and matched > 3


def test_read_only_and_allocation_free(ledger, gpu_engine_factory):
    sc, transfers = ledger["sc"], ledger["transfers"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    twin = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, engine, twin, steps=sc.steps[:-1])
    resident = engine.export_transfers()
    events, _ = spec_events(resident, engine.export_accounts())
    before = (engine.commit_timestamp, engine.export_accounts().tobytes(), resident.tobytes(),
              engine.export_posted().tobytes())
    rng = random.Random(3)
    allocations = engine.lib.tbgpu_debug_allocations()
    stats = engine.stats()
    stamps = np.sort(resident["timestamp"])
    for _ in range(48):
        engine.get_change_events(limit=rng.choice((1, 5, MAX)), timestamp_min=int(rng.choice((0, stamps[len(stamps) // 3]))),
                                 timestamp_max=int(rng.choice((0, stamps[-5]))))
    assert engine.lib.tbgpu_debug_allocations() == allocations
    after = engine.stats()
    assert all(after[k] == stats[k] for k in ("passes", "events", "transfers", "accounts", "log_used"))
    assert before == (engine.commit_timestamp, engine.export_accounts().tobytes(), engine.export_transfers().tobytes(),
                      engine.export_posted().tobytes())
    # The forty-ninth between an asynchronous write-back's start and its wait leaves the delta alone.
    caps = (1 << 14, 1 << 14, 1 << 14)
    engine.checkpoint_delta_async(caps)
    allocations = engine.lib.tbgpu_debug_allocations()
    check(engine, events, limit=5, timestamp_min=int(stamps[len(stamps) // 2]))
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
    """The fiftieth: tests/test_gpu_alloc.py's way to a device panic (a post whose checked `-=` traps
    after the setup action zeroed the pending balance).  The stopped engine still answers."""
    engine = gpu_engine_factory()
    accounts = b"".join(pack_account(id=i, ledger=1, code=1) for i in (1, 2))
    assert engine.commit(128, 10, accounts) == b""
    assert engine.commit(129, 20, pack_transfer(id=10, debit_account_id=1, credit_account_id=2, amount=100, ledger=1, code=1,
                                                flags=PENDING)) == b""
    assert engine.commit(129, 25, pack_transfer(id=12, debit_account_id=2, credit_account_id=1, amount=7, ledger=1, code=1)) == b""
    healthy, matched, complete = engine.get_change_events()
    assert len(healthy) == matched == 2 and complete
    assert u128(healthy[0]["debit_account"], "debits_pending") == 100 and u128(healthy[1]["credit_account"], "debits_pending") == 100
    engine.set_balances(1, 0, 0, 0, 0)
    with pytest.raises(EnginePanic):
        engine.commit(129, 30, pack_transfer(id=11, pending_id=10, flags=POST))
    with pytest.raises(EnginePanic, match="stopped"):
        engine.commit(129, 40, pack_transfer(id=13, debit_account_id=1, credit_account_id=2, amount=1, ledger=1, code=1))
    allocations = engine.lib.tbgpu_debug_allocations()
    got, matched, _ = engine.get_change_events()
    assert engine.lib.tbgpu_debug_allocations() == allocations
    assert matched >= 2 and got[:2]["transfer"].tobytes() == healthy["transfer"].tobytes()
    events, _ = spec_events(got["transfer"].copy(), engine.export_accounts())
    assert got.tobytes() == events.tobytes()
