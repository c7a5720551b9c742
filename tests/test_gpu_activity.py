"""get_active_accounts (include/tbgpu.h tbgpu_get_active_accounts, csrc/k_activity.h): for a period, one
row per distinct account its records name, from one scan of the HBM log — a device group-by on both of
every record's 128-bit account ids, then a top-k.  Rows, `matched` and `complete` are compared byte for
byte with the checker of tests/harness/activity.py (itself pinned in tests/test_activity_checkers.py),
and the header's four identities are asserted against the engine's own calls."""
import ctypes
import random

import numpy as np
import pytest

from tests.harness.activity import (BY_TRANSFERS, BY_VOLUME, CREDITS, DEBITS, REVERSED, ROWS_MAX, Activity, half_sums, id_of,
                                    transfers_of, volume_of)
from tests.harness.balances import u128
from tests.harness.counterparties import flow_sums
from tests.harness.oracle import OracleEngine
from tests.harness.shard_double import homes_of
from tests.harness.statements import sums, sweep_pairs
from tests.harness.workload import account_id, make_scenario
from tests.test_gpu_query import SCENARIO, by_id, commit_all, posted_states
from tigerbeetle_amd import _lib
from tigerbeetle_amd._lib import EngineError, EnginePanic
from tigerbeetle_amd.types import (ACCOUNT_ACTIVITY_DTYPE, TRANSFER_DTYPE, U64_MAX, TransferFlags, pack_account, pack_activity_filter,
                                   pack_transfer)

pytestmark = pytest.mark.gpu

PENDING = int(TransferFlags.pending)
POST = int(TransferFlags.post_pending_transfer)
VOID = int(TransferFlags.void_pending_transfer)
ROW = 128
MOD = 1 << 128
BOTH = DEBITS | CREDITS
ORDERS = (0, BY_VOLUME, BY_TRANSFERS)


def check(engine, checker, t_open=0, t_close=0, flags=BOTH, id_min=0, limit=ROWS_MAX, cap=None, ledger=0, code=0, evicted=False):
    """One request: rows, matched and complete as the checker has them."""
    want, matched, orphan = checker.of(t_open, t_close, flags, id_min, limit, cap, ledger, code)
    got, got_matched, got_complete = engine.get_active_accounts_raw(
        pack_activity_filter(t_open, t_close, id_min, ledger, code, limit, flags), cap)
    assert len(got) == len(want), (t_open, t_close, flags, id_min, limit, ledger, code, len(got), len(want), got_matched, matched)
    if got.tobytes() != want.tobytes():
        bad = [n for n in range(len(got)) if got[n].tobytes() != want[n].tobytes()]
        raise AssertionError("rows differ: %d of %d, the first %s, period (%d, %d], flags %d, id_min %d, limit %d, ledger %d, code %d"
                             % (len(bad), len(got), bad[:8], t_open, t_close, flags, id_min, limit, ledger, code))
    assert (got_matched, got_complete) == (matched, not evicted and not orphan), (t_open, t_close, flags, id_min, ledger, code)
    return got


def raw_call(engine, filter_bytes, cap, rows=64, fill=b"\xAB", null=()):
    """The C call into a sentinel-filled buffer: (status, result, the buffer's bytes)."""
    src = ctypes.create_string_buffer(bytes(filter_bytes), 64)
    out = ctypes.create_string_buffer(fill * (ROW * rows), ROW * rows)
    res = _lib.tbgpu_query_result(count=77, complete=77, matched=77)
    status = engine.lib.tbgpu_get_active_accounts(engine.h, None if "filter" in null else src, None if "out" in null else out,
                                                  cap, None if "result" in null else ctypes.byref(res))
    return status, (res.count, res.complete, res.matched), out.raw


class Memo:
    """A checker whose answers are kept: the node tests ask what the single engine's sweep asked."""

    def __init__(self, checker):
        self.checker, self.kept = checker, {}

    def of(self, *args, **kwargs):
        key = (args, tuple(sorted(kwargs.items())))
        if key not in self.kept:
            self.kept[key] = self.checker.of(*args, **kwargs)
        return self.kept[key]


def records_of(rows):
    """TRANSFER_DTYPE records from dicts of pack_transfer's arguments (ledger and code filled in)."""
    return np.frombuffer(b"".join(pack_transfer(**dict(dict(ledger=1, code=1), **r)) for r in rows), dtype=TRANSFER_DTYPE)


def loaded(gpu_engine_factory, records, commit_timestamp=None, **options):
    """An engine restarted from `records` alone (no account: the call reads no account table)."""
    engine = gpu_engine_factory(**options)
    engine.load_transfers(records, np.zeros(len(records), dtype=np.uint8))
    engine.set_commit_timestamp(commit_timestamp or int(records["timestamp"].max()))
    return engine


@pytest.fixture(scope="module")
def ledger():
    """test_gpu_query.py's scenario, the oracle that committed all of it, its exports and the checker
    over them (never changed)."""
    sc = make_scenario(2025, **SCENARIO)
    oracle = OracleEngine(4096, 1 << 15)
    replies = commit_all(sc, oracle)
    transfers, accounts = oracle.export_transfers(), oracle.export_accounts()
    sweep = sweep_pairs(sc.steps, transfers, oracle.commit_timestamp)
    count = lambda field: sorted(set(transfers[field].tolist()), key=lambda v: (-int((transfers[field] == v).sum()), v))
    return dict(sc=sc, replies=replies, transfers=transfers, accounts=accounts, commit_timestamp=oracle.commit_timestamp,
                posted=oracle.export_posted(), checker=Memo(Activity(transfers)),
                created={u128(a, "id"): int(a["timestamp"]) for a in accounts}, ledger_of={u128(a, "id"): int(a["ledger"]) for a in accounts},
                ledgers=count("ledger")[:2], codes=count("code")[:2], sweep=sweep[::6] + [(0, 0), (sweep[9][0], 0), (0, sweep[-1][1])])


def paged(engine, checker, t_open, t_close, limit, evicted=False, **kw):
    pages, cursor = [], 0
    while True:
        page = check(engine, checker, t_open, t_close, id_min=cursor, limit=limit, evicted=evicted, **kw)
        if len(page) == 0:
            break
        pages.append(page)
        cursor = id_of(page[-1]) + 1
    return pages


def sweep_engine(engine, ledger, evicted=False):
    """The sweep of the issue: periods, three side choices, three orders, three limits, paging by id_min,
    two ledgers and two codes."""
    checker = ledger["checker"]
    assert checker.of()[1] > 40 and len(ledger["ledgers"]) == 2 and len(ledger["codes"]) == 2
    busy = 0
    for t_open, t_close in ledger["sweep"]:
        for sides in (DEBITS, CREDITS, BOTH):
            for order in ORDERS:
                for limit in (1, 7, ROWS_MAX):
                    busy += len(check(engine, checker, t_open, t_close, sides | order, 0, limit, evicted=evicted))
    assert busy > 2000
    for t_open, t_close in ((0, 0), ledger["sweep"][1]):
        for L in ledger["ledgers"] + [0]:
            for code in ledger["codes"]:
                for flags in (BOTH, DEBITS | BY_VOLUME, BOTH | BY_TRANSFERS):
                    got = check(engine, checker, t_open, t_close, flags, ledger=L, code=code, limit=50, evicted=evicted)
                    assert len(got) > 3 or t_open
            check(engine, checker, t_open, t_close, ledger=L, evicted=evicted)
        check(engine, checker, t_open, t_close, ledger=0xFFFFFF, evicted=evicted)  # a ledger and a code no record carries
        check(engine, checker, t_open, t_close, code=0xFFFF, evicted=evicted)
    # The pages by id_min with limit 7, concatenated, are the unpaged answer.
    for t_open, t_close in ((0, 0), ledger["sweep"][4]):
        whole = check(engine, checker, t_open, t_close, evicted=evicted)
        pages = paged(engine, checker, t_open, t_close, 7, evicted=evicted)
        assert b"".join(p.tobytes() for p in pages) == whole.tobytes() and (len(pages) > 3 or len(whole) < 22)
    return busy


def check_identities(engine, ledger, t_open, t_close):
    """The header's four identities, against the engine's own calls."""
    rows, matched, _ = engine.get_active_accounts(t_open, t_close)
    assert matched == len(rows)
    created = ledger["created"]
    held = [r for r in rows if id_of(r) in created and (t_close == 0 or created[id_of(r)] <= t_close)]
    if held and t_close:  # the statement identity: byte for byte the halves
        statements = engine.get_account_statements([id_of(r) for r in held], t_open, t_close)[0]
        assert len(statements) == len(held)
        for r, s in zip(held, statements):
            (d_in, d_out, d_posted, d_n), (c_in, c_out, c_posted, c_n) = sums(s)
            assert half_sums(r, "debits") == (d_posted, d_in, d_out, d_n) and half_sums(r, "credits") == (c_posted, c_in, c_out, c_n)
    for r in held[::11]:  # the counterparty identity
        paid = engine.get_account_counterparties(id_of(r), t_open, t_close, credits=False)[0]
        assert tuple(sum(flow_sums(p, "to")[q] for p in paid) % MOD for q in range(4)) == half_sums(r, "debits")
    totals = [[sum(half_sums(r, half)[q] for r in rows) for q in range(4)] for half in ("debits", "credits")]  # double entry
    assert [v % MOD for v in totals[0][:3]] == [v % MOD for v in totals[1][:3]] and totals[0][3] % (1 << 64) == totals[1][3] % (1 << 64)
    for L in ledger["ledgers"]:  # the ledger identity
        mine = rows[[ledger["ledger_of"].get(id_of(r)) == L for r in rows]]
        assert engine.get_active_accounts(t_open, t_close, ledger=L)[0].tobytes() == mine.tobytes()
    return len(held)


def test_single_engine_sweep(ledger, gpu_engine_factory):
    sc = ledger["sc"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    assert commit_all(sc, engine) == ledger["replies"]
    assert engine.commit_timestamp == ledger["commit_timestamp"]
    sweep_engine(engine, ledger)
    held = 0
    for t_open, t_close in ledger["sweep"][::2] + [(0, ledger["commit_timestamp"])]:
        held += check_identities(engine, ledger, t_open, t_close)
    assert held > 100
    # out_cap_rows cuts the answer in order, and nothing past count rows is written.
    checker = ledger["checker"]
    for order in ORDERS:
        whole = check(engine, checker, flags=BOTH | order)
        matched = len(whole)
        for cap in (0, 1, matched - 1, matched, matched + 3):
            check(engine, checker, flags=BOTH | order, cap=cap)
            status, result, raw = raw_call(engine, pack_activity_filter(flags=BOTH | order), cap, rows=matched + 8)
            count = min(cap, matched)
            assert status == _lib.STATUS_OK and result == (count, 1, matched)
            assert raw[:ROW * count] == whole[:count].tobytes() and raw[ROW * count:] == b"\xAB" * (len(raw) - ROW * count)
        status, result, raw = raw_call(engine, pack_activity_filter(flags=BOTH | order, limit=9), 5, rows=16)  # a cap below the limit
        assert status == _lib.STATUS_OK and result == (5, 1, matched) and raw[:5 * ROW] == whole[:5].tobytes()
        assert raw[5 * ROW:] == b"\xAB" * (len(raw) - 5 * ROW)
    for by, order in (("volume", BY_VOLUME), ("transfers", BY_TRANSFERS)):
        top = engine.top_accounts(k=5, by=by)
        want = check(engine, checker, flags=BOTH | order, limit=5)
        assert top == [(id_of(r), u128(r, "debits_posted"), u128(r, "credits_posted"), transfers_of(r)) for r in want] and len(top) == 5


def mixed_log(n, n_accounts=50, seed=11):
    """n records over n_accounts accounts in every kind, two ledgers, two codes, amounts that carry across
    the 64-bit word; every pending transfer's post or void follows it."""
    rng = random.Random(seed)
    amounts = [(1 << 64) - 1, 1 << 64, 1 << 100, 1, (1 << 64) - 7]
    rows, open_holds = [], []
    for i in range(n):
        dr = rng.randrange(n_accounts)
        r = dict(id=10**6 + i, debit_account_id=account_id(dr), credit_account_id=account_id((dr + 1 + rng.randrange(n_accounts - 1)) % n_accounts),
                 amount=amounts[i % 5] + i, timestamp=10**12 + i, ledger=1 + i % 2, code=1 + (i // 2) % 2)
        roll = rng.random()
        if roll < 0.2:
            r["flags"] = PENDING
            open_holds.append(r)
        elif roll < 0.35 and open_holds:
            p = open_holds.pop(rng.randrange(len(open_holds)))
            r.update(debit_account_id=p["debit_account_id"], credit_account_id=p["credit_account_id"], pending_id=p["id"],
                     ledger=p["ledger"], code=p["code"])
            if rng.random() < 0.5:
                r.update(flags=POST, amount=p["amount"] - rng.randrange(2))
            else:
                r.update(flags=VOID, amount=p["amount"])
        rows.append(r)
    return records_of(rows)


@pytest.mark.parametrize("n", [63, 64, 65, 511, 512, 513, 8191, 8192, 8193])
def test_log_lengths_at_the_wave_tile_and_workgroup_edges(n, gpu_engine_factory):
    records = mixed_log(n)
    engine = loaded(gpu_engine_factory, records, transfers_max=1 << 14)
    exported = engine.export_transfers()
    assert len(exported) == n
    checker = Activity(exported)
    at = lambda pos: 10**12 + pos
    for order in ORDERS:
        whole = check(engine, checker, flags=BOTH | order)
        assert len(whole) > 20 and sum(transfers_of(r) for r in whole) == 2 * n
    for t_open, t_close in ((at(n - 2), 0), (at(n - 1), 0), (0, at(0)), (at(n // 2), at(n - 2)), (at(62), at(64))):
        for flags in (BOTH, DEBITS | BY_VOLUME, CREDITS | BY_TRANSFERS):
            check(engine, checker, t_open, t_close, flags)
    check(engine, checker, ledger=2, code=1)
    check(engine, checker, flags=BOTH | BY_TRANSFERS, ledger=1, limit=7)


def test_a_tile_of_one_pair_and_a_tile_of_distinct_accounts(gpu_engine_factory):
    """Tile 0: 512 records that all name one pair, H -> G.  Tile 1: 512 records whose 1,024 account fields
    are all distinct.  Tile 2: the pair again, the other way round, mixed with new accounts."""
    H, G = account_id(1), account_id(2)
    rows = [dict(debit_account_id=H, credit_account_id=G, amount=(1 << 64) - 1 - i, flags=PENDING if i % 9 == 0 else 0) for i in range(512)]
    rows += [dict(debit_account_id=account_id(100 + 2 * i), credit_account_id=account_id(101 + 2 * i) | (i % 3) << 64, amount=1 + i)
             for i in range(512)]
    rows += [dict(debit_account_id=G, credit_account_id=H, amount=7) if i % 2 else
             dict(debit_account_id=account_id(3000 + i), credit_account_id=H, amount=1 << 70) for i in range(512)]
    for k, r in enumerate(rows):
        r.update(id=10**6 + k, timestamp=10**12 + k)
    engine = loaded(gpu_engine_factory, records_of(rows), accounts_max=4096, transfers_max=1 << 12)
    checker = Activity(engine.export_transfers())
    at = lambda pos: 10**12 + pos
    for order in ORDERS:
        whole = check(engine, checker, flags=BOTH | order)
        assert len(whole) == 2 + 1024 + 256
        assert len(check(engine, checker, 0, at(511), BOTH | order)) == 2       # the tile of one pair alone
        assert len(check(engine, checker, at(511), at(1023), BOTH | order)) == 1024  # the tile of distinct accounts alone
        check(engine, checker, at(100), at(700), DEBITS | order)
        check(engine, checker, at(100), at(1300), CREDITS | order, limit=9)
    rows = {id_of(r): r for r in check(engine, checker)}
    assert half_sums(rows[H], "debits")[3] == 512 and half_sums(rows[H], "credits")[3] == 512 and u128(rows[H], "debits_posted") >> 64
    assert half_sums(rows[G], "credits")[3] == 512 and half_sums(rows[G], "debits") == (7 * 256, 0, 0, 256)


def test_more_distinct_keys_than_lds_bins_and_the_group_table_full(gpu_engine_factory):
    """One workgroup scans 8,192 positions into 512 claimed LDS bins.  513 debit accounts, each named in
    several of its records, are one more key than the bins hold under DEBITS; both sides double that.
    Then a table of 32 slots exactly full, and one group over."""
    groups = 513
    order = list(range(4 * groups))
    random.Random(5).shuffle(order)
    sink = account_id(9)
    records = records_of([dict(id=10**6 + j, debit_account_id=account_id(100 + j % groups),
                               credit_account_id=sink if j % 3 else account_id(100 + (j + 1) % groups), amount=(1 << 63) + j,
                               timestamp=10**12 + k, flags=PENDING if j % 7 == 0 else 0) for k, j in enumerate(order)])
    wide = loaded(gpu_engine_factory, records, accounts_max=1 << 12, transfers_max=1 << 13)
    checker = Activity(wide.export_transfers())
    for flags in (DEBITS, BOTH, CREDITS | BY_VOLUME, BOTH | BY_TRANSFERS, DEBITS | BY_VOLUME):
        got = check(wide, checker, flags=flags)
        assert len(got) == {DEBITS: groups, BOTH: groups + 1, CREDITS: 172}[flags & BOTH]
    assert (check(wide, checker, flags=DEBITS)["debits_transfers"] == 4).all()
    check(wide, checker, 10**12 + 99, 10**12 + 1500, BOTH | BY_VOLUME, limit=100)
    # accounts_max 16: a table of 32 slots.  32 distinct accounts fill it exactly; a 33rd has no slot.
    pairs = [dict(id=10**6 + j, debit_account_id=1000 + 2 * j, credit_account_id=1001 + 2 * j, amount=1 + j, timestamp=10**12 + j)
             for j in range(16)]
    over = dict(id=10**6 + 16, debit_account_id=1000, credit_account_id=2000, amount=5, timestamp=10**12 + 16)
    engine = loaded(gpu_engine_factory, records_of(pairs + [over]), accounts_max=16, transfers_max=1 << 10)
    checker = Activity(engine.export_transfers())
    full = 10**12 + 15
    for order in ORDERS:
        assert len(check(engine, checker, 0, full, BOTH | order)) == 32  # exactly full
        assert len(check(engine, checker, 0, full, BOTH | order, limit=5)) == 5
    assert checker.of()[1] == 33
    for order in ORDERS:
        status, result, raw = raw_call(engine, pack_activity_filter(flags=BOTH | order), 64)
        assert status == _lib.STATUS_INVALID and result[0] == 0 and result[2] == 0 and raw == b"\xAB" * len(raw)
        message = engine.lib.tbgpu_last_error().decode()
        assert "capacity" in message and "16 groups" in message and "get_active_accounts" in message
    with pytest.raises(EngineError):
        engine.get_active_accounts(by="volume")
    assert len(check(engine, checker, flags=DEBITS)) == 16 and len(check(engine, checker, id_min=1001)) == 32  # narrower requests fit
    assert len(check(engine, checker, 10**12 + 8, 0, flags=BOTH | BY_VOLUME)) == 16


@pytest.fixture(scope="module")
def select_log():
    """8,200 accounts that each pay one sink once, in a shuffled log: every count is 1 on the debit side,
    and the volumes are (j % 41) << 64 | 5 — equal low words that differ in the high word and long runs
    of ties the id breaks; every 40th account only holds (volume 0); some ids carry a high word."""
    groups, sink = 8200, account_id(0)
    x = lambda j: (100 + j) | ((j % 3) << 64)
    rows = []
    for j in range(groups):
        if j % 40 == 7:
            rows.append(dict(debit_account_id=x(j), credit_account_id=sink, amount=1 + j, flags=PENDING))
        else:
            rows.append(dict(debit_account_id=x(j), credit_account_id=sink, amount=((j % 41) << 64) | 5))
    random.Random(7).shuffle(rows)
    for k, r in enumerate(rows):
        r.update(id=10**6 + k, timestamp=10**12 + k)
    return dict(records=records_of(rows), groups=groups, x=x, sink=sink)


def test_selection(select_log, gpu_engine_factory):
    groups = select_log["groups"]
    engine = loaded(gpu_engine_factory, select_log["records"], accounts_max=1 << 14, transfers_max=1 << 14)
    checker = Activity(engine.export_transfers())
    assert checker.of(flags=DEBITS)[1] == groups and checker.of()[1] == groups + 1
    by_volume = checker.of(flags=DEBITS | BY_VOLUME, limit=ROWS_MAX)[0]
    volumes = [volume_of(r) for r in by_volume]
    assert volumes[0] >> 64 and volumes[-1] == 0 and len(set(volumes)) < 200  # long ties
    assert any(volumes[k] == volumes[k + 1] for k in (0, 99, 4999))  # ... across these cuts
    assert {transfers_of(r) for r in by_volume} == {1}  # every count is 1: the id words decide
    for order in ORDERS:
        for limit in (1, 2, 100, 101, 5000, ROWS_MAX, ROWS_MAX + 500):  # k = 8,191 of M = 8,200
            got = check(engine, checker, flags=DEBITS | order, limit=limit)
            assert len(got) == min(limit, ROWS_MAX)
        check(engine, checker, flags=BOTH | order, limit=777)
        check(engine, checker, flags=CREDITS | order, limit=777)
    assert id_of(check(engine, checker, flags=BOTH | BY_TRANSFERS, limit=3)[0]) == select_log["sink"]
    # M = k - 1, k and k + 1: a period that holds M groups' records.
    stamps = select_log["records"]["timestamp"]
    for m in (40, 300):
        t_close = int(stamps[m])
        have = checker.of(0, t_close, DEBITS)[1]
        for order in ORDERS:
            for limit in (have - 1, have, have + 1):
                check(engine, checker, 0, t_close, DEBITS | order, limit=limit)
    # id_min: above every id, with a high word, and in between; under the ranked orders it narrows the groups.
    top = max(max(select_log["x"](j) for j in range(groups)), select_log["sink"])
    assert top >> 64
    for id_min in (top + 1, top, 1 << 64, (2 << 64) | 5, 4000, (1 << 64) | 4000):
        for order in ORDERS:
            check(engine, checker, flags=BOTH | order, id_min=id_min, limit=50)
    assert checker.of(id_min=top + 1)[1] == 0 and checker.of(id_min=top)[1] == 1


def test_eviction_and_orphaned_posts(ledger, gpu_engine_factory):
    transfers, accounts = ledger["transfers"], ledger["accounts"]
    evicted = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(ledger["sc"], evicted)
    assert evicted.get_active_accounts()[2] is True
    evicted.checkpoint_delta()
    assert evicted.evict_transfers(700) > 0
    resident = evicted.export_transfers()
    checker = Activity(resident)
    stamps = [int(t) for t in np.sort(resident["timestamp"])]
    for t_open, t_close in ((0, 0), (stamps[0] - 1, 0), (stamps[len(stamps) // 2], stamps[-5]), (1, stamps[0] - 1)):
        for flags in (BOTH, DEBITS | BY_VOLUME, CREDITS | BY_TRANSFERS):
            check(evicted, checker, t_open, t_close, flags, evicted=True)
    # Loaded without some pending transfers: nothing was evicted, the orphans alone drop `complete`.
    states = posted_states(transfers, ledger["posted"])
    pending = {u128(t, "id"): t for t in transfers if int(t["flags"]) & PENDING}
    posts = [t for t in transfers if int(t["flags"]) & POST and not int(t["flags"]) & PENDING
             and u128(t, "debit_account_id") != u128(t, "credit_account_id") and u128(t, "pending_id") in pending]
    assert len(posts) > 3
    orphans = posts[len(posts) // 2:]
    lost = {u128(p, "pending_id") for p in orphans}
    keep = np.array([u128(t, "id") not in lost for t in transfers])
    engine = gpu_engine_factory(transfers_max=1 << 14)
    engine.load_accounts(accounts)
    engine.load_transfers(transfers[keep], states[keep])
    engine.set_commit_timestamp(ledger["commit_timestamp"])
    checker = Activity(engine.export_transfers())
    o = min(orphans, key=lambda p: int(p["timestamp"]))  # the oldest orphan post
    d, c, ts = u128(o, "debit_account_id"), u128(o, "credit_account_id"), int(o["timestamp"])
    L, code = int(o["ledger"]), int(o["code"])
    requests = [dict(t_open=ts - 1, t_close=ts), dict(t_open=ts - 1, t_close=ts, flags=DEBITS | BY_VOLUME),
                dict(t_open=ts - 1, t_close=ts, flags=CREDITS | BY_TRANSFERS), dict(t_open=ts - 1, t_close=ts, ledger=L, code=code),
                dict(t_open=0, t_close=ts - 1), dict(t_open=ts, t_close=ts),                         # outside the period
                dict(t_open=ts - 1, t_close=ts, code=code + 1), dict(t_open=ts - 1, t_close=ts, ledger=L + 1),  # a failing code, a failing ledger
                dict(t_open=ts - 1, t_close=ts, id_min=max(d, c) + 1), dict(t_open=0, t_close=0, limit=1)]  # its groups below id_min, or cut off
    verdicts = []
    for kw in requests:
        check(engine, checker, **kw)
        verdicts.append(checker.of(**kw)[2])
    assert verdicts == [True, True, True, True, False, False, False, False, True, True]
    rows = {id_of(r): r for r in engine.get_active_accounts(ts - 1, ts)[0]}
    amount = u128(o, "amount")
    assert half_sums(rows[d], "debits") == (amount, 0, amount, 1) == half_sums(rows[c], "credits")  # P = its own amount
    assert engine.get_active_accounts(ts - 1, ts, out_cap_rows=0)[1:] == (2, False)


def test_restart_from_a_shuffled_log(gpu_engine_factory):
    kw = dict(n_accounts=8, n_transfer_batches=20, batch_len=(100, 300), p_pending=0.3, p_dup=0.05, p_linked=0.05,
              p_limit=0.0, p_balancing=0.0, p_invalid=0.05, id_space=1 << 40)
    sa = make_scenario(31, p_post_void=0.25, **kw)
    oracle = OracleEngine(64, 1 << 15)
    commit_all(sa, oracle)
    transfers, accounts = oracle.export_transfers(), oracle.export_accounts()
    states = posted_states(transfers, oracle.export_posted())
    last = oracle.commit_timestamp
    S = u128(accounts[0], "id")
    selfs = records_of([dict(id=(1 << 50) + k, debit_account_id=S, credit_account_id=S, amount=(1 << 64) - 1 - k,
                             flags=PENDING if k == 1 else 0, timestamp=last + 1 + k) for k in range(3)])
    everything = np.concatenate([transfers, selfs])
    every_state = np.concatenate([states, np.zeros(3, dtype=np.uint8)])
    ordered = gpu_engine_factory(transfers_max=1 << 15)
    ordered.load_accounts(accounts)
    ordered.load_transfers(everything, every_state)
    ordered.set_commit_timestamp(last + 3)
    order = np.random.default_rng(5).permutation(len(everything))
    engine = gpu_engine_factory(transfers_max=1 << 15)
    engine.load_accounts(accounts)
    engine.load_transfers(everything[order], every_state[order])
    engine.set_commit_timestamp(last + 3)
    exported = engine.export_transfers()
    assert len(exported) == len(everything) and len(transfers) > 500
    checker = Activity(exported)
    stamps = [int(t) for t in np.sort(exported["timestamp"])]
    for t_open, t_close in ((0, 0), (stamps[len(stamps) // 3], stamps[-40]), (last, 0), (last + 1, last + 2), (0, stamps[50])):
        for flags in (BOTH, DEBITS, CREDITS, BOTH | BY_VOLUME, BOTH | BY_TRANSFERS):
            got = check(engine, checker, t_open, t_close, flags)
            same = ordered.get_active_accounts_raw(pack_activity_filter(t_open, t_close, flags=flags))
            assert same[0].tobytes() == got.tobytes() and same[1] == len(got)  # the same bytes as from the log in order
    own = {id_of(r): r for r in check(engine, checker, last, 0)}  # the loaded records from S to itself: both halves of one row
    assert list(own) == [S] and half_sums(own[S], "debits") == half_sums(own[S], "credits") == (2 * (1 << 64) - 4, (1 << 64) - 2, 0, 3)
    half = check(engine, checker, last, 0, DEBITS)[0]
    assert half_sums(half, "credits") == (0, 0, 0, 0) and half_sums(half, "debits")[3] == 3


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=["node2", "node3"])
def test_node(devices, ledger, gpu_engine_factory):
    sc, checker, transfers = ledger["sc"], ledger["checker"], ledger["transfers"]
    world = len(devices)
    single = gpu_engine_factory(transfers_max=1 << 14)
    engine = gpu_engine_factory(accounts_max=4096, transfers_max=1 << 14, pass_events_max=2048, pass_batches_max=16, devices=devices)
    assert commit_all(sc, engine, single) == ledger["replies"]
    home = homes_of(np.stack([transfers["id_lo"], transfers["id_hi"]], axis=1), world)
    assert len(set(home.tolist())) == world  # every shard holds a part of the log
    sweep_engine(engine, ledger)
    for order in ORDERS:
        for t_open, t_close in ledger["sweep"][::4]:
            got = check(engine, checker, t_open, t_close, BOTH | order)
            assert got.tobytes() == single.get_active_accounts_raw(pack_activity_filter(t_open, t_close, flags=BOTH | order))[0].tobytes()
    check_identities(engine, ledger, 0, ledger["commit_timestamp"])
    whole = check(engine, checker)
    status, result, raw = raw_call(engine, pack_activity_filter(limit=9), 5, rows=16)
    assert status == _lib.STATUS_OK and result == (5, 1, len(whole))
    assert raw[:5 * ROW] == whole[:5].tobytes() and raw[5 * ROW:] == b"\xAB" * (len(raw) - 5 * ROW)


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=["node2", "node3"])
def test_node_rank_is_of_the_totals(devices, gpu_engine_factory):
    """Every shard holds a payer of its own worth 100 in two records and one worth 90 in one, and one
    record of 60 from a payer all shards share: in each shard's part the shared payer ranks last by
    volume and by count alike, in the totals it ranks first by both."""
    world = len(devices)
    engine = gpu_engine_factory(accounts_max=4096, transfers_max=1 << 12, pass_events_max=2048, pass_batches_max=16, devices=devices)
    sink, shared = 1, 2
    n_acc = 2 + 2 * world
    assert engine.commit(128, 10**12, b"".join(pack_account(id=1 + i, ledger=1, code=1) for i in range(n_acc))) == b""
    candidates = np.array([[10**6 + k, 0] for k in range(64 * world)], dtype=np.uint64)
    home = homes_of(candidates, world)
    events = []
    for s in range(world):
        ids = [int(candidates[k][0]) for k in range(len(candidates)) if home[k] == s][:4]
        assert len(ids) == 4
        events.append(pack_transfer(id=ids[0], debit_account_id=3 + 2 * s, credit_account_id=sink, amount=50, ledger=1, code=1))
        events.append(pack_transfer(id=ids[1], debit_account_id=3 + 2 * s, credit_account_id=sink, amount=50, ledger=1, code=1))
        events.append(pack_transfer(id=ids[2], debit_account_id=4 + 2 * s, credit_account_id=sink, amount=90, ledger=1, code=1))
        events.append(pack_transfer(id=ids[3], debit_account_id=shared, credit_account_id=sink, amount=60, ledger=1, code=1))
    assert engine.commit(129, 2 * 10**12, b"".join(events)) == b""
    exported = engine.export_transfers()
    assert len(exported) == 4 * world
    assert sorted(homes_of(np.stack([exported["id_lo"], exported["id_hi"]], axis=1), world).tolist()) == sorted(list(range(world)) * 4)
    checker = Activity(exported)
    top = check(engine, checker, flags=DEBITS | BY_VOLUME, limit=2)
    assert [id_of(r) for r in top] == [shared, 3] and [volume_of(r) for r in top] == [60 * world, 100]
    top = check(engine, checker, flags=DEBITS | BY_TRANSFERS, limit=2)
    assert [id_of(r) for r in top] == [shared, 3] and [transfers_of(r) for r in top] == [world, 2]
    assert half_sums(top[0], "debits") == (60 * world, 0, 0, world)
    for order in ORDERS:
        whole = check(engine, checker, flags=BOTH | order)
        assert len(whole) == 2 + 2 * world and (order == 0 or id_of(whole[0]) == sink)
        check(engine, checker, flags=CREDITS | order, limit=2)
        check(engine, checker, flags=DEBITS | order, limit=3)


def test_read_only_and_allocation_free(ledger, gpu_engine_factory):
    """50 calls around which the allocation count, commit_timestamp, the exports and the commit-path
    counters of tbgpu_get_stats stand still; one more inside an asynchronous write-back; then the next
    commit answers as the oracle did."""
    sc, transfers = ledger["sc"], ledger["transfers"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    twin = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, engine, twin, steps=sc.steps[:-1])
    resident = engine.export_transfers()
    checker = Activity(resident)
    before = (engine.commit_timestamp, engine.export_accounts().tobytes(), resident.tobytes(), engine.export_posted().tobytes())
    rng = random.Random(3)
    allocations = engine.lib.tbgpu_debug_allocations()
    stats = engine.stats()
    stamps = [int(t) for t in np.sort(resident["timestamp"])]
    marks = [0, 1, stamps[len(stamps) // 3], stamps[-5], stamps[-1] + 7]
    for _ in range(50):
        t_open = rng.choice(marks)
        t_close = rng.choice([0] + [m for m in marks if m >= t_open])
        engine.get_active_accounts(t_open, t_close, by=rng.choice((None, "volume", "transfers")), limit=rng.choice((1, 9, 8191)),
                                   ledger=rng.choice((0, ledger["ledgers"][0])), code=rng.choice((0, ledger["codes"][0])))
    assert engine.lib.tbgpu_debug_allocations() == allocations
    after = engine.stats()
    assert all(after[k] == stats[k] for k in ("passes", "events", "transfers", "accounts", "log_used"))
    assert before == (engine.commit_timestamp, engine.export_accounts().tobytes(), engine.export_transfers().tobytes(),
                      engine.export_posted().tobytes())
    # One between an asynchronous write-back's start and its wait leaves the delta alone.
    caps = (1 << 14, 1 << 14, 1 << 14)
    engine.checkpoint_delta_async(caps)
    allocations = engine.lib.tbgpu_debug_allocations()
    check(engine, checker, stamps[len(stamps) // 3], stamps[-5], BOTH | BY_VOLUME)
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
    healthy, matched, complete = engine.get_active_accounts(10, 25)
    assert matched == 2 and complete and [id_of(r) for r in healthy] == [1, 2]
    assert (half_sums(healthy[0], "debits"), half_sums(healthy[0], "credits")) == ((0, 100, 0, 1), (7, 0, 0, 1))
    engine.set_balances(1, 0, 0, 0, 0)
    with pytest.raises(EnginePanic):
        engine.commit(129, 30, pack_transfer(id=11, pending_id=10, flags=POST))
    with pytest.raises(EnginePanic, match="stopped"):
        engine.commit(129, 40, pack_transfer(id=13, debit_account_id=1, credit_account_id=2, amount=1, ledger=1, code=1))
    checker = Activity(engine.export_transfers())
    allocations = engine.lib.tbgpu_debug_allocations()
    for t_open, t_close in ((0, 0), (10, 20), (19, 24), (20, 0), (24, 25)):
        for order, by in zip(ORDERS, (None, "volume", "transfers")):
            want, matched, _ = checker.of(t_open, t_close, BOTH | order)
            got, got_matched, _ = engine.get_active_accounts(t_open, t_close, by=by)
            assert got.tobytes() == want.tobytes() and got_matched == matched
    assert engine.lib.tbgpu_debug_allocations() == allocations


def test_invalid_input(ledger, gpu_engine_factory):
    sc = ledger["sc"]
    engine = gpu_engine_factory(transfers_max=1 << 12)
    empty = engine.get_active_accounts(0, 9)
    assert len(empty[0]) == 0 and empty[0].dtype == ACCOUNT_ACTIVITY_DTYPE and empty[1:] == (0, True)  # an empty engine
    commit_all(sc, engine, steps=sc.steps[:4])
    t0, t1, t2 = sc.steps[1][2], sc.steps[2][2], sc.steps[3][2]
    valid, matched, complete = engine.get_active_accounts(t0, t2, limit=50)
    assert matched >= len(valid) > 3 and complete
    good = dict(t_open=t0, t_close=t2, id_min=0, limit=50, flags=BOTH)
    bad = [dict(flags=0), dict(flags=BY_VOLUME), dict(flags=BY_TRANSFERS), dict(flags=BOTH | BY_VOLUME | BY_TRANSFERS),
           dict(flags=BOTH | REVERSED), dict(flags=BOTH | 1 << 3), dict(flags=BOTH | 1 << 10), dict(flags=BOTH | 1 << 31),
           dict(t_open=U64_MAX), dict(t_close=U64_MAX), dict(t_open=U64_MAX, t_close=U64_MAX), dict(t_open=t1, t_close=t0),
           dict(t_open=t2, t_close=1), dict(limit=0)]
    filters = [pack_activity_filter(**dict(good, **kw)) for kw in bad]
    blank = pack_activity_filter(**good)
    filters += [blank[:k] + b"\x01" + blank[k + 1:] for k in (38, 39, 48, 55, 63)]  # a reserved byte
    for f in filters:
        status, result, raw = raw_call(engine, f, 64)
        assert status == _lib.STATUS_OK and result == (0, 1, 0) and raw == b"\xAB" * len(raw), f
        got, m, complete = engine.get_active_accounts_raw(f)
        assert len(got) == 0 and m == 0 and complete
    for null in (("filter",), ("out",), ("result",), ("filter", "out", "result")):
        status, result, raw = raw_call(engine, blank, 64, null=null)
        assert status == _lib.STATUS_INVALID and result == (77, 77, 77) and raw == b"\xAB" * len(raw)
    status, result, raw = raw_call(engine, filters[0], 64, null=("out",))  # NULL before the filter's own checks
    assert status == _lib.STATUS_INVALID
    status, result, raw = raw_call(engine, blank, 64)
    assert status == _lib.STATUS_OK and result == (len(valid), 1, matched)
    assert raw[:ROW * len(valid)] == valid.tobytes() and raw[ROW * len(valid):] == b"\xAB" * (len(raw) - ROW * len(valid))
    assert engine.get_active_accounts(t2, t2)[1] == 0  # an empty period is a valid one
