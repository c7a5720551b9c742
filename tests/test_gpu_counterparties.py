"""get_account_counterparties (include/tbgpu.h tbgpu_get_account_counterparties,
csrc/k_counterparties.h): for one subject account and a period, one row per distinct counterparty from
one scan of the HBM log — a device group-by on the 128-bit id, then a top-k.  Rows, `matched` and
`complete` are compared byte for byte with the checker of tests/harness/counterparties.py (itself pinned
in tests/test_counterparties_checkers.py), and the header's two identities are asserted against the
engine's own get_account_flow_matrix and get_account_statements."""
import ctypes
import random

import numpy as np
import pytest

from tests.harness.balances import u128
from tests.harness.counterparties import BY_VOLUME, CREDITS, DEBITS, REVERSED, ROWS_MAX, Counterparties, flow_sums, id_of, volume_of
from tests.harness.matrix import cell_sums
from tests.harness.oracle import OracleEngine
from tests.harness.shard_double import homes_of
from tests.harness.statements import sums, sweep_pairs
from tests.harness.workload import account_id, make_scenario
from tests.test_gpu_query import SCENARIO, by_id, commit_all, posted_states
from tigerbeetle_amd import _lib
from tigerbeetle_amd._lib import EngineError, EnginePanic
from tigerbeetle_amd.types import (COUNTERPARTY_DTYPE, TRANSFER_DTYPE, U64_MAX, TransferFlags, pack_account, pack_counterparty_filter,
                                   pack_transfer)

pytestmark = pytest.mark.gpu

PENDING = int(TransferFlags.pending)
POST = int(TransferFlags.post_pending_transfer)
VOID = int(TransferFlags.void_pending_transfer)
ROW = 128
MOD = 1 << 128
BOTH = DEBITS | CREDITS
ABSENT = account_id(5000)


def check(engine, checker, account, t_open=0, t_close=0, flags=BOTH, id_min=0, limit=ROWS_MAX, cap=None, evicted=False):
    """One request: rows, matched and complete as the checker has them."""
    want, matched, orphan = checker.of(account, t_open, t_close, flags, id_min, limit, cap)
    got, got_matched, got_complete = engine.get_account_counterparties_raw(
        pack_counterparty_filter(account, t_open, t_close, id_min, limit, flags), cap)
    assert len(got) == len(want), (account, t_open, t_close, flags, id_min, limit, len(got), len(want))
    if got.tobytes() != want.tobytes():
        bad = [n for n in range(len(got)) if got[n].tobytes() != want[n].tobytes()]
        raise AssertionError("rows differ: %d of %d, the first %s, subject %d, period (%d, %d], flags %d, id_min %d, limit %d"
                             % (len(bad), len(got), bad[:8], account, t_open, t_close, flags, id_min, limit))
    assert (got_matched, got_complete) == (matched, not evicted and not orphan), (account, t_open, t_close, flags, id_min)
    return got


def check_identities(engine, created, account, t_open, t_close):
    """The header's identities, against the engine's own calls: `to` is the matrix's cell (a, x), `from`
    its cell (x, a), for every x the table holds at t_close; the halves add up to a's statement."""
    rows, matched, _ = engine.get_account_counterparties(account, t_open, t_close)
    assert matched == len(rows)
    found = lambda i: i in created and (t_close == 0 or created[i] <= t_close)
    if not found(account):
        return 0
    held = [r for r in rows if found(id_of(r))]
    xs = [id_of(r) for r in held]
    if xs:
        paid = engine.get_account_flow_matrix([account], xs, t_open, t_close)[0]
        received = engine.get_account_flow_matrix(xs, [account], t_open, t_close)[0]
        assert len(paid) == len(received) == len(xs)
        for r, p, q in zip(held, paid, received):
            assert r.tobytes()[16:72] == p.tobytes()[32:88] and r.tobytes()[72:128] == q.tobytes()[32:88]  # byte for byte
            assert flow_sums(r, "to") == cell_sums(p) and flow_sums(r, "from") == cell_sums(q)
    statement = engine.get_account_statements([account], t_open, t_close)[0]
    (d_in, d_out, d_posted, d_n), (c_in, c_out, c_posted, c_n) = sums(statement[0])
    for flags, direction, want in ((DEBITS, "to", (d_posted, d_in, d_out, d_n)), (CREDITS, "from", (c_posted, c_in, c_out, c_n))):
        one = engine.get_account_counterparties_raw(pack_counterparty_filter(account, t_open, t_close, 0, ROWS_MAX, flags))[0]
        total = [sum(flow_sums(r, direction)[q] for r in one) for q in range(4)]
        assert tuple(v % MOD for v in total) == want, (account, t_open, t_close, direction)
    return len(held)


def raw_call(engine, filter_bytes, cap, rows=64, fill=b"\xAB", null=()):
    """The C call into a sentinel-filled buffer: (status, result, the buffer's bytes)."""
    src = ctypes.create_string_buffer(bytes(filter_bytes), 64)
    out = ctypes.create_string_buffer(fill * (ROW * rows), ROW * rows)
    res = _lib.tbgpu_query_result(count=77, complete=77, matched=77)
    status = engine.lib.tbgpu_get_account_counterparties(engine.h, None if "filter" in null else src, None if "out" in null else out,
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
    named = {}
    for t in transfers:
        for side in ("debit_account_id", "credit_account_id"):
            named.setdefault(u128(t, side), []).append(int(t["timestamp"]))
    by_count = sorted(named, key=lambda i: (len(named[i]), i))
    hot, cold = by_count[-1], by_count[0]
    late = max(named, key=lambda i: (min(named[i]), i))  # its first record is the newest first record
    sweep = sweep_pairs(sc.steps, transfers, oracle.commit_timestamp)
    return dict(sc=sc, replies=replies, transfers=transfers, accounts=accounts, commit_timestamp=oracle.commit_timestamp,
                posted=oracle.export_posted(), checker=Memo(Counterparties(transfers)), hot=hot, cold=cold, late=late,
                late_first=min(named[late]), created={u128(a, "id"): int(a["timestamp"]) for a in accounts},
                everyone=[u128(a, "id") for a in accounts], sweep=sweep[::5] + [(0, 0), (sweep[9][0], 0), (0, sweep[-1][1])])


def sweep_engine(engine, ledger, evicted=False):
    """The sweep of the issue: four subjects, three sides, both orders, three limits, paging."""
    checker, hot = ledger["checker"], ledger["hot"]
    subjects = [hot, ledger["cold"], ledger["late"], ABSENT]
    groups = checker.of(hot)[1]
    assert groups > 20 and checker.of(ledger["cold"])[1] > 0 and checker.of(ABSENT)[1] == 0
    busy = 0
    for t_open, t_close in ledger["sweep"] + [(0, ledger["late_first"] - 1)]:  # (the last: `late` has records only outside it)
        for a in subjects:
            for sides in (DEBITS, CREDITS, BOTH):
                for order in (0, BY_VOLUME):
                    for limit in (1, groups // 2, groups + 50):
                        busy += len(check(engine, checker, a, t_open, t_close, sides | order, 0, limit, evicted=evicted))
    assert busy > 2000
    assert checker.of(ledger["late"], 0, ledger["late_first"] - 1)[1] == 0 and checker.of(ledger["late"])[1] > 0
    # The pages by id_min with limit 7, concatenated, are the unpaged answer.
    for t_open, t_close in ((0, 0), ledger["sweep"][4]):
        whole = check(engine, checker, hot, t_open, t_close, evicted=evicted)
        pages, cursor = [], 0
        while True:
            page = check(engine, checker, hot, t_open, t_close, id_min=cursor, limit=7, evicted=evicted)
            if len(page) == 0:
                break
            pages.append(page)
            cursor = id_of(page[-1]) + 1
        assert b"".join(p.tobytes() for p in pages) == whole.tobytes() and (len(pages) > 3 or len(whole) < 22)
    return busy


def test_single_engine_sweep(ledger, gpu_engine_factory):
    sc = ledger["sc"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    assert commit_all(sc, engine) == ledger["replies"]
    assert engine.commit_timestamp == ledger["commit_timestamp"]
    sweep_engine(engine, ledger)
    held = 0
    for t_open, t_close in ledger["sweep"][::2]:
        for a in (ledger["hot"], ledger["cold"], ledger["late"]):
            held += check_identities(engine, ledger["created"], a, t_open, t_close)
    assert held > 100
    # out_cap_rows cuts the answer in order, and nothing past count rows is written.
    hot, checker = ledger["hot"], ledger["checker"]
    for order in (0, BY_VOLUME):
        whole = check(engine, checker, hot, flags=BOTH | order)
        matched = len(whole)
        for cap in (0, 1, matched - 1, matched, matched + 3):
            check(engine, checker, hot, flags=BOTH | order, cap=cap)
            status, result, raw = raw_call(engine, pack_counterparty_filter(hot, flags=BOTH | order), cap, rows=matched + 8)
            count = min(cap, matched)
            assert status == _lib.STATUS_OK and result == (count, 1, matched)
            assert raw[:ROW * count] == whole[:count].tobytes() and raw[ROW * count:] == b"\xAB" * (len(raw) - ROW * count)
    top = engine.top_counterparties(hot, 5)
    by_volume = check(engine, checker, hot, flags=BOTH | BY_VOLUME, limit=5)
    assert top == [(id_of(r), u128(r, "to_posted"), u128(r, "from_posted")) for r in by_volume] and len(top) == 5


def edge_log():
    """2 x 8,192 + 1 positions, three workgroups of the scan.  The subject S's records sit at positions
    0, 63, 64, 511, 512, 8,191, 8,192 and the last, each with counterparty E — hit in all three
    workgroups; the wave at 1,024 holds 64 records S -> W; the wave at 2,048 holds 64 records with 64
    different counterparties, alternating direction; amounts carry across the 64-bit word."""
    n = 2 * 8192 + 1
    S, E, W = account_id(0), account_id(1), account_id(2)
    amounts = [(1 << 64) - 1, 1 << 64, 1 << 100, 1, (1 << 64) - 7]
    rng = random.Random(11)
    rows = []
    for i in range(n):
        dr = 10 + rng.randrange(50)
        r = dict(id=10**6 + i, debit_account_id=account_id(dr), credit_account_id=account_id(10 + (dr - 9) % 50), amount=1 + i,
                 timestamp=10**12 + i)
        if i in (0, 63, 64, 511, 512, 8191, 8192, n - 1):
            r.update(debit_account_id=S, credit_account_id=E, amount=amounts[i % 5], flags=PENDING if i % 2 else 0)
        elif 1024 <= i < 1088:
            r.update(debit_account_id=S, credit_account_id=W, amount=amounts[i % 5])
        elif 2048 <= i < 2112:
            x = account_id(100 + i - 2048)
            r.update(amount=amounts[i % 5])
            r.update(debit_account_id=S, credit_account_id=x) if i % 2 else r.update(debit_account_id=x, credit_account_id=S)
        rows.append(r)
    return records_of(rows), S, E, W


def test_tile_wave_and_workgroup_edges(gpu_engine_factory):
    records, S, E, W = edge_log()
    n = len(records)
    engine = loaded(gpu_engine_factory, records, transfers_max=1 << 15)
    exported = engine.export_transfers()
    assert len(exported) == n
    checker = Counterparties(exported)
    at = lambda pos: 10**12 + pos
    for order in (0, BY_VOLUME):
        whole = check(engine, checker, S, flags=BOTH | order)
        assert len(whole) == 2 + 64
    rows = {id_of(r): r for r in check(engine, checker, S)}
    assert flow_sums(rows[E], "to")[3] == 8 and flow_sums(rows[W], "to")[3] == 64 and u128(rows[W], "to_posted") >> 64
    assert sorted(flow_sums(r, "to")[3] + flow_sums(r, "from")[3] for x, r in rows.items() if x not in (E, W)) == [1] * 64
    marks = sorted({e + d for e in (0, 63, 64, 511, 512, 8191, 8192, n - 1, 1024, 1087, 2048, 2111) for d in (-1, 0, 1) if 0 <= e + d < n})
    seen = set()
    for k, m in enumerate(marks):
        for t_open, t_close in ((at(m), 0), (0, at(m)), (at(m), at(marks[k + 1]) if k + 1 < len(marks) else at(m))):
            for flags in (BOTH, DEBITS | BY_VOLUME):
                seen.add(check(engine, checker, S, t_open, t_close, flags).tobytes())
    assert len(seen) > 40
    assert len(check(engine, checker, S, at(2047), at(2111), CREDITS)) == 32  # inside the wave of 64 counterparties
    assert len(check(engine, checker, S, at(1030), at(1050))) == 1
    check(engine, checker, E)
    check(engine, checker, W, flags=CREDITS | BY_VOLUME)


def test_group_table_full_and_more_groups_than_lds_bins(gpu_engine_factory):
    """accounts_max 64 and a subject that deals with all 63 others, committed.  Then 1,499 groups inside
    one workgroup's 8,192 positions — more than its claimed LDS bins — each hit four times there."""
    engine = gpu_engine_factory(accounts_max=64, transfers_max=1 << 12)
    assert engine.commit(128, 10**12, b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(64))) == b""
    S = account_id(0)
    body = b"".join(pack_transfer(id=10**6 + j, debit_account_id=S if j % 2 else account_id(1 + j % 63),
                                  credit_account_id=account_id(1 + j % 63) if j % 2 else S, amount=(1 << 63) + j, ledger=1, code=1,
                                  flags=PENDING if j % 5 == 0 else 0) for j in range(63 * 6))
    assert engine.commit(129, 2 * 10**12, body) == b""
    checker = Counterparties(engine.export_transfers())
    for order in (0, BY_VOLUME):
        assert len(check(engine, checker, S, flags=BOTH | order)) == 63
        check(engine, checker, S, flags=DEBITS | order, limit=10)
    check_identities(engine, {account_id(i): 10**12 for i in range(64)}, S, 0, 0)
    groups = 1499  # not a multiple of 3: either direction reaches every group
    order = list(range(4 * groups))
    random.Random(5).shuffle(order)
    records = records_of([dict(id=10**6 + j, debit_account_id=S if j % 3 else account_id(100 + j % groups),
                               credit_account_id=account_id(100 + j % groups) if j % 3 else S, amount=(1 << 63) + j,
                               timestamp=10**12 + k, flags=PENDING if j % 7 == 0 else 0) for k, j in enumerate(order)])
    wide = loaded(gpu_engine_factory, records, accounts_max=1 << 12, transfers_max=1 << 13)
    checker = Counterparties(wide.export_transfers())
    for flags in (BOTH, BOTH | BY_VOLUME, DEBITS, CREDITS | BY_VOLUME):
        got = check(wide, checker, S, flags=flags)
        assert len(got) == groups
    assert (got["from_transfers"] >= 1).all() and int(got["from_transfers"].sum()) == len(range(0, 4 * groups, 3))
    check(wide, checker, S, 10**12 + 999, 10**12 + 5000, BOTH | BY_VOLUME, limit=100)


def test_group_table_overflow(gpu_engine_factory):
    """accounts_max 16 — a table of 32 slots — and loaded records naming 40 distinct counterparties:
    TBGPU_STATUS_INVALID, the capacity named, nothing written; a narrower period still answers."""
    S = account_id(0)
    records = records_of([dict(id=10**6 + j, debit_account_id=S, credit_account_id=1000 + j, amount=1 + j,
                               timestamp=10**12 + j) for j in range(40)])
    engine = loaded(gpu_engine_factory, records, accounts_max=16, transfers_max=1 << 10)
    checker = Counterparties(engine.export_transfers())
    assert checker.of(S)[1] == 40
    status, result, raw = raw_call(engine, pack_counterparty_filter(S), 64)
    assert status == _lib.STATUS_INVALID and result[0] == 0 and result[2] == 0 and raw == b"\xAB" * len(raw)
    message = engine.lib.tbgpu_last_error().decode()
    assert "capacity" in message and "16 groups" in message
    with pytest.raises(EngineError):
        engine.get_account_counterparties(S, by_volume=True)
    assert len(check(engine, checker, S, 10**12 + 9, 10**12 + 25)) == 16  # a narrower period fits
    assert len(check(engine, checker, S, id_min=1030, flags=DEBITS | BY_VOLUME)) == 10  # and so does a narrower id range


@pytest.fixture(scope="module")
def select_log():
    """8,200 counterparties of one subject, in a shuffled log.  Volumes: counterparty j posts
    (j % 41) << 64 | 5 one way and adds nothing, 2^64 - 5 or 2^64 + 7 the other way: equal low words that
    differ in the high word, sums that carry across 2^64, long runs of ties that the id breaks; every
    40th group holds only (volume 0); some ids carry a high word."""
    S, groups = account_id(0), 8200
    x = lambda j: (100 + j) | ((j % 3) << 64)
    rows = []
    for j in range(groups):
        if j % 40 == 7:
            rows.append(dict(debit_account_id=S, credit_account_id=x(j), amount=1 + j, flags=PENDING))
            continue
        rows.append(dict(debit_account_id=S, credit_account_id=x(j), amount=((j % 41) << 64) | 5))
        if j % 4 == 1:
            rows.append(dict(debit_account_id=x(j), credit_account_id=S, amount=(1 << 64) - 5))
        elif j % 4 == 2:
            rows.append(dict(debit_account_id=x(j), credit_account_id=S, amount=(1 << 64) + 7))
    random.Random(7).shuffle(rows)
    for k, r in enumerate(rows):
        r.update(id=10**6 + k, timestamp=10**12 + k)
    return dict(records=records_of(rows), S=S, groups=groups, x=x)


def test_selection(select_log, gpu_engine_factory):
    S, groups = select_log["S"], select_log["groups"]
    engine = loaded(gpu_engine_factory, select_log["records"], accounts_max=1 << 14, transfers_max=1 << 14)
    checker = Counterparties(engine.export_transfers())
    assert checker.of(S)[1] == groups
    by_volume = checker.of(S, flags=BOTH | BY_VOLUME, limit=ROWS_MAX)[0]
    volumes = [volume_of(r) for r in by_volume]
    assert volumes[0] >> 64 and volumes[-1] == 0 and len(set(volumes)) < 200  # long ties
    assert any(volumes[k] == volumes[k + 1] for k in (0, 99, 4999))  # ... across these cuts
    for order in (0, BY_VOLUME):
        for limit in (1, 2, 100, 101, 5000, ROWS_MAX, ROWS_MAX + 500):  # k = 8,191 of M = 8,200
            got = check(engine, checker, S, flags=BOTH | order, limit=limit)
            assert len(got) == min(limit, ROWS_MAX)
        check(engine, checker, S, flags=DEBITS | order, limit=777)
        check(engine, checker, S, flags=CREDITS | order, limit=777)
    # M = k - 1, k and k + 1: a period that holds M groups' first records.
    stamps = select_log["records"]["timestamp"]
    for m in (40, 300):
        t_close = int(stamps[m])
        have = checker.of(S, 0, t_close)[1]
        for order in (0, BY_VOLUME):
            for limit in (have - 1, have, have + 1):
                check(engine, checker, S, 0, t_close, BOTH | order, limit=limit)
    # id_min: above every id, with a high word, and in between; under BY_VOLUME it narrows the groups.
    top = max(select_log["x"](j) for j in range(groups))
    assert top >> 64
    for id_min in (top + 1, top, 1 << 64, (2 << 64) | 5, 4000, (1 << 64) | 4000):
        for order in (0, BY_VOLUME):
            check(engine, checker, S, flags=BOTH | order, id_min=id_min, limit=50)
    assert checker.of(S, id_min=top + 1)[1] == 0 and checker.of(S, id_min=top)[1] == 1


def test_eviction_and_orphaned_posts(ledger, gpu_engine_factory):
    transfers, accounts = ledger["transfers"], ledger["accounts"]
    evicted = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(ledger["sc"], evicted)
    assert evicted.get_account_counterparties(ledger["hot"])[2] is True
    evicted.checkpoint_delta()
    assert evicted.evict_transfers(700) > 0
    resident = evicted.export_transfers()
    checker = Counterparties(resident)
    stamps = [int(t) for t in np.sort(resident["timestamp"])]
    for t_open, t_close in ((0, 0), (stamps[0] - 1, 0), (stamps[len(stamps) // 2], stamps[-5]), (1, stamps[0] - 1)):
        for a in (ledger["hot"], ledger["cold"], ABSENT):
            for flags in (BOTH, DEBITS | BY_VOLUME):
                check(evicted, checker, a, t_open, t_close, flags, evicted=True)
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
    checker = Counterparties(engine.export_transfers())
    o = min(orphans, key=lambda p: int(p["timestamp"]))  # the oldest orphan post
    d, c, ts = u128(o, "debit_account_id"), u128(o, "credit_account_id"), int(o["timestamp"])
    requests = [(d, ts - 1, ts, DEBITS, 0), (d, ts - 1, ts, BOTH | BY_VOLUME, 0), (c, ts - 1, ts, CREDITS, 0),
                (d, ts - 1, ts, CREDITS, 0), (c, ts - 1, ts, DEBITS, 0),          # the side that is not wanted
                (d, 0, ts - 1, BOTH, 0), (d, ts, ts, BOTH, 0),                    # outside the period
                (d, ts - 1, ts, DEBITS, c + 1), (d, 0, 0, BOTH, 0)]               # its group below id_min: it still matched
    verdicts = []
    for a, t_open, t_close, flags, id_min in requests:
        check(engine, checker, a, t_open, t_close, flags, id_min)
        verdicts.append(checker.of(a, t_open, t_close, flags, id_min)[2])
    assert verdicts == [True, True, True, False, False, False, False, True, True]
    row = engine.get_account_counterparties(d, ts - 1, ts, credits=False)[0][0]
    assert id_of(row) == c and flow_sums(row, "to") == (u128(o, "amount"), 0, u128(o, "amount"), 1)  # P = its own amount
    # Whether or not its group is returned.
    busy = next(p for p in ledger["sweep"] if p[0] < ts <= (p[1] or ts) and checker.of(d, p[0], p[1])[1] > 1)
    assert checker.of(d, *busy)[2] and any(id_of(checker.of(d, *busy, BOTH | order, 0, 1)[0][0]) != c for order in (0, BY_VOLUME))
    check(engine, checker, d, *busy, limit=1)
    check(engine, checker, d, *busy, flags=BOTH | BY_VOLUME, limit=1)
    assert engine.get_account_counterparties(d, *busy, out_cap_rows=0)[1:] == (checker.of(d, *busy)[1], False)


def test_restart_shuffled_log_and_the_loaded_self_record(gpu_engine_factory):
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
    order = np.random.default_rng(5).permutation(len(everything))
    engine = gpu_engine_factory(transfers_max=1 << 15)
    engine.load_accounts(accounts)
    engine.load_transfers(everything[order], np.concatenate([states, np.zeros(3, dtype=np.uint8)])[order])
    engine.set_commit_timestamp(last + 3)
    exported = engine.export_transfers()
    assert len(exported) == len(everything) and len(transfers) > 500
    checker = Counterparties(exported)
    stamps = [int(t) for t in np.sort(exported["timestamp"])]
    created = {u128(a, "id"): int(a["timestamp"]) for a in accounts}
    for t_open, t_close in ((0, 0), (stamps[len(stamps) // 3], stamps[-40]), (last, 0), (last + 1, last + 2), (0, stamps[50])):
        for a in [u128(x, "id") for x in accounts[:4]]:
            for flags in (BOTH, DEBITS, CREDITS, BOTH | BY_VOLUME):
                check(engine, checker, a, t_open, t_close, flags)
        check_identities(engine, created, S, t_open, t_close)
    own = {id_of(r): r for r in check(engine, checker, S, last, 0)}
    assert list(own) == [S] and flow_sums(own[S], "to") == flow_sums(own[S], "from")
    assert flow_sums(own[S], "to") == (2 * (1 << 64) - 4, (1 << 64) - 2, 0, 3)
    half = check(engine, checker, S, last, 0, DEBITS)[0]
    assert flow_sums(half, "from") == (0, 0, 0, 0) and flow_sums(half, "to")[3] == 3


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=["node2", "node3"])
def test_node(devices, ledger, gpu_engine_factory):
    sc, checker, transfers = ledger["sc"], ledger["checker"], ledger["transfers"]
    world = len(devices)
    single = gpu_engine_factory(transfers_max=1 << 14)
    engine = gpu_engine_factory(accounts_max=4096, transfers_max=1 << 14, pass_events_max=2048, pass_batches_max=16, devices=devices)
    assert commit_all(sc, engine, single) == ledger["replies"]
    # The hottest account's counterparties have records on more than one home shard.
    hot = ledger["hot"]
    mine = transfers[[u128(t, "debit_account_id") == hot or u128(t, "credit_account_id") == hot for t in transfers]]
    home = homes_of(np.stack([mine["id_lo"], mine["id_hi"]], axis=1), world)
    other = [u128(t, "credit_account_id") if u128(t, "debit_account_id") == hot else u128(t, "debit_account_id") for t in mine]
    assert any(len({int(h) for h, x in zip(home, other) if x == who}) >= 2 for who in set(other))
    sweep_engine(engine, ledger)
    for order in (0, BY_VOLUME):
        for t_open, t_close in ledger["sweep"][::4]:
            got = check(engine, checker, hot, t_open, t_close, BOTH | order)
            assert got.tobytes() == single.get_account_counterparties(hot, t_open, t_close, by_volume=bool(order))[0].tobytes()
    check_identities(engine, ledger["created"], hot, 0, 0)
    whole = check(engine, checker, hot)
    status, result, raw = raw_call(engine, pack_counterparty_filter(hot, limit=9), 5, rows=16)
    assert status == _lib.STATUS_OK and result == (5, 1, len(whole))
    assert raw[:5 * ROW] == whole[:5].tobytes() and raw[5 * ROW:] == b"\xAB" * (len(raw) - 5 * ROW)


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=["node2", "node3"])
def test_node_volume_rank_is_of_the_totals(devices, gpu_engine_factory):
    """Every shard holds two counterparties of its own, worth 100 and 90 there, and 60 of one counterparty
    all shards share: each shard's local top two are its own pair, the top two of the totals are the
    shared one and the smallest id among the 100s."""
    world = len(devices)
    engine = gpu_engine_factory(accounts_max=4096, transfers_max=1 << 12, pass_events_max=2048, pass_batches_max=16, devices=devices)
    S, shared = 1, 2
    n_acc = 2 + 2 * world
    assert engine.commit(128, 10**12, b"".join(pack_account(id=1 + i, ledger=1, code=1) for i in range(n_acc))) == b""
    candidates = np.array([[10**6 + k, 0] for k in range(64 * world)], dtype=np.uint64)
    home = homes_of(candidates, world)
    events = []
    for s in range(world):
        ids = [int(candidates[k][0]) for k in range(len(candidates)) if home[k] == s][:3]
        assert len(ids) == 3
        events.append(pack_transfer(id=ids[0], debit_account_id=S, credit_account_id=3 + 2 * s, amount=100, ledger=1, code=1))
        events.append(pack_transfer(id=ids[1], debit_account_id=4 + 2 * s, credit_account_id=S, amount=90, ledger=1, code=1))
        events.append(pack_transfer(id=ids[2], debit_account_id=S, credit_account_id=shared, amount=60, ledger=1, code=1))
    assert engine.commit(129, 2 * 10**12, b"".join(events)) == b""
    exported = engine.export_transfers()
    assert len(exported) == 3 * world
    assert sorted(homes_of(np.stack([exported["id_lo"], exported["id_hi"]], axis=1), world).tolist()) == sorted(list(range(world)) * 3)
    checker = Counterparties(exported)
    top = check(engine, checker, S, flags=BOTH | BY_VOLUME, limit=2)
    assert [id_of(r) for r in top] == [shared, 3] and [volume_of(r) for r in top] == [60 * world, 100]
    assert flow_sums(top[0], "to") == (60 * world, 0, 0, world)
    whole = check(engine, checker, S, flags=BOTH | BY_VOLUME)
    assert len(whole) == 1 + 2 * world
    check(engine, checker, S, limit=2)
    check(engine, checker, S, flags=CREDITS | BY_VOLUME, limit=2)


def test_read_only_and_allocation_free(ledger, gpu_engine_factory):
    """50 calls around which the allocation count, commit_timestamp, the exports and the commit-path
    counters of tbgpu_get_stats stand still; one more inside an asynchronous write-back; then the next
    commit answers as the oracle did."""
    sc, transfers, everyone = ledger["sc"], ledger["transfers"], ledger["everyone"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    twin = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, engine, twin, steps=sc.steps[:-1])
    resident = engine.export_transfers()
    checker = Counterparties(resident)
    before = (engine.commit_timestamp, engine.export_accounts().tobytes(), resident.tobytes(), engine.export_posted().tobytes())
    rng = random.Random(3)
    allocations = engine.lib.tbgpu_debug_allocations()
    stats = engine.stats()
    stamps = [int(t) for t in np.sort(resident["timestamp"])]
    marks = [0, 1, stamps[len(stamps) // 3], stamps[-5], stamps[-1] + 7]
    for _ in range(50):
        t_open = rng.choice(marks)
        t_close = rng.choice([0] + [m for m in marks if m >= t_open])
        engine.get_account_counterparties(rng.choice(everyone), t_open, t_close, by_volume=rng.random() < 0.5, limit=rng.choice((1, 9, 8191)))
    assert engine.lib.tbgpu_debug_allocations() == allocations
    after = engine.stats()
    assert all(after[k] == stats[k] for k in ("passes", "events", "transfers", "accounts", "log_used"))
    assert before == (engine.commit_timestamp, engine.export_accounts().tobytes(), engine.export_transfers().tobytes(),
                      engine.export_posted().tobytes())
    # One between an asynchronous write-back's start and its wait leaves the delta alone.
    caps = (1 << 14, 1 << 14, 1 << 14)
    engine.checkpoint_delta_async(caps)
    allocations = engine.lib.tbgpu_debug_allocations()
    check(engine, checker, ledger["hot"], stamps[len(stamps) // 3], stamps[-5], BOTH | BY_VOLUME)
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
    healthy, matched, complete = engine.get_account_counterparties(1, 10, 25)
    assert matched == 1 and complete and id_of(healthy[0]) == 2
    assert (flow_sums(healthy[0], "to"), flow_sums(healthy[0], "from")) == ((0, 100, 0, 1), (7, 0, 0, 1))
    engine.set_balances(1, 0, 0, 0, 0)
    with pytest.raises(EnginePanic):
        engine.commit(129, 30, pack_transfer(id=11, pending_id=10, flags=POST))
    with pytest.raises(EnginePanic, match="stopped"):
        engine.commit(129, 40, pack_transfer(id=13, debit_account_id=1, credit_account_id=2, amount=1, ledger=1, code=1))
    checker = Counterparties(engine.export_transfers())
    allocations = engine.lib.tbgpu_debug_allocations()
    for t_open, t_close in ((0, 0), (10, 20), (19, 24), (20, 0), (24, 25)):
        for a in (1, 2):
            want, matched, _ = checker.of(a, t_open, t_close, BOTH | BY_VOLUME)
            got, got_matched, _ = engine.get_account_counterparties(a, t_open, t_close, by_volume=True)
            assert got.tobytes() == want.tobytes() and got_matched == matched
    assert engine.lib.tbgpu_debug_allocations() == allocations


def test_invalid_input(ledger, gpu_engine_factory):
    sc, hot = ledger["sc"], ledger["hot"]
    engine = gpu_engine_factory(transfers_max=1 << 12)
    empty = engine.get_account_counterparties(hot, 0, 9)
    assert len(empty[0]) == 0 and empty[0].dtype == COUNTERPARTY_DTYPE and empty[1:] == (0, True)  # an empty engine
    commit_all(sc, engine, steps=sc.steps[:4])
    t0, t1, t2 = sc.steps[1][2], sc.steps[2][2], sc.steps[3][2]
    a = max(ledger["everyone"], key=lambda i: engine.get_account_counterparties(i, t0, t2)[1])
    valid, matched, complete = engine.get_account_counterparties(a, t0, t2)
    assert matched == len(valid) > 3 and complete
    good = dict(account_id=a, t_open=t0, t_close=t2, id_min=0, limit=50, flags=BOTH)
    bad = [dict(account_id=0), dict(account_id=MOD - 1), dict(flags=0), dict(flags=BY_VOLUME), dict(flags=BOTH | REVERSED),
           dict(flags=BOTH | 1 << 3), dict(flags=BOTH | 1 << 9), dict(flags=BOTH | 1 << 31), dict(t_open=U64_MAX), dict(t_close=U64_MAX),
           dict(t_open=U64_MAX, t_close=U64_MAX), dict(t_open=t1, t_close=t0), dict(t_open=t2, t_close=1), dict(limit=0)]
    filters = [pack_counterparty_filter(**dict(good, **kw)) for kw in bad]
    filters += [pack_counterparty_filter(**good)[:56 + k] + b"\x01" + bytes(7 - k) for k in (0, 3, 7)]  # a reserved byte
    for f in filters:
        status, result, raw = raw_call(engine, f, 64)
        assert status == _lib.STATUS_OK and result == (0, 1, 0) and raw == b"\xAB" * len(raw), f
        got, m, complete = engine.get_account_counterparties_raw(f)
        assert len(got) == 0 and m == 0 and complete
    f = pack_counterparty_filter(**good)
    for null in (("filter",), ("out",), ("result",), ("filter", "out", "result")):
        status, result, raw = raw_call(engine, f, 64, null=null)
        assert status == _lib.STATUS_INVALID and result == (77, 77, 77) and raw == b"\xAB" * len(raw)
    status, result, raw = raw_call(engine, filters[0], 64, null=("out",))  # NULL before the filter's own checks
    assert status == _lib.STATUS_INVALID
    status, result, raw = raw_call(engine, f, 64)
    assert status == _lib.STATUS_OK and result == (len(valid), 1, matched)
    assert raw[:ROW * len(valid)] == valid.tobytes() and raw[ROW * len(valid):] == b"\xAB" * (len(raw) - ROW * len(valid))
    assert engine.get_account_counterparties(a, t2, t2)[1] == 0  # an empty period is a valid one
