"""get_account_balance_extremes (include/tbgpu.h tbgpu_get_account_balance_extremes, csrc/k_extremes.h):
for the accounts a caller names, a period and a measure, the lowest and the highest value the measure
reached, when, and the measure at both ends.  Rows, `matched` and `complete` are compared byte for byte
with the checker of tests/harness/extremes.py (held to the oracle's per-event balances in
tests/test_extremes_checkers.py), and the ordered walk with the exact path, which an engine made under
TBGPU_EXTREMES_EXACT=1 takes; TBGPU_EXTREMES_SLABS caps the slabs of the walk.  No tolerances."""
import ctypes
import random

import numpy as np
import pytest

from tests.harness.balances import balances_of, u128
from tests.harness.extremes import Extremes, ids_body
from tests.harness.oracle import OracleEngine
from tests.harness.statements import request_of, sweep_pairs
from tests.harness.workload import account_id, make_scenario
from tests.test_gpu_query import SCENARIO, by_id, commit_all, posted_states
from tigerbeetle_amd import _lib
from tigerbeetle_amd._lib import EngineError
from tigerbeetle_amd import types as T
from tigerbeetle_amd.types import EXTREME_DTYPE, U64_MAX, TransferFlags, extreme_value, pack_account, pack_balance_measure, pack_transfer

pytestmark = pytest.mark.gpu

PENDING = int(TransferFlags.pending)
POST = int(TransferFlags.post_pending_transfer)
VOID = int(TransferFlags.void_pending_transfer)
MAX = 4095
ROW = 192
ABSENT = (account_id(5000), account_id(5001))
MEASURES = (T.MEASURE_CREDIT_NET_POSTED, T.MEASURE_CREDIT_AVAILABLE, T.MEASURE_DEBIT_NET_POSTED, T.MEASURE_DEBIT_AVAILABLE,
            T.MEASURE_DEBITS_PENDING, T.MEASURE_DEBITS_POSTED, T.MEASURE_CREDITS_PENDING, T.MEASURE_CREDITS_POSTED)
NET, AVAILABLE = T.MEASURE_CREDIT_NET_POSTED, T.MEASURE_CREDIT_AVAILABLE


def make(factory, monkeypatch, exact=False, slabs=None, **kw):
    """An engine whose knobs, read at tbgpu_init, force the exact path or cap the walk's slabs."""
    monkeypatch.setenv("TBGPU_EXTREMES_EXACT", "1" if exact else "0")
    if slabs is None:
        monkeypatch.delenv("TBGPU_EXTREMES_SLABS", raising=False)
    else:
        monkeypatch.setenv("TBGPU_EXTREMES_SLABS", str(slabs))
    engine = factory(**kw)
    monkeypatch.delenv("TBGPU_EXTREMES_EXACT")
    monkeypatch.delenv("TBGPU_EXTREMES_SLABS", raising=False)
    return engine


def check(engine, checker, ids, t_open, t_close, measure, evicted=False, cap=None, others=()):
    """One request: rows, matched and complete as the checker has them — and as every engine of
    `others` (the exact path, other slab counts) answers."""
    want, matched, orphan = checker.of(ids, t_open, t_close, measure, cap)
    got, got_matched, got_complete = engine.get_account_balance_extremes(ids, t_open, t_close, measure, cap)
    assert len(got) == len(want), (t_open, t_close, measure, len(got), len(want))
    if got.tobytes() != want.tobytes():
        bad = next(k for k in range(len(got)) if got[k].tobytes() != want[k].tobytes())
        assert False, (t_open, t_close, measure, bad, got[bad], want[bad])
    assert (got_matched, got_complete) == (matched, not evicted and not orphan), (t_open, t_close, measure)
    for other in others:
        rows, m, complete = other.get_account_balance_extremes(ids, t_open, t_close, measure, cap)
        assert rows.tobytes() == got.tobytes() and (m, complete) == (got_matched, got_complete), (t_open, t_close, measure)
    return got


def raw_call(engine, t_open, t_close, measure_bytes, ids, n, cap, fill=b"\xAB"):
    """The C call into a sentinel-filled buffer: (status, result, the buffer's bytes)."""
    src = ctypes.create_string_buffer(ids_body(ids), 16 * len(ids))
    m = ctypes.create_string_buffer(measure_bytes, 8)
    out = ctypes.create_string_buffer(fill * (ROW * max(len(ids), 1)), ROW * max(len(ids), 1))
    res = _lib.tbgpu_query_result(count=77, complete=77, matched=77)
    status = engine.lib.tbgpu_get_account_balance_extremes(engine.h, t_open, t_close, m, src, n, out, cap, ctypes.byref(res))
    return status, (res.count, res.complete, res.matched), out.raw


def statement_value(row, when, measure):
    cols = ("debits_pending", "debits_posted", "credits_pending", "credits_posted")
    return sum(k * u128(row, when + "_" + c) for k, c in zip(measure, cols))


@pytest.fixture(scope="module")
def ledger():
    """test_gpu_query.py's scenario, the oracle that committed all of it, its exports and the checker
    over them (never changed)."""
    sc = make_scenario(2025, **SCENARIO)
    oracle = OracleEngine(4096, 1 << 15)
    replies = commit_all(sc, oracle)
    transfers, accounts = oracle.export_transfers(), oracle.export_accounts()
    return dict(sc=sc, replies=replies, transfers=transfers, accounts=accounts, commit_timestamp=oracle.commit_timestamp,
                posted=oracle.export_posted(), checker=Extremes(transfers, accounts, oracle.commit_timestamp),
                ids=request_of(accounts, ABSENT), pairs=sweep_pairs(sc.steps, transfers, oracle.commit_timestamp))


def test_single_engine_sweep(ledger, gpu_engine_factory, monkeypatch):
    """Every period of the sweep — t_open == t_close, t_close == 0, records above t_end, a period newer
    than every record, accounts created after t_end — under every measure macro in turn, the walk
    against the checker and every third also against the exact path; opening and closing are the
    statements call's fields recombined."""
    sc, checker, ids = ledger["sc"], ledger["checker"], ledger["ids"]
    engine = make(gpu_engine_factory, monkeypatch, transfers_max=1 << 14)
    exact = make(gpu_engine_factory, monkeypatch, exact=True, transfers_max=1 << 14)
    assert commit_all(sc, engine, exact) == ledger["replies"]
    now = ledger["commit_timestamp"]
    answers = {}
    for k, pair in enumerate(ledger["pairs"]):
        measure = MEASURES[k % len(MEASURES)]
        answers[pair] = check(engine, checker, ids, *pair, measure, others=(exact,) if k % 3 == 0 else ())
    assert len({rows.tobytes() for rows in answers.values()}) > 20
    whole = check(engine, checker, ids, 0, 0, NET, others=(exact,))
    assert len(whole) == len(ids) - 4 and all(extreme_value(r, "opening") == 0 and int(r["t_end"]) == now for r in whole)
    assert any(extreme_value(r, "low") < 0 for r in whole) and any(extreme_value(r, "high") > 0 for r in whole)
    assert any(int(r["t_low"]) not in (0, now) for r in whole) and sum(int(r["records"]) for r in whole[:len(ids) - 10]) > 1000
    assert len(answers[(now + 1, 0)]) == 0 and 0 < len(answers[(0, sc.steps[0][2])]) < len(whole)
    # A period newer than every record, and an empty one: the opening is everything.
    for t_open, t_close in ((now, now + 5), (sc.steps[7][2], sc.steps[7][2])):
        for r in check(engine, checker, ids, t_open, t_close, AVAILABLE, others=(exact,)):
            if t_open == now:
                assert int(r["records"]) == 0
            if int(r["records"]) == 0:
                assert r["opening_w0"] == r["closing_w0"] == r["low_w0"] == r["high_w0"] and int(r["t_low"]) == int(r["t_high"]) == t_open
    # t_close == 0 is t_close == commit_timestamp.
    for t_open in (0, 1, sc.steps[5][2], now):
        assert engine.get_account_balance_extremes(ids, t_open, 0, NET)[0].tobytes() == check(engine, checker, ids, t_open, now, NET).tobytes()
    # A single posted column only grows: its low is its opening, its high its closing.
    for measure in (T.MEASURE_DEBITS_POSTED, T.MEASURE_CREDITS_POSTED):
        for r in check(engine, checker, ids, sc.steps[3][2], sc.steps[14][2], measure):
            assert extreme_value(r, "low") == extreme_value(r, "opening") and extreme_value(r, "high") == extreme_value(r, "closing")
            assert int(r["t_low"]) == sc.steps[3][2]
    # Against the statements call: both ends are its fields recombined, for every measure.
    stamps = np.sort(ledger["transfers"]["timestamp"])
    for t_open, t_end in ((sc.steps[2][2], sc.steps[9][2]), (int(stamps[300]), int(stamps[1500])), (0, sc.steps[4][2])):
        held = engine.get_account_statements(ids, t_open, t_end)[0]
        for measure in MEASURES:
            rows = check(engine, checker, ids, t_open, t_end, measure)
            assert len(rows) == len(held) > 0
            for r, h in zip(rows, held):
                assert u128(r, "id") == u128(h, "id")
                assert extreme_value(r, "opening") == statement_value(h, "opening", measure)
                assert extreme_value(r, "closing") == statement_value(h, "closing", measure)
    # out_cap_rows cuts the answer in request order, and nothing past count rows is written.
    pair = ledger["pairs"][len(ledger["pairs"]) // 2]
    full = check(engine, checker, ids, *pair, NET)
    matched = len(full)
    assert matched > 8
    for cap in (0, 1, matched - 1, matched, matched + 3):
        check(engine, checker, ids, *pair, NET, cap=cap, others=(exact,))
        status, (count, complete, m), raw = raw_call(engine, pair[0], pair[1], pack_balance_measure(NET), ids, len(ids), cap)
        assert status == _lib.STATUS_OK and (count, complete, m) == (min(cap, matched), 1, matched)
        assert raw[:ROW * count] == full[:count].tobytes() and raw[ROW * count:] == b"\xAB" * (ROW * (len(ids) - count))


def in_place(engine, bodies, stamps, counts):
    """Prepares committed in place (tbgpu_log_window): log position = event index."""
    total = sum(counts)
    window = engine.log_window(total)
    engine.to_device(window, np.frombuffer(b"".join(bodies), dtype=np.uint8))
    res, rb = engine.alloc(total * 8), engine.alloc(8)
    engine.commit_device_async(129, stamps, counts, window, res, rb)
    return res, rb


def test_wave_tile_and_border_extremes(gpu_engine_factory, monkeypatch):
    """One prepare of 600 events committed in place, so log position = event index and timestamp =
    first + position.  A sits in all 64 lanes of the wave at 64..127 with alternating sides and amounts
    that put its low and its high mid-wave; B's high is on lane 63 and its low on lane 0 of the next
    wave (191 / 192), C's on the tile border (511 / 512), with failing events that name them on either
    side; D holds a pending transfer that is partly posted and another that is voided; E's steps are
    2^127 and 2^64 - 1, so sums carry; F is debited first, so its net goes negative, and reaches its
    high three times, the first counts; G is only credited, so its opening is its low."""
    n_acc, n = 16, 600
    A, B, C, D, E, F, G = (account_id(i) for i in range(7))
    fill = [account_id(i) for i in range(8, n_acc)]
    engine = make(gpu_engine_factory, monkeypatch, transfers_max=1 << 12)
    exact = make(gpu_engine_factory, monkeypatch, exact=True, transfers_max=1 << 12)
    oracle = OracleEngine(64, 1 << 12)
    accounts = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(n_acc))
    assert engine.commit(128, 10**12, accounts) == exact.commit(128, 10**12, accounts) == oracle.commit(128, 10**12, accounts) == b""
    rng = random.Random(5)
    events = []
    for i in range(n):
        dr = rng.choice(fill)
        cr = rng.choice([a for a in fill if a != dr])
        events.append(dict(id=1000 + i, debit_account_id=dr, credit_account_id=cr, amount=1 + i, ledger=1, code=1))

    def plant(i, debit, credit, amount, **kw):
        events[i].update(debit_account_id=debit, credit_account_id=credit, amount=amount, **kw)

    for i in range(64, 128):  # A in every lane, sides alternating: down for 24 lanes, up for 24, down again
        lane = i - 64
        down, up = ((250, 60), (50, 700), (900, 10))[lane // 24 if lane < 48 else 2]
        plant(i, A, fill[lane % 8], down + lane) if lane % 2 == 0 else plant(i, fill[lane % 8], A, up + lane)
    plant(20, fill[0], A, 70)
    plant(189, fill[1], B, 300), plant(191, fill[1], B, 1000), plant(192, B, fill[2], 5000), plant(194, fill[2], B, 100)
    plant(190, B, fill[1], 9999, id=0), plant(193, fill[1], B, 9999, id=1000 + 191)  # both fail
    plant(509, fill[3], C, 10), plant(511, fill[3], C, 2000), plant(512, C, fill[4], 6000), plant(514, fill[4], C, 50)
    plant(510, C, fill[3], 8888, id=0), plant(513, fill[3], C, 8888, id=1000 + 511)  # both fail
    plant(30, D, fill[5], 900, flags=PENDING), plant(31, fill[5], D, 400, flags=PENDING)
    events[250].update(debit_account_id=0, credit_account_id=0, amount=350, pending_id=1030, flags=POST)
    events[260].update(debit_account_id=0, credit_account_id=0, amount=0, pending_id=1031, flags=VOID)
    plant(40, fill[6], E, 1 << 127), plant(41, E, fill[6], (1 << 64) - 1), plant(300, E, fill[6], (1 << 64) - 1)
    plant(301, fill[6], E, (1 << 64) - 1), plant(302, E, fill[7], 1 << 100)
    plant(50, F, fill[7], 500), plant(51, fill[7], F, 505), plant(320, F, fill[7], 5), plant(321, fill[7], F, 5), plant(322, F, fill[0], 5)
    plant(323, fill[0], F, 5)
    plant(60, fill[1], G, 11), plant(330, fill[1], G, 12), plant(599, fill[1], G, 13)
    body = b"".join(pack_transfer(**ev) for ev in events)
    stamp = 10**12 + 10**6
    expected = oracle.commit(129, stamp, body)
    assert np.frombuffer(expected, dtype=np.uint32)[0::2].tolist() == [190, 193, 510, 513]  # exactly the planted events failed
    assert exact.commit(129, stamp, body) == expected
    res, rb = in_place(engine, [body], [stamp], [n])
    first = stamp - n + 1
    at = lambda pos: first + pos
    last = at(n - 1)
    ids = [A, B, C, D, E, F, G] + fill + [A, ABSENT[0], 0]
    exported = oracle.export_transfers()
    checker = Extremes(exported, oracle.export_accounts(), last)
    edges = [0, 19, 20, 29, 63, 64, 100, 127, 128, 190, 191, 192, 193, 260, 322, 510, 511, 512, 513, 599]
    pairs = [(at(a), at(b)) for a, b in zip(edges, edges[1:])] + [(at(a), at(b)) for a, b in zip(edges, edges[3:])]
    pairs += [(0, 0), (0, at(127)), (at(63), 0), (at(63), at(127)), (at(64), at(126)), (at(190), at(192)), (at(191), at(512)), (last, last + 9)]
    for k, (t_open, t_close) in enumerate(pairs):  # the first call drains the asynchronous commit itself
        for measure in (NET, MEASURES[k % len(MEASURES)]):
            got = check(engine, checker, ids, t_open, t_close, measure, others=(exact,) if k % 4 == 0 else ())
            assert got[0].tobytes() == got[len(ids) - 3].tobytes()
    row = lambda account, t_open, t_close, measure=NET: check(engine, checker, [account], t_open, t_close, measure, others=(exact,))[0]
    # Non-vacuity, on the answers the checker confirmed.
    r = row(A, at(63), at(127))
    assert int(r["records"]) == 64 and at(64) < int(r["t_low"]) < at(127) and at(64) < int(r["t_high"]) < at(127)
    assert int(r["t_low"]) != int(r["t_high"]) and extreme_value(r, "low") < extreme_value(r, "opening") < extreme_value(r, "high")
    assert (int(r["t_low"]), int(r["t_high"])) == (at(64 + 22), at(64 + 47))
    r = row(B, at(100), at(400))
    assert (int(r["t_high"]), int(r["t_low"]), int(r["records"])) == (at(191), at(192), 4)
    r = row(C, at(100), last)
    assert (int(r["t_high"]), int(r["t_low"]), int(r["records"])) == (at(511), at(512), 4)
    r = row(D, 0, 0, T.MEASURE_DEBITS_PENDING)
    assert (extreme_value(r, "high"), int(r["t_high"]), extreme_value(r, "closing")) == (900, at(30), 0)
    r = row(D, at(30), 0, (1, 1, 0, 0))  # a post is one step: 900 held becomes 350 posted, never 0 and never 1,250 between
    assert (extreme_value(r, "opening"), extreme_value(r, "high"), int(r["t_high"])) == (900, 900, at(30))
    assert (extreme_value(r, "low"), int(r["t_low"]), extreme_value(r, "closing")) == (350, at(250), 350)
    r = row(D, 0, 0, T.MEASURE_DEBIT_AVAILABLE)  # the hold on the credit side is placed at 31 and voided at 260
    assert (extreme_value(r, "low"), int(r["t_low"]), extreme_value(r, "high"), int(r["t_high"])) == (-400, at(31), 350, at(260))
    r = row(E, 0, 0)
    assert extreme_value(r, "high") == 1 << 127 and extreme_value(r, "low") == 0 and int(r["t_high"]) == at(40)
    assert extreme_value(r, "closing") == (1 << 127) - ((1 << 64) - 1) - (1 << 100) and r["closing_w1"] != 0
    r = row(E, at(41), 0, T.MEASURE_DEBIT_NET_POSTED)
    assert extreme_value(r, "opening") < -(1 << 126) and r["opening_w2"] == U64_MAX and int(r["t_high"]) == at(302)
    r = row(F, 0, 0)
    assert (extreme_value(r, "low"), int(r["t_low"]), extreme_value(r, "high"), int(r["t_high"])) == (-500, at(50), 5, at(51))
    assert extreme_value(r, "closing") == 5 and int(r["records"]) == 6  # 5 again at 321 and 323: the first timestamp wins
    r = row(G, at(59), 0)
    assert (extreme_value(r, "low"), int(r["t_low"]), extreme_value(r, "high"), int(r["t_high"])) == (0, at(59), 36, last)
    assert engine.export_accounts().tobytes() == oracle.export_accounts().tobytes()
    assert engine.export_transfers().tobytes() == exported.tobytes()
    engine.free(res)
    engine.free(rb)


def test_three_spans_under_one_two_and_three_slabs(gpu_engine_factory, monkeypatch):
    """Three prepares of 8,190 events committed in place: three spans of a workgroup's 8,192 records.
    A's extremes lie in the middle span, or on the positions either side of a span border (8,191 /
    8,192 and 16,383 / 16,384), depending on the period.  The walk is cut into 1, 2 and 3 slabs
    (TBGPU_EXTREMES_SLABS) and left to itself: the bytes are equal, and the checker's."""
    n_acc, per = 8, 8190
    A = account_id(0)
    others = [account_id(i) for i in range(1, n_acc)]
    engines = [make(gpu_engine_factory, monkeypatch, slabs=s, transfers_max=1 << 15) for s in (None, 1, 2, 3)]
    oracle = OracleEngine(64, 1 << 15)
    accounts = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(n_acc))
    for e in engines + [oracle]:
        assert e.commit(128, 10**12, accounts) == b""
    rng = random.Random(23)
    events = []
    for i in range(3 * per):
        dr = rng.choice(others)
        cr = rng.choice([a for a in others if a != dr])
        ev = dict(id=10**6 + i, debit_account_id=dr, credit_account_id=cr, amount=1 + i % 97, ledger=1, code=1)
        if i % 5 == 0:  # A moves a little, up and down
            ev.update(debit_account_id=A, credit_account_id=cr) if (i // 5) % 2 else ev.update(debit_account_id=dr, credit_account_id=A)
        events.append(ev)
    for i, debit, amount in ((8191, False, 10**6), (8192, True, 3 * 10**6), (16383, True, 10**7), (16384, False, 3 * 10**7),
                             (12000, True, 3 * 10**9), (12001, False, 6 * 10**9)):
        events[i].update(debit_account_id=A if debit else others[i % 7], credit_account_id=others[i % 7] if debit else A, amount=amount)
    bodies = [b"".join(pack_transfer(**ev) for ev in events[k * per:(k + 1) * per]) for k in range(3)]
    stamps = [10**12 + 10**6 + per * k for k in range(3)]
    for ts, body in zip(stamps, bodies):
        assert oracle.commit(129, ts, body) == b""
    held = [in_place(e, bodies, stamps, [per] * 3) for e in engines]
    first = stamps[0] - per + 1
    at = lambda pos: first + pos
    last = at(3 * per - 1)
    checker = Extremes(oracle.export_transfers(), oracle.export_accounts(), last)
    ids = [A] + others + [A]
    where = {}
    for t_open, t_close in ((0, 0), (at(8189), at(8194)), (at(16380), at(16386)), (at(8000), at(8400)), (at(8191), at(8400)), (at(16000), at(16500)), (at(16383), at(16390)),
                            (at(8190), at(8192)), (at(6000), at(18000)), (at(12001), 0), (0, at(8191)), (at(16384), 0)):
        for measure in (NET, T.MEASURE_DEBIT_NET_POSTED, T.MEASURE_CREDITS_POSTED):
            got = check(engines[0], checker, ids, t_open, t_close, measure, others=engines[1:])
            where[(t_open, t_close, measure)] = (int(got[0]["t_low"]), int(got[0]["t_high"]))
    # (t_low, t_high) of A: either side of each span border, and in the middle span (A's small moves
    # in between are far below the planted ones, but they decide among near-equal values, so only the
    # planted margins are asserted).
    assert where[(at(8189), at(8194), NET)] == (at(8192), at(8191))
    assert where[(at(16380), at(16386), NET)] == (at(16383), at(16384))
    assert where[(at(6000), at(18000), NET)][0] == at(12000) and where[(0, 0, NET)][0] == at(12000)
    assert where[(at(6000), at(18000), T.MEASURE_DEBIT_NET_POSTED)][1] == at(12000)
    for e, (res, rb) in zip(engines, held):
        assert e.export_accounts().tobytes() == oracle.export_accounts().tobytes()
        e.free(res)
        e.free(rb)


def test_more_active_accounts_than_lds_bins(gpu_engine_factory, monkeypatch):
    """4,200 accounts; two 4,000-transfer prepares in which 600 accounts debit again and again, more
    than a workgroup's claimed LDS bins, from every wave of one slab: an account without a bin is
    composed in its cell of the slab in HBM.  Amounts of 2^63 + j carry out of the low word.  Requests
    of exactly 4,095 ids, with repeated, absent and reserved ones; one more is invalid and writes
    nothing."""
    n_acc, hot = 4200, 600
    engine = make(gpu_engine_factory, monkeypatch, accounts_max=1 << 13, transfers_max=1 << 14)
    two = make(gpu_engine_factory, monkeypatch, slabs=1, accounts_max=1 << 13, transfers_max=1 << 14)
    body = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(n_acc))
    assert engine.commit(128, 10**12, body) == two.commit(128, 10**12, body) == b""
    for k in range(2):
        body = b"".join(pack_transfer(id=10**6 + 4000 * k + j, debit_account_id=account_id((7 * j) % hot),
                                      credit_account_id=account_id(hot + (j * 13 + k) % (n_acc - hot)), amount=(1 << 63) + j, ledger=1,
                                      code=1, flags=PENDING if (j // hot) % 3 == 0 else 0) for j in range(4000))
        assert engine.commit(129, 2 * 10**12 + k * 10**6, body) == two.commit(129, 2 * 10**12 + k * 10**6, body) == b""
    transfers = engine.export_transfers()
    assert len(transfers) == 8000
    checker = Extremes(transfers, engine.export_accounts(), engine.commit_timestamp)
    stamps = np.sort(transfers["timestamp"])
    inside_first, inside_second = int(stamps[1700]), int(stamps[6100])
    hot_ids = [account_id(i) for i in range(hot - 1, -1, -1)]
    mixed = [account_id(i) for i in range(MAX - 40)] + [0, (1 << 128) - 1, ABSENT[0], ABSENT[1]] + hot_ids[:36]
    random.Random(9).shuffle(mixed)
    assert len(mixed) == MAX
    for ids in (hot_ids, mixed):
        for t_open, t_close in ((0, 0), (10**12, inside_first), (inside_first, inside_second), (inside_second, 0)):
            for measure in (T.MEASURE_DEBIT_AVAILABLE, NET):
                got = check(engine, checker, ids, t_open, t_close, measure, others=(two,))
                assert len(got) == (len(ids) if ids is hot_ids else MAX - 4)
        got = check(engine, checker, hot_ids, inside_first, inside_second, T.MEASURE_DEBITS_POSTED)
        assert (got["records"] >= 2).all() and (got["high_w0"] != got["low_w0"]).sum() == hot and (got["high_w1"] > 0).all()
    status, result, raw = raw_call(engine, 0, 0, pack_balance_measure(NET), mixed + [account_id(MAX)], MAX + 1, 8)
    assert status == _lib.STATUS_INVALID and result == (77, 77, 77) and raw == b"\xAB" * len(raw)


def test_eviction_and_orphaned_posts(ledger, gpu_engine_factory, monkeypatch):
    """After tbgpu_evict_transfers of an old prefix `complete` is 0 and the rows are the checker's over
    the resident export, an orphan post among them (P = its own amount), on both paths."""
    ids = ledger["ids"]
    evicted = make(gpu_engine_factory, monkeypatch, transfers_max=1 << 14)
    exact = make(gpu_engine_factory, monkeypatch, exact=True, transfers_max=1 << 14)
    commit_all(ledger["sc"], evicted, exact)
    for e in (evicted, exact):
        e.checkpoint_delta()
        assert e.evict_transfers(700) > 0
    resident = evicted.export_transfers()
    checker = Extremes(resident, evicted.export_accounts(), evicted.commit_timestamp)
    stamps = np.sort(resident["timestamp"])
    assert checker.of(ids, int(stamps[0]), 0, AVAILABLE)[2]  # an orphan post is resident
    third, half = int(stamps[len(stamps) // 3]), int(stamps[len(stamps) // 2])
    for t_open, t_close in ((0, 0), (int(stamps[0]) - 1, third), (int(stamps[0]), int(stamps[-1])), (half, 0), (third, half)):
        for measure in (AVAILABLE, T.MEASURE_DEBITS_PENDING):
            got = check(evicted, checker, ids, t_open, t_close, measure, evicted=True)
            rows, m, complete = exact.get_account_balance_extremes(ids, t_open, t_close, measure)
            assert rows.tobytes() == got.tobytes() and m == len(got) and not complete


CHAIN_FREE = dict(n_accounts=8, n_transfer_batches=4, batch_len=(100, 200), p_linked=0, p_limit=0, p_balancing=0,
                  p_pending=0.3, p_post_void=0.25)


def test_anchor_setup_action(gpu_engine_factory, monkeypatch):
    """tbgpu_test_set_balances between two runs of commits: the answers are anchored at the engine's
    current balances."""
    sc = make_scenario(17, **CHAIN_FREE)
    half = len(sc.steps) - 2
    big = [(1 << 100) + 5, (1 << 64) + 1, (1 << 90) + 9, (1 << 64) - 1]
    oracle = OracleEngine(64, 1 << 12)
    engine = make(gpu_engine_factory, monkeypatch, transfers_max=1 << 12)
    exact = make(gpu_engine_factory, monkeypatch, exact=True, transfers_max=1 << 12)
    commit_all(sc, oracle, engine, exact, steps=sc.steps[:half])
    ids = request_of(oracle.export_accounts(), ABSENT)
    for i, a in enumerate(oracle.export_accounts()):
        for e in (oracle, engine, exact):
            e.set_balances(u128(a, "id"), *[b + i for b in big])
    commit_all(sc, oracle, engine, exact, steps=sc.steps[half:])
    checker = Extremes(engine.export_transfers(), engine.export_accounts(), engine.commit_timestamp)
    assert engine.export_accounts().tobytes() == oracle.export_accounts().tobytes()
    for k, (lo, hi) in enumerate(zip(sc.steps, sc.steps[1:])):
        check(engine, checker, ids, lo[2], hi[2], MEASURES[k % len(MEASURES)], others=(exact,))
        check(engine, checker, ids, lo[2] - 3, hi[2] - 3, AVAILABLE, others=(exact,))
    rows = check(engine, checker, ids, sc.steps[half - 1][2], 0, T.MEASURE_DEBITS_PENDING, others=(exact,))
    assert all(r["opening_w1"] >> 36 for r in rows)  # 2^100 and more, as set
    check(engine, checker, ids, 0, 0, NET, others=(exact,))


def test_restart_and_unordered_log(gpu_engine_factory, monkeypatch):
    """The accounts loaded (tbgpu_load_accounts), the newer half committed, then the older half loaded
    shuffled (tbgpu_load_transfers): older timestamps sit behind newer ones in the log, the walk finds
    its order broken and the call answers by the exact path — the checker's bytes still."""
    kw = dict(n_accounts=8, n_transfer_batches=20, batch_len=(100, 300), p_pending=0.3, p_dup=0.05, p_linked=0.05,
              p_limit=0.0, p_balancing=0.0, p_invalid=0.05, id_space=1 << 40)
    sa = make_scenario(31, p_post_void=0.25, **kw)
    last = sa.steps[-1][2]
    sb = make_scenario(32, p_post_void=0.25, start_ts=last + 10**9, **kw)
    acct_steps = [s for s in sa.steps if s[1] == 128]
    a_steps = [s for s in sa.steps if s[1] == 129]
    b_steps = [s for s in sb.steps if s[1] == 129]
    oracle = OracleEngine(64, 1 << 15)
    engine1 = make(gpu_engine_factory, monkeypatch, transfers_max=1 << 15)
    engine2 = make(gpu_engine_factory, monkeypatch, transfers_max=1 << 15)
    commit_all(sa, oracle, engine1, steps=acct_steps + a_steps)
    half_a = engine1.export_transfers()
    states = posted_states(half_a, engine1.export_posted())
    at_restart = {u128(a, "id"): balances_of(a) for a in oracle.export_accounts()}
    engine2.load_accounts(engine1.export_accounts())
    engine2.set_commit_timestamp(last)
    ids = request_of(oracle.export_accounts(), ABSENT)
    # Restarted from the balances alone, an empty log: the loaded balances held for the whole period.
    loaded = Extremes(engine2.export_transfers(), engine2.export_accounts(), last)
    rows = check(engine2, loaded, ids, 5, 0, T.MEASURE_CREDITS_POSTED)
    assert len(rows) == len(ids) - 4
    assert all(extreme_value(r, "low") == extreme_value(r, "high") == at_restart[u128(r, "id")][3] and int(r["records"]) == 0 for r in rows)
    commit_all(sb, oracle, engine2, steps=b_steps)
    # Ordered so far: the period after the restart is the walk's, anchored at what was loaded.
    check(engine2, Extremes(engine2.export_transfers(), engine2.export_accounts(), engine2.commit_timestamp), ids, last, 0, NET)
    order = np.random.default_rng(5).permutation(len(half_a))
    engine2.load_transfers(half_a[order], states[order])
    transfers = oracle.export_transfers()
    assert engine2.export_transfers().tobytes() == transfers.tobytes()
    assert len(half_a) > 500 and len(transfers) - len(half_a) > 500
    checker = Extremes(engine2.export_transfers(), engine2.export_accounts(), engine2.commit_timestamp)
    stamps = np.sort(transfers["timestamp"])
    created = sorted(int(a["timestamp"]) for a in oracle.export_accounts())
    marks = [0, created[0] - 1, created[0], created[-1], int(stamps[0]), int(stamps[len(half_a) // 2]), int(half_a["timestamp"].max()),
             last, last + 1, int(stamps[len(half_a) + 50]), int(stamps[-1]), 0]
    lengths = set()
    for k, (t_open, t_close) in enumerate(list(zip(marks, marks[1:])) + [(int(stamps[200]), int(stamps[-200]))]):
        lengths.add(len(check(engine2, checker, ids, t_open, t_close, MEASURES[k % 4])))
    assert 0 in lengths and len(lengths) >= 3  # accounts loaded with a timestamp above t_end are skipped


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=["node2", "node3"])
def test_node(devices, ledger, gpu_engine_factory, monkeypatch):
    """A node's shards interleave in time: it answers by the exact path, with the single engine's bytes."""
    sc, checker, ids = ledger["sc"], ledger["checker"], ledger["ids"]
    single = make(gpu_engine_factory, monkeypatch, transfers_max=1 << 14)
    engine = make(gpu_engine_factory, monkeypatch, accounts_max=4096, transfers_max=1 << 14, pass_events_max=2048, pass_batches_max=16,
                  devices=devices)
    assert commit_all(sc, engine, single) == ledger["replies"]
    pairs = ledger["pairs"]
    for k, pair in enumerate(pairs[::5] + [(0, 0)]):
        check(single, checker, ids, *pair, MEASURES[k % len(MEASURES)], others=(engine,))
    pair = pairs[len(pairs) // 2]
    for cap in (0, 3, len(ids)):
        check(engine, checker, ids, *pair, AVAILABLE, cap=cap)
    status, result, raw = raw_call(engine, pair[0], pair[1], pack_balance_measure(NET), ids, len(ids), 3)
    assert status == _lib.STATUS_OK and result[0] == 3 and raw[3 * ROW:] == b"\xAB" * (len(raw) - 3 * ROW)


def test_read_only_and_allocation_free(ledger, gpu_engine_factory, monkeypatch):
    """50 calls around which the allocation count, commit_timestamp, the exports and the commit-path
    counters of tbgpu_get_stats stand still; one more inside an asynchronous write-back; then the
    next commit answers as the oracle did."""
    sc, transfers, ids = ledger["sc"], ledger["transfers"], ledger["ids"]
    engine = make(gpu_engine_factory, monkeypatch, transfers_max=1 << 14)
    twin = make(gpu_engine_factory, monkeypatch, exact=True, transfers_max=1 << 14)
    commit_all(sc, engine, twin, steps=sc.steps[:-1])
    resident = engine.export_transfers()
    checker = Extremes(resident, engine.export_accounts(), engine.commit_timestamp)
    before = (engine.commit_timestamp, engine.export_accounts().tobytes(), resident.tobytes(), engine.export_posted().tobytes())
    rng = random.Random(3)
    allocations = [e.lib.tbgpu_debug_allocations() for e in (engine, twin)]
    stats = engine.stats()
    stamps = np.sort(resident["timestamp"])
    marks = (0, 1, int(stamps[len(stamps) // 3]), int(stamps[-5]), int(stamps[-1]) + 7)
    for k in range(50):
        t_open = rng.choice(marks)
        t_close = rng.choice([0] + [m for m in marks if m >= t_open])
        (twin if k % 10 == 9 else engine).get_account_balance_extremes(rng.sample(ids, rng.choice((1, 5, len(ids)))), t_open, t_close,
                                                                         rng.choice(MEASURES))
    assert [e.lib.tbgpu_debug_allocations() for e in (engine, twin)] == allocations
    after = engine.stats()
    assert all(after[k] == stats[k] for k in ("passes", "events", "transfers", "accounts", "log_used"))
    assert before == (engine.commit_timestamp, engine.export_accounts().tobytes(), engine.export_transfers().tobytes(),
                      engine.export_posted().tobytes())
    # One between an asynchronous write-back's start and its wait leaves the delta alone.
    caps = (1 << 14, 1 << 14, 1 << 14)
    engine.checkpoint_delta_async(caps)
    count = engine.lib.tbgpu_debug_allocations()
    check(engine, checker, ids, int(stamps[len(stamps) // 3]), int(stamps[-5]), AVAILABLE)
    assert engine.lib.tbgpu_debug_allocations() == count
    delta = engine.checkpoint_delta_wait()
    sync = twin.checkpoint_delta(caps)
    assert len(delta.transfers) == len(resident)
    assert delta.transfers.tobytes() == sync.transfers.tobytes() and delta.posted.tobytes() == sync.posted.tobytes()
    assert by_id(delta.accounts) == by_id(sync.accounts) and delta.created_after == sync.created_after
    _, op, ts, batch = sc.steps[-1]
    assert engine.commit(op, ts, b"".join(batch)) == ledger["replies"][-1]
    assert engine.export_transfers().tobytes() == transfers.tobytes()
    assert engine.export_accounts().tobytes() == ledger["accounts"].tobytes()


def test_invalid_input(ledger, gpu_engine_factory, monkeypatch):
    sc, ids = ledger["sc"], ledger["ids"]
    engine = make(gpu_engine_factory, monkeypatch, transfers_max=1 << 12)
    for t_close in (0, 5):  # an empty engine: commit_timestamp is 0, nothing existed at 5
        empty = engine.get_account_balance_extremes(ids, 0, t_close, NET)
        assert len(empty[0]) == 0 and empty[0].dtype == EXTREME_DTYPE and empty[1:] == (0, True)
    commit_all(sc, engine, steps=sc.steps[:4])
    now = engine.commit_timestamp
    t_open, t_close = sc.steps[1][2], sc.steps[3][2]
    valid, matched, complete = engine.get_account_balance_extremes(ids, t_open, t_close, NET)
    assert matched == len(valid) == len(ids) - 4 and complete and (valid["records"] > 0).any()
    good = pack_balance_measure(NET)
    # Invalid periods are answered OK with zeros and write nothing.
    for o, c in ((U64_MAX, 0), (0, U64_MAX), (U64_MAX, U64_MAX), (t_close, t_open), (t_close + 1, t_close), (now + 1, 0)):
        got, m, complete = engine.get_account_balance_extremes(ids, o, c, NET)
        assert len(got) == 0 and m == 0 and complete
        status, result, raw = raw_call(engine, o, c, good, ids, len(ids), len(ids))
        assert status == _lib.STATUS_OK and result == (0, 1, 0) and raw == b"\xAB" * len(raw)
    assert len(engine.get_account_balance_extremes(ids, now, 0, NET)[0]) == len(valid)  # an empty period is a period
    # An invalid measure is a status and writes nothing: a coefficient outside {-1, 0, +1}, no column, a reserved byte.
    for bad in (pack_balance_measure((2, 0, 0, 0)), pack_balance_measure((0, -2, 0, 1)), pack_balance_measure((0, 0, 127, 0)),
                pack_balance_measure((0, 0, 0, -128)), pack_balance_measure((0, 0, 0, 0)), pack_balance_measure(NET, b"\0\0\0\1"),
                pack_balance_measure(NET, b"\1\0\0\0")):
        status, result, raw = raw_call(engine, t_open, t_close, bad, ids, len(ids), len(ids))
        assert status == _lib.STATUS_INVALID and result == (77, 77, 77) and raw == b"\xAB" * len(raw), bad
        with pytest.raises(EngineError):
            engine.get_account_balance_extremes_raw(ids_body(ids), t_open, t_close, bad)
    fn = engine.lib.tbgpu_get_account_balance_extremes
    src = ctypes.create_string_buffer(ids_body(ids), 16 * len(ids))
    m = ctypes.create_string_buffer(good, 8)
    sentinel = b"\xAB" * (ROW * len(ids))
    out = ctypes.create_string_buffer(sentinel, len(sentinel))
    res = _lib.tbgpu_query_result(count=77, complete=77, matched=77)
    untouched = lambda: out.raw == sentinel and (res.count, res.complete, res.matched) == (77, 77, 77)
    assert fn(engine.h, t_open, t_close, m, src, 0, out, len(ids), ctypes.byref(res)) == _lib.STATUS_OK and untouched()
    assert fn(engine.h, t_open, t_close, None, None, 0, None, 0, None) == _lib.STATUS_OK
    assert fn(engine.h, t_open, t_close, None, src, len(ids), out, len(ids), ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, t_open, t_close, m, None, len(ids), out, len(ids), ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, t_open, t_close, m, src, len(ids), None, len(ids), ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, t_open, t_close, m, src, len(ids), out, len(ids), None) == _lib.STATUS_INVALID and out.raw == sentinel
    assert fn(engine.h, t_open, t_close, m, src, MAX + 1, out, len(ids), ctypes.byref(res)) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, t_open, t_close, m, src, len(ids), out, len(ids), ctypes.byref(res)) == _lib.STATUS_OK
    assert res.count == len(valid) and out.raw[:ROW * len(valid)] == valid.tobytes()
