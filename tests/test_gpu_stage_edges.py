"""Edges of kernel 1's tile stage and of tb_resolve_lean's per-thread rows, against the oracle byte
for byte (replies, accounts, transfers, the posted groove, commit_timestamp).

The stage issues a tile's eight 16-B loads per thread from chunk indices clamped into the tile, looks
the lanes' batches up while they are in flight, and commits them to LDS predicated on the event count
(csrc/pass.h tb_stage_issue / tb_stage_commit).  What can go wrong is an LDS row or lane taken from a
neighbour, a clamped lane's value written, or a write past the tile's events; so the calls here end
inside a wave, on a wave edge and on a tile edge, their prepares are cut inside a wave and on a tile
edge, every event has its own amount (a swapped row changes a balance), failing events sit at lane 0
and lane 63 of a wave and at the first and last event of the tile and of the call (a lane that reads
another lane's record moves a reply), and the 4 KB of the transfer log after the call's last record
hold a sentinel that must survive the commit.  The sources of a case, and which kernel each runs:

  copy          a separate HBM buffer (commit_device_async): `<false>`
  inplace       the log window (tbgpu_log_window): `<false>`, PassArgs.inplace
  commit        Engine.commit, one call per prepare: the body is copied to the engine's staging
                buffer from pageable memory, then `<false>`
  pipelined     a registered buffer through commit_pipelined: DMA into a pipeline slot, then `<false>`
  read_through  tbgpu_commit, one call per prepare, with the body inside a registered buffer: the
                `<true>` instantiation reads it over PCIe and writes it through to the staging buffer,
                the stage's only store to global memory

For `commit` and `read_through` the 4 KB of the staging buffer (tbgpu_debug_staging) after the
prepare's events hold a sentinel too, and after `read_through` the staging buffer's first L events
are the body.  The pipeline slot that `pipelined` copies into is not reachable and is not checked.

tb_resolve_lean loads the account slots and amounts of a thread's RESOLVE_K events behind
`i < L && HZ_ACCTS`: one in-place legs pass whose short prepares put the `i < L` edge at the first,
the last and a middle thread of a row, with a late-path amount or a failing event on each edge, and
a second one in which a linked pair sends one prepare to tb_resolve while its neighbours stay lean.
(Regression cover for that loop, which a change that loads unconditionally from clamped indices
would have to keep right.)"""
import ctypes

import numpy as np
import pytest

from tests.harness.configs import timestamps
from tests.harness.oracle import OracleEngine
from tests.test_gpu_differential import assert_same_state
from tigerbeetle_amd import _lib
from tigerbeetle_amd.types import ACCOUNT_DTYPE, TRANSFER_DTYPE, TransferFlags

pytestmark = pytest.mark.gpu

N_ACCOUNTS = 64
SENTINEL_BYTES = 4096
SENTINEL = 0xA5
# total events -> the prepares the call is cut into
CUTS = [
    (1, [1]), (7, [3, 4]), (8, [7, 1]), (9, [3, 5, 1]), (63, [62, 1]), (64, [63, 1]), (65, [63, 1, 1]),
    (255, [200, 55]), (256, [255, 1]), (257, [200, 57]), (257, [256, 1]), (511, [255, 256]), (513, [255, 258]),
]
CUT_IDS = ["%d-%s" % (n, "_".join(map(str, cuts))) for n, cuts in CUTS]
TRANSFER_SOURCES = ["copy", "inplace", "commit", "pipelined", "read_through"]
ACCOUNT_SOURCES = ["copy", "commit", "pipelined", "read_through"]


def edge_positions(n):
    """Lane 0 and lane 63 of a wave, the first and last event of a tile and of the call."""
    return sorted(p for p in {0, 63, 64, 127, 255, 256, n - 1} if p < n) if n > 1 else []


def account_events(n, first_id=1):
    a = np.zeros(n, dtype=ACCOUNT_DTYPE)
    k = np.arange(n, dtype=np.uint64)
    a["id_lo"] = first_id + k
    a["user_data_64"] = 1000 + k  # a swapped row shows in the account
    a["ledger"] = 1
    a["code"] = 7
    return a


def transfer_events(n):
    t = np.zeros(n, dtype=TRANSFER_DTYPE)
    k = np.arange(n, dtype=np.uint64)
    t["id_lo"] = 1 + k
    t["debit_account_id_lo"] = 1 + k % N_ACCOUNTS
    t["credit_account_id_lo"] = 1 + (k + 1 + k // N_ACCOUNTS) % N_ACCOUNTS  # never the debit account (n < 63 * 64)
    t["amount_lo"] = 1 + k * k + k  # distinct, and distinct sums for swapped neighbours
    t["ledger"] = 1
    t["code"] = 7
    for q, p in enumerate(edge_positions(n)):
        if q % 3 == 0:
            t["id_lo"][p] = 0  # id_must_not_be_zero
        elif q % 3 == 1:
            t["debit_account_id_lo"][p] = 10_000  # debit_account_not_found
        else:
            t["timestamp"][p] = 5  # timestamp_must_be_zero
    return t


def split_bodies(events, cuts):
    raw, bodies, off = events.tobytes(), [], 0
    for L in cuts:
        bodies.append(raw[off * 128:(off + L) * 128])
        off += L
    return bodies


def device_replies(engine, res_dev, rb_dev, cuts):
    rb = engine.to_host(rb_dev, len(cuts) * 4).view(np.uint32)
    res = engine.to_host(res_dev, sum(cuts) * 8)
    out, off = [], 0
    for L, nb in zip(cuts, rb):
        out.append(bytes(res[off * 8:off * 8 + int(nb)]))
        off += L
    return out


def staging_address(engine):
    p = ctypes.c_void_p(0)
    _lib.check(engine.lib.tbgpu_debug_staging(engine.h, ctypes.byref(p)))
    return int(p.value)


def host_commits(engine, op, ts, cuts, bodies, registered):
    """One tbgpu_commit per prepare.  registered: the bodies lie inside a registered host buffer, so
    kernel 1's `<true>` instantiation reads each one through and writes it to the staging buffer;
    otherwise the engine copies a pageable body there.  Either way the staging buffer after the
    prepare's events is untouched, and after a read-through its first L events are the body."""
    staging = staging_address(engine)
    sentinel = np.full(SENTINEL_BYTES, SENTINEL, dtype=np.uint8)
    pool = np.zeros(max(sum(len(b) for b in bodies), 4096), dtype=np.uint8)
    if registered:
        engine.register_host(pool)
    replies, at = [], 0
    try:
        for t, L, body in zip(ts, cuts, bodies):
            engine.to_device(staging + L * 128, sentinel)
            if registered:
                pool[at:at + len(body)] = np.frombuffer(body, dtype=np.uint8)
                out = ctypes.create_string_buffer(max(L * 8, 8))
                out_len = ctypes.c_uint32(0)
                _lib.check(engine.lib.tbgpu_commit(engine.h, op, t, ctypes.c_void_p(pool.ctypes.data + at), len(body), out,
                                                   len(out), ctypes.byref(out_len)))
                replies.append(out.raw[:out_len.value])
                assert bytes(engine.to_host(staging, len(body))) == body, "the write-through copy differs from the body"
                at += len(body)
            else:
                replies.append(engine.commit(op, t, body))
            assert bytes(engine.to_host(staging + L * 128, SENTINEL_BYTES)) == sentinel.tobytes(), \
                "written past the prepare's events in the staging buffer"
    finally:
        if registered:
            engine.unregister_host(pool)
    return replies


def run_source(engine, source, op, ts, cuts, bodies):
    """The call's replies, one per prepare, committed through `source`."""
    n = sum(cuts)
    body = np.frombuffer(b"".join(bodies), dtype=np.uint8)
    if source in ("commit", "read_through"):
        return host_commits(engine, op, ts, cuts, bodies, registered=source == "read_through")
    if source == "pipelined":
        buf = np.zeros(max(body.nbytes, 4096), dtype=np.uint8)
        buf[:body.nbytes] = body
        engine.register_host(buf)
        try:
            out_lens, replies, _ = engine.commit_pipelined(op, ts, cuts, buf)
        finally:
            engine.unregister_host(buf)
        out, off = [], 0
        for L, nb in zip(cuts, out_lens):
            out.append(bytes(replies[off * 8:off * 8 + int(nb)]))
            off += L
        return out
    ev = engine.log_window(n) if source == "inplace" else engine.alloc(n * 128)
    engine.to_device(ev, body)
    res_dev, rb_dev = engine.alloc(n * 8), engine.alloc(len(cuts) * 4)
    engine.commit_device_async(op, ts, cuts, ev, res_dev, rb_dev)
    engine.sync()
    return device_replies(engine, res_dev, rb_dev, cuts)


def make_pair(gpu_engine_factory, n_accounts=N_ACCOUNTS, **kw):
    """An oracle and an engine holding the same accounts 1..n_accounts; returns the next timestamp too."""
    oracle = OracleEngine(max(n_accounts, 1024), kw.get("transfers_max", 1 << 12))
    engine = gpu_engine_factory(**kw)
    t = 10**9
    if n_accounts:
        acc = account_events(n_accounts)
        for first in range(0, n_accounts, 8190):
            body = acc[first:first + 8190].tobytes()
            t += len(body) // 128 + 1
            assert oracle.commit(128, t, body) == engine.commit(128, t, body) == b""
    return oracle, engine, t


@pytest.mark.parametrize("source", TRANSFER_SOURCES)
@pytest.mark.parametrize("n,cuts", CUTS, ids=CUT_IDS)
def test_transfer_stage_edges(n, cuts, source, gpu_engine_factory):
    assert sum(cuts) == n
    oracle, engine, t = make_pair(gpu_engine_factory)
    bodies = split_bodies(transfer_events(n), cuts)
    ts, _ = timestamps(cuts, t + 10)
    expected = [oracle.commit(129, tk, b) for tk, b in zip(ts, bodies)]
    # The log after the call's last record: whichever source the events come from, their records go
    # to log positions [0, n), and nothing may be written at n and after.
    tail = engine.log_window(n + SENTINEL_BYTES // 128) + n * 128
    engine.to_device(tail, np.full(SENTINEL_BYTES, SENTINEL, dtype=np.uint8))
    actual = run_source(engine, source, 129, ts, cuts, bodies)
    for k, (e, a) in enumerate(zip(expected, actual)):
        assert e == a, "reply of prepare %d differs" % k
    assert len(actual) == len(expected)
    assert_same_state(oracle, engine)
    assert bytes(engine.to_host(tail, SENTINEL_BYTES)) == bytes([SENTINEL]) * SENTINEL_BYTES, "written past the call's events"


@pytest.mark.parametrize("source", ACCOUNT_SOURCES)
@pytest.mark.parametrize("n,cuts", CUTS, ids=CUT_IDS)
def test_account_stage_edges(n, cuts, source, gpu_engine_factory):
    oracle, engine, t = make_pair(gpu_engine_factory, n_accounts=0)
    acc = account_events(n)
    for q, p in enumerate(edge_positions(n)):
        if q % 3 == 0:
            acc["id_lo"][p] = 0  # id_must_not_be_zero
        elif q % 3 == 1:
            acc["ledger"][p] = 0  # ledger_must_not_be_zero
        else:
            acc["timestamp"][p] = 5  # timestamp_must_be_zero
    bodies = split_bodies(acc, cuts)
    ts, _ = timestamps(cuts, t + 10)
    expected = [oracle.commit(128, tk, b) for tk, b in zip(ts, bodies)]
    actual = run_source(engine, source, 128, ts, cuts, bodies)
    for k, (e, a) in enumerate(zip(expected, actual)):
        assert e == a, "reply of prepare %d differs" % k
    assert len(actual) == len(expected)
    assert_same_state(oracle, engine)


# -- tb_resolve_lean ------------------------------------------------------------------------------
LEAN_ACCOUNTS = 50_000
LEAN_CUTS = [8190] * 32 + [1, 1023, 1024, 1025, 8189, 8190]
LATE_AMOUNT = 1 << 52  # not a leg amount (csrc/pass.h LEG_AMT_BITS): applied by the late path


def lean_events(linked_pair):
    n = sum(LEAN_CUTS)
    assert n >= 1 << 18  # csrc/pass.h LEGS_MIN_EVENTS: below it the legs path is off
    t = np.zeros(n, dtype=TRANSFER_DTYPE)
    k = np.arange(n, dtype=np.uint64)
    t["id_lo"] = 1 + k
    t["debit_account_id_lo"] = 1 + k % LEAN_ACCOUNTS
    t["credit_account_id_lo"] = 1 + (k + 1 + k // LEAN_ACCOUNTS) % LEAN_ACCOUNTS
    t["amount_lo"] = 1 + k
    t["ledger"] = 1
    t["code"] = 7
    first = 0
    for p, L in enumerate(LEAN_CUTS):
        if p >= 32:  # the short prepares: the edges of a thread's row of RESOLVE_K events
            edges = {L - 1} | {i for m in range(1, L // 1024 + 2) for i in (1024 * m - 1, 1024 * m + 1) if i < L}
            for q, i in enumerate(sorted(edges)):
                if (q + p) % 2:
                    t["amount_lo"][first + i] = LATE_AMOUNT + i
                else:
                    t["debit_account_id_lo"][first + i] = 10**9  # debit_account_not_found
        first += L
    if linked_pair:  # in the 1024-event prepare: it alone goes to tb_resolve
        at = sum(LEAN_CUTS[:34]) + 10
        t["flags"][at] = int(TransferFlags.linked)
    return t


@pytest.mark.parametrize("linked_pair", [False, True], ids=["lean", "one_prepare_to_resolve"])
def test_resolve_lean_row_edges(linked_pair, gpu_engine_factory):
    n = sum(LEAN_CUTS)
    oracle, engine, t = make_pair(gpu_engine_factory, n_accounts=LEAN_ACCOUNTS, accounts_max=LEAN_ACCOUNTS,
                                  transfers_max=1 << 19, pass_events_max=n, pass_batches_max=len(LEAN_CUTS))
    bodies = split_bodies(lean_events(linked_pair), LEAN_CUTS)
    ts, _ = timestamps(LEAN_CUTS, t + 10)
    expected = [oracle.commit(129, tk, b) for tk, b in zip(ts, bodies)]
    actual = run_source(engine, "inplace", 129, ts, LEAN_CUTS, bodies)
    for k, (e, a) in enumerate(zip(expected, actual)):
        assert e == a, "reply of prepare %d differs" % k
    assert any(expected[32:]), "the planted failures must show in the replies"
    assert_same_state(oracle, engine)
