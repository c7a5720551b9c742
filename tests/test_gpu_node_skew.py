"""The node engine (csrc/node.h, k_node.h, k_route.h) where its shards are NOT loaded evenly, against
the oracle byte for byte.  Every other node test feeds ids that hash evenly, so each home receives
about 1/N of a pass in one routed sub-pass, each owner about 1/N of the legs, and no import gate fires
where a test can see it.  Here (workloads: tests/harness/node_ids.py, checked on the oracle alone in
tests/test_node_ids.py):

  A. every transfer of whole passes homed on one shard: that home commits a pass in several
     sub-passes (import gate, flush, import, the in-place log window, codes, the owner-leg regions and
     leg_counts carried from one to the next) while the other homes receive nothing;
  B. every account owned by one shard (it applies every leg of every home, the others import every
     account they name), or a shard that owns none;
  C. dirty passes (limit accounts, chains, two-phase) with every transfer the sequencer creates
     written back to one home, or every account loaded from one owner;
  D. a home's import gate at its boundary: live imports at room - 1, room and room + 1 when a
     sub-pass of 1024 new foreign accounts arrives — the gate must flush when live + 2 n would pass
     the room, and only then (tbgpu_bench_node_imports);
  E. the single-engine edge scenarios (8191-event prepares, whole-batch chains, extreme ids and
     amounts, sums past 2^128) on 2 and 3 shards.
"""
import numpy as np
import pytest

from tests.harness import node_ids
from tests.harness.oracle import OracleEngine
from tests.harness.workload import run_many, run_oracle
from tests.test_gpu_differential import CONFIGS, _run, assert_same_state
from tests.test_gpu_edges import SCENARIOS, _state
from tests.test_gpu_node import node_factory  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def _ids2(ids):
    ids = np.asarray(ids, dtype=np.uint64)
    return np.stack([ids, np.zeros_like(ids)], axis=1)


def _commit(engine, call, pipelined):
    """One call's replies, one bytes per prepare: commit_many, or commit_pipelined from registered
    host memory in one-prepare blocks."""
    if not pipelined:
        return engine.commit_many(call.op, call.ts, call.bodies())
    host = call.events if call.events.size else np.zeros(128, dtype=np.uint8)
    engine.register_host(host)
    try:
        rb, rep, _ = engine.commit_pipelined(call.op, call.ts, call.lens, host, chunk_batches=1)
    finally:
        engine.unregister_host(host)
    out, off = [], 0
    for L, nb in zip(call.lens, rb):
        out.append(bytes(rep[off * 8:off * 8 + int(nb)]))
        off += L
    return out


def _run_skew(sk, engine, oracle, pipelined=False, lookups=False):
    """Every call on both; replies, state, the ledger summary (read with the imports still in the
    tables), the stored transfer count and (lookups) every account read where it lives."""
    for k, call in enumerate(sk.calls):
        want = oracle.commit_many(call.op, call.ts, call.bodies())
        got = _commit(engine, call, pipelined and call.op == node_ids.CREATE_TRANSFERS)
        for j, (w, g) in enumerate(zip(want, got)):
            assert w == g, "call %d: reply of prepare %d differs" % (k, j)
        assert len(got) == len(want)
    led = engine.ledger_summary()
    assert led["accounts"] == len(sk.account_ids) and led["stray"] == 0, led
    assert engine.stats()["transfers"] == len(oracle.export_transfers())
    if lookups:
        ids = _ids2(np.concatenate([sk.account_ids, sk.account_ids[:16] + np.uint64(1 << 41)]))
        got, g_found = engine.fetch_accounts(ids)
        want, w_found = oracle.fetch_accounts(ids)
        assert np.array_equal(g_found, w_found) and int(w_found.sum()) == len(sk.account_ids)
        assert got.tobytes() == want.tobytes()
    assert_same_state(oracle, engine)


def _never_flushed(engine, world):
    """The room is the whole ledger (every small shape): the import gate never flushes."""
    for d in range(world):
        imp = engine.node_imports(d)
        assert imp["flushes"] == 0 and imp["live"] <= imp["room"], (d, imp)


# -- A. home skew ------------------------------------------------------------------------------------

@pytest.mark.parametrize("pipelined", [False, True], ids=["commit_many", "pipelined"])
@pytest.mark.parametrize("target", [0, 3])
def test_node_home_skew(target, pipelined, node_factory):
    """16384-event passes homed whole on one of 4 shards (shard pass_events_max 13312: two routed
    sub-passes of 8190 and 8194 events; in one-prepare blocks a pass is 4096 events, one sub-pass)
    while three homes receive nothing; ids repeated across passes and across the sub-passes of one,
    events answered at the source, missing accounts, amount_hi != 0, a ragged last pass."""
    cfg = node_ids.HOME_SKEW
    engine = node_factory(devices=(0,) * cfg["world"], accounts_max=cfg["accounts_max"], transfers_max=cfg["transfers_max"],
                          pass_events_max=cfg["pass_events_max"], pass_batches_max=cfg["pass_batches_max"])
    _run_skew(node_ids.home_skew(target), engine, OracleEngine(cfg["accounts_max"], cfg["transfers_max"]), pipelined)
    st = engine.stats()
    assert st["node_passes_split"] == 0 and st["node_passes_whole"] == 0, st  # clean passes: all of it routed
    _never_flushed(engine, cfg["world"])


# -- B. owner skew -----------------------------------------------------------------------------------

@pytest.mark.parametrize("owners", [(0,), (2,), (0, 1)], ids=["all-on-0", "all-on-2", "none-on-2"])
def test_node_owner_skew(owners, node_factory):
    """3000 accounts on one owner of 3 (tb_node_apply_legs: one owner takes every home's every leg,
    the others none), or none on shard 2; hot accounts, balances that cross 2^64 by carry under a
    u128 certificate."""
    cfg = node_ids.OWNER_SKEW
    engine = node_factory(devices=(0,) * cfg["world"], accounts_max=cfg["accounts_max"], transfers_max=cfg["transfers_max"],
                          pass_events_max=cfg["pass_events_max"], pass_batches_max=cfg["pass_batches_max"])
    _run_skew(node_ids.owner_skew(owners), engine, OracleEngine(cfg["accounts_max"], cfg["transfers_max"]), lookups=True)
    st = engine.stats()
    assert st["node_passes_split"] == 0 and st["node_passes_whole"] == 0, st
    _never_flushed(engine, cfg["world"])


# -- C. skew under dirty passes ------------------------------------------------------------------------

@pytest.mark.parametrize("many", [False, True], ids=["commit", "commit_many"])
@pytest.mark.parametrize("variant", ["home", "owner"])
@pytest.mark.parametrize("config", ["limits", "chains", "two_phase"])
def test_node_dirty_skew(config, variant, many, node_factory):
    sc, _ = node_ids.dirty_skew(CONFIGS[config], variant)
    engine = node_factory(devices=(0,) * node_ids.DIRTY_SKEW_WORLD)
    _run(sc, OracleEngine(), engine, many)
    st = engine.stats()
    assert st["node_passes_split"] + st["node_passes_whole"] > 0, st
    assert engine.ledger_summary()["stray"] == 0


# -- D. the import gate at its boundary ------------------------------------------------------------------

@pytest.mark.parametrize("target", [node_ids.GATE_ROOM - 1, node_ids.GATE_ROOM, node_ids.GATE_ROOM + 1],
                         ids=["room-1", "room", "room+1"])
def test_node_import_gate_boundary(target, node_factory):
    """Home 0 of 2 imports one new foreign account per event (no two lanes the same id, so the live
    count is exact).  gate_fill raises its live imports to room - 1 = 2047 in steps the gate's rule lets
    through, then (room, room + 1) one step more that the rule must flush before; then 1024 accounts
    never named, the first 1024 again, ids no owner holds, those accounts created, and named again.
    After every call: the oracle's replies, accounts (read where they live: an export would flush the
    imports), transfers and ledger summary; live <= room; live >= the existing foreign ids named since
    the last flush; and the flush counter moved exactly when live + 2 n > room held before the call's
    one sub-pass.  (With the gate's need at 0 the fill reaches room - 1, room and room + 1 unflushed
    and the next 1024 imports land on top: live <= room fails.)"""
    cfg = node_ids.GATE
    engine = node_factory(devices=(0, 0), accounts_max=cfg["accounts_max"], transfers_max=cfg["transfers_max"],
                          pass_events_max=cfg["pass_events_max"], pass_batches_max=cfg["pass_batches_max"])
    oracle = OracleEngine(cfg["accounts_max"], cfg["transfers_max"])
    sk, named = node_ids.gate_boundary(target)
    every = _ids2(sk.account_ids)
    room = engine.node_imports(0)["room"]
    assert room == node_ids.GATE_ROOM
    since_flush, created, flushed_ever = set(), 0, 0
    for k, (call, ids) in enumerate(zip(sk.calls, named)):
        before = engine.node_imports(0)
        want = oracle.commit_many(call.op, call.ts, call.bodies())
        assert engine.commit_many(call.op, call.ts, call.bodies()) == want, "call %d" % k
        after = engine.node_imports(0)
        where = "call %d (%d events): %r -> %r" % (k, sum(call.lens), before, after)
        if ids is None:  # create_accounts: every import out, no gate involved
            created += sum(call.lens)
            since_flush = set()
            assert after["live"] == 0 and after["flushes"] == before["flushes"], where
        else:
            must_flush = before["live"] + 2 * sum(call.lens) > room
            assert after["flushes"] - before["flushes"] == (1 if must_flush else 0), where
            since_flush = set(ids) if must_flush else since_flush | ids
            flushed_ever += must_flush
        assert after["live"] <= room, where
        assert after["live"] >= len(since_flush), where
        assert engine.node_imports(1)["live"] == 0  # home 1 receives nothing
        led = engine.ledger_summary()
        assert led["accounts"] == created and led["stray"] == 0, (where, led)
        got, g_found = engine.fetch_accounts(every)
        exp, e_found = oracle.fetch_accounts(every)
        assert np.array_equal(g_found, e_found) and got.tobytes() == exp.tobytes(), where
        assert engine.export_transfers().tobytes() == oracle.export_transfers().tobytes(), where
        assert engine.commit_timestamp == oracle.commit_timestamp
    assert flushed_ever >= 2  # the rule fired: at the latest before the 1024 new and the 1024 old ones
    assert_same_state(oracle, engine)


# -- E. the single-engine edge scenarios on a node ---------------------------------------------------------

@pytest.mark.parametrize("many", [False, True], ids=["commit", "commit_many"])
@pytest.mark.parametrize("shards", [2, 3])
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_node_edges(name, shards, many, node_factory):
    sc = SCENARIOS[name]()
    oracle = OracleEngine()
    expected = run_oracle(sc, oracle)
    engine = node_factory(devices=(0,) * shards, transfers_max=1 << 16)
    actual = run_many(sc, engine) if many else run_oracle(sc, engine)
    assert actual == expected
    led = engine.ledger_summary()
    assert led["stray"] == 0, led
    assert _state(engine) == _state(oracle)
    _never_flushed(engine, shards)
