"""Every result code and check-order pair (tests/harness/ladder.py) on every commit path, GPU vs the
oracle byte for byte: replies, accounts, transfers, the posted groove, commit_timestamp, then the
lookups of every id the family named.

The reference's check order is restated in k_validate.h (kernel 1), in k_replay.h twice (FLOW = false:
the one-lane replay; FLOW = true: tb_flow) and in k_resolve.h tb_classify (may kernel 1's code be
trusted?).  The placements put the same events on each: one prepare per call, one multi-prepare
pass, the sorted balance legs, the sequential fallback, an in-place pass, and the node engine on two
and three shards.  The `ordered*` families chain every mutated event to a dependent transfer and
same_pass_exists collides ids inside a pass, so those are judged by k_replay.h's ladders; the stats
assertions show the path was the one taken.  tests/test_result_ladder.py keeps the scenarios honest
on the CPU."""
import pytest

from tests.harness import ladder
from tests.harness.oracle import OracleEngine
from tests.harness.workload import run_many, run_oracle
from tests.test_gpu_differential import assert_same_state
from tests.test_gpu_inplace import run_inplace

pytestmark = pytest.mark.gpu

FAMILIES = sorted(ladder.FAMILIES)
ORDERED_PATH = ("ordered", "ordered_late", "same_pass_exists")
PLACEMENTS = ("commit", "commit_many", "legs", "sequential", "inplace", "node2", "node3")


@pytest.fixture
def node_factory():
    from tigerbeetle_amd.state_machine import Engine, Options

    made = []

    def make(devices=(0, 0), **kw):
        opts = dict(accounts_max=4096, transfers_max=1 << 17, pass_events_max=8192 * 4, pass_batches_max=64,
                    devices=tuple(devices))
        opts.update(kw)
        e = Engine(Options(**opts))
        made.append(e)
        return e

    yield make
    for e in made:
        e.close()


def _engine(placement, gpu_engine_factory, node_factory):
    """(engine, how the scenario is committed on it)."""
    if placement == "commit":
        return gpu_engine_factory(), run_oracle
    if placement == "commit_many":
        return gpu_engine_factory(), run_many
    if placement == "legs":
        engine = gpu_engine_factory()
        engine.legs_min_events(0)
        return engine, run_many
    if placement == "sequential":
        return gpu_engine_factory(sequential_fallback=True), run_many
    if placement == "inplace":
        return gpu_engine_factory(), run_inplace
    if placement == "node2":
        return node_factory(devices=(0, 0)), run_oracle
    return node_factory(devices=(0, 0, 0)), run_many


def _dependent_floor(sc, family, placement):
    """Events the builder made dependent that this placement keeps in one pass."""
    if family != "same_pass_exists":
        return sc.counts["chain_members"]
    # one prepare per call: only the collisions inside one prepare share a pass
    return sc.counts["colliding_same_prepare"] if placement == "commit" else sc.counts["colliding"]


def _check_lookups(sc, oracle, engine):
    ts = max(sc.ts, oracle.commit_timestamp) + 10
    for op, body in ladder.lookup_requests(sc):
        assert len(body) // 16 <= 8191
        want = oracle.commit(op, ts, body)
        got = engine.commit(op, ts, body)
        assert got == want, "lookup %d differs" % op  # a failed event's id is found by neither
        assert len(want) > 0
        ts += 10


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("family", FAMILIES)
def test_result_ladder(family, placement, gpu_engine_factory, node_factory):
    sc = ladder.family(family)
    oracle = OracleEngine()
    expected = run_oracle(sc, oracle)
    engine, run = _engine(placement, gpu_engine_factory, node_factory)
    actual = run(sc, engine)
    assert len(actual) == len(expected)
    for k, (e, a) in enumerate(zip(expected, actual)):
        if e != a:
            pytest.fail("reply of prepare %d differs:\n%s" % (k, _describe(sc, k, e, a)))
    assert_same_state(oracle, engine)

    st = engine.stats()
    if placement == "sequential":
        assert st["flow_passes"] == 0 and st["dependent_events"] > 0, st
    elif placement.startswith("node"):
        if family in ORDERED_PATH:  # a dirty pass: its dependent events went through the sequencer
            assert st["node_passes_split"] + st["node_passes_whole"] > 0, st
    elif family in ORDERED_PATH:
        assert st["flow_passes"] > 0, st
        assert st["dependent_events"] >= _dependent_floor(sc, family, placement) > 0, st

    _check_lookups(sc, oracle, engine)
    if family in ("late_clock", "ordered_late"):
        stored = oracle.export_transfers()
        assert len(stored) and int(stored["timestamp"].min()) >= ladder.LATE_START


def _describe(sc, k, expected, actual, limit=12):
    """The events of prepare k whose codes differ, with the mutations that made them."""
    import numpy as np

    from tigerbeetle_amd.types import RESULT_DTYPE

    def table(reply):
        r = np.frombuffer(reply, dtype=RESULT_DTYPE)
        return dict(zip(r["index"].tolist(), r["result"].tolist()))

    step = [i for i, s in enumerate(sc.steps) if s[0] == "commit"][k]
    names = {kk: "+".join(m.name for m in muts) for s, kk, muts, _c in sc.marks if s == step}
    e, a = table(expected), table(actual)
    lines = []
    for i in sorted(set(e) | set(a)):
        if e.get(i, 0) != a.get(i, 0):
            lines.append("  event %d (%s): oracle %d, engine %d" % (i, names.get(i, "-"), e.get(i, 0), a.get(i, 0)))
    return "\n".join(lines[:limit] + (["  ... %d more" % (len(lines) - limit)] if len(lines) > limit else []))
