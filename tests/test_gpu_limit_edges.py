"""tb_flow's limit-check path (csrc/k_flow.h fl_bounds, fl_sweep, fl_walk*; csrc/pass.h
tb_pass_cert) at its tier, window and segment boundaries, against the oracle.

The path picks among several implementations from values the input controls: the magnitude of
bound + S (walkers below 2^62, the signed window sweep below 2^63, the u64 sweep below 2^64, the
ordered run above; no global certificate from 2^128), the amounts of a walked run (32-bit chain iff
all below 2^24, the running value clamped to +-2^30), the length of a segment (WALK_HEAVY = 256,
64-position windows), the number of heavy segments against the workgroups launched (merged / a wave
each / all light), and the rounds a pass needs (FLOW_BOUNDS_ROUNDS_MAX = 4096).  The random suites
reach these statistically at best; tests/harness/limit_cases.py builds passes that sit on each edge
(its claims are held to the oracle in tests/test_limit_cases.py), and every test here commits one on
the engine and on the oracle, compares every reply byte and the whole state, and reads the engine's
counters to see that the intended path ran.

Every wait of the kernel is bounded at 2 s here (TBGPU_STALL_MS), so a walker that stops making
progress is an EnginePanic within seconds, not a hang."""
import numpy as np
import pytest

from tests.harness import limit_cases as lc
from tests.harness.oracle import OracleEngine
from tests.test_gpu_differential import assert_same_state
from tigerbeetle_amd import _lib

pytestmark = pytest.mark.gpu

COUNTERS = ("passes", "flow_passes", "bounds_passes", "bounds_rounds", "bounds_abandoned", "bounds_swept",
            "sweep_u64_passes", "walk_segments", "walk_heavy", "walk_heavy_positions", "walk_heavy_windows",
            "walk_crit_windows")


@pytest.fixture(scope="module")
def reference():
    """case -> the oracle that committed it and its replies per step (computed once per case name,
    never changed)."""
    made = {}

    def get(case):
        if case.name not in made:
            oracle = OracleEngine(4096, 1 << 16)
            made[case.name] = (oracle, case.run(oracle))
        return made[case.name]

    yield get
    for oracle, _ in made.values():
        oracle.close()


@pytest.fixture
def engines(gpu_engine_factory, monkeypatch):
    monkeypatch.setenv("TBGPU_STALL_MS", "2000")  # read by tbgpu_init: every wait bounded at 2 s
    return gpu_engine_factory


def commit_case(engine, case, reference):
    """Commits `case` on `engine`: replies and state equal to the oracle's.  Returns, per
    create_transfers pass, what the engine's counters gained in it (walk_longest: its value after)."""
    oracle, replies = reference(case)
    gains = []
    for step, want in zip(case.steps, replies):
        before = engine.stats()
        got = step.commit(engine)
        assert len(got) == len(want)
        for k, (w, g) in enumerate(zip(want, got)):
            if w != g:
                w, g = np.frombuffer(w, dtype=np.uint32).reshape(-1, 2), np.frombuffer(g, dtype=np.uint32).reshape(-1, 2)
                raise AssertionError("%s, pass %r, prepare %d: reply differs: oracle %s..., engine %s..." % (
                    case.name, step.label, k, w[:8].tolist(), g[:8].tolist()))
        if step.op == 129:
            after = engine.stats()
            gain = {c: after[c] - before[c] for c in COUNTERS}
            gain["walk_longest"] = after["walk_longest"]
            assert gain["passes"] == 1 and after["bounds_skipped"] == 0
            gains.append(gain)
    assert_same_state(oracle, engine)
    return gains


def launch(engine, workgroups):
    _lib.check(engine.lib.tbgpu_bench_flow_launch(engine.h, workgroups))


# ---- magnitude tiers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds_sweep", ["auto", "early"])
@pytest.mark.parametrize("where", lc.WHERE)
@pytest.mark.parametrize("tier,at", [(t, at) for t in lc.TIERS for at in (-1, 0)])
def test_tier(tier, at, where, bounds_sweep, engines, reference):
    """The same hovering pass with bound + S at T - 1 and at T, the big amount on free accounts or
    inside the heavy limit account (X and Y of its checks about T / 2), or in the pass's own legs of
    T / 1024 each."""
    case = lc.tier_case(tier, at, where)
    g = commit_case(engines(bounds_sweep=bounds_sweep), case, reference)[-1]
    assert g["flow_passes"] == 1 and g["bounds_abandoned"] == 0
    if (tier, at) == ("2^62", -1):
        assert g["bounds_passes"] == 1 and g["walk_segments"] == 2 and g["walk_heavy"] == 1 and g["sweep_u64_passes"] == 0
    elif (tier, at) in (("2^62", 0), ("2^63", -1)):
        assert g["bounds_passes"] == 1 and g["walk_segments"] == 0 and g["bounds_swept"] > 300 and g["sweep_u64_passes"] == 0
    elif (tier, at) in (("2^63", 0), ("2^64", -1)):
        assert g["bounds_passes"] == 1 and g["walk_segments"] == 0 and g["bounds_swept"] > 300 and g["sweep_u64_passes"] == 1
    else:
        assert g["bounds_passes"] == 0 and g["bounds_swept"] == 0 and g["walk_segments"] == 0


@pytest.mark.parametrize("legs", ["default", "legs"])
@pytest.mark.parametrize("hover", [False, True])
def test_balance_words_carry_across_2_64(hover, legs, engines, reference):
    """The first pass without the 64-bit certificate: a free account's debits_posted and a limit
    account's credits_posted go from 2^64 - 1 to 2^64 in it (hover: under that account's own checks).
    legs: with the sorted-legs apply on for every pass."""
    case = lc.carry_case(hover)
    engine = engines()
    if legs == "legs":
        engine.legs_min_events(0)
    g = commit_case(engine, case, reference)[-1]
    assert g["flow_passes"] == 1 and g["bounds_passes"] == 0 and g["walk_segments"] == 0


@pytest.mark.parametrize("at", [-1, 0])
def test_global_certificate_flip(at, engines, reference):
    """bound + S = 2^128 - 1 against 2^128 with limit accounts hovering: no bounds either way."""
    g = commit_case(engines(), lc.global_case(at), reference)[-1]
    assert g["bounds_passes"] == 0 and g["bounds_swept"] == 0


# ---- the walkers' 32-bit / 64-bit arithmetic -----------------------------------------------------------------
WALKS = {c.name: c for heavy in (False, True) for c in lc.walk_cases(heavy)}


@pytest.mark.parametrize("walk_merge", [0, 63])
@pytest.mark.parametrize("name", sorted(WALKS))
def test_walk_arithmetic(name, walk_merge, engines, reference):
    """Amounts at the 2^24 gate, slack at the amount and one off, the running value at the 2^30 clamp:
    each from a window boundary of a light segment and of a heavy one, a wave per heavy segment and
    merged."""
    case = WALKS[name]
    engine = engines(bounds_sweep="early")
    engine.walk_merge_max(walk_merge)
    g = commit_case(engine, case, reference)[-1]
    n = case.intent["start"] + len(case.intent["amounts"])
    assert g["bounds_passes"] == 1 and g["walk_segments"] == 1 and g["bounds_swept"] == n
    assert g["walk_heavy"] == (1 if case.intent["heavy"] else 0)
    if case.intent["heavy"]:
        assert g["walk_longest"] == n and g["walk_heavy_windows"] > 0 and g["walk_heavy_positions"] == n
        assert (g["walk_crit_windows"] > 0) == (walk_merge == 0)  # a wave of its own / the merged walk


# ---- segment lengths ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk_merge", [0, 63])
def test_segment_lengths(walk_merge, engines, reference):
    """One limit account with 1 ... 577 undecided positions, pass after pass on one engine: every
    window count from 1 to 10, and WALK_HEAVY from below, at and above."""
    case = lc.lengths_case()
    engine = engines(bounds_sweep="early")
    engine.walk_merge_max(walk_merge)  # 63: the heavy ones through the merged walker and its ring of 8 windows
    gains = commit_case(engine, case, reference)
    assert len(gains) == len(lc.LENGTHS)
    longest, seen = 0, {}
    for L, g in zip(lc.LENGTHS, gains):
        assert g["bounds_passes"] == 1 and g["walk_segments"] == 1 and g["bounds_abandoned"] == 0, L
        seen[L] = (g["bounds_swept"], g["walk_heavy"], g["walk_longest"], g["walk_heavy_windows"])
        print("L=%d: swept %d, heavy %d, longest %d, heavy windows %d" % ((L,) + seen[L]))
    for L, (swept, heavy, wl, windows) in seen.items():
        # (a segment within one 1024-position chunk is read before any of the round's decisions land:
        # the undecided length is the construction's)
        assert swept == L and heavy == (1 if L >= 256 else 0), (L, seen[L])
        if heavy:
            longest = max(longest, L)
            assert wl == longest and windows >= (L + 63) // 64, (L, seen[L])
        else:
            assert wl == longest and windows == 0, (L, seen[L])
    assert seen[255][1] == 0 and seen[256][2] == 256 and seen[257][2] == 257


# ---- dispatch of the heavy segments ----------------------------------------------------------------------------
def expect_dispatch(g, nh, workgroups, walk_merge):
    assert g["bounds_passes"] == 1 and g["walk_heavy"] == nh and g["walk_segments"] >= nh + 2
    if nh <= walk_merge:  # merged: the units with a heavy leg counted, no walker of its own
        assert g["walk_heavy_positions"] > 0 and g["walk_heavy_windows"] > 0 and g["walk_crit_windows"] == 0
    elif nh <= workgroups // 2:  # split: a wave per heavy segment
        assert g["walk_heavy_positions"] >= 256 * nh and g["walk_heavy_windows"] >= 4 * nh and g["walk_crit_windows"] > 0
    else:  # heavy-length segments walked by the light waves
        assert g["walk_heavy_positions"] == 0 and g["walk_heavy_windows"] == 0 and g["walk_crit_windows"] == 0


@pytest.mark.parametrize("workgroups", [4, 1, 2])
@pytest.mark.parametrize("linked,walk_merge", [(False, 0), (True, 0), (True, 63)])
@pytest.mark.parametrize("nh", [1, 2, 3])
def test_dispatch(nh, linked, walk_merge, workgroups, engines, reference):
    """nh heavy segments in a pass small enough for 4 workgroups (and launched with 1 and 2): merged,
    a wave each (nh <= workgroups / 2), or walked by the light waves (nh = 3 of 4 workgroups)."""
    case = lc.dispatch_case(nh, linked)
    engine = engines(bounds_sweep="early")
    engine.walk_merge_max(walk_merge)
    if workgroups != 4:
        launch(engine, workgroups)
    g = commit_case(engine, case, reference)[-1]
    expect_dispatch(g, nh, workgroups, walk_merge)


@pytest.mark.parametrize("workgroups", [4, 1])
def test_more_light_segments_than_light_waves(workgroups, engines, reference):
    """96 segments of 4 checks linked by two-check units over 64 (16) light waves: waves cycle over
    segments that wait on each other."""
    engine = engines(bounds_sweep="early")
    if workgroups != 4:
        launch(engine, workgroups)
    g = commit_case(engine, lc.mesh_case(), reference)[-1]
    assert g["bounds_passes"] == 1 and g["walk_segments"] >= 80 and g["walk_heavy"] == 0


# ---- the segmented scan's carries ----------------------------------------------------------------------------------
SCANS = {c.name: c for c in (lc.equal_segments_case(64), lc.equal_segments_case(128), lc.long_segment_case())}


@pytest.mark.parametrize("bounds_sweep", ["early", "off"])
@pytest.mark.parametrize("name", sorted(SCANS))
def test_scan_carries(name, bounds_sweep, engines, reference):
    """Segments that start on every wave, chunk and tile boundary of the scan, and one that covers a
    whole tile; early: one round and the walk, off: rounds alone."""
    g = commit_case(engines(bounds_sweep=bounds_sweep), SCANS[name], reference)[-1]
    assert g["bounds_passes"] == 1 and g["bounds_abandoned"] == 0
    if bounds_sweep == "off":
        assert g["bounds_swept"] == 0 and g["walk_segments"] == 0
        assert g["bounds_rounds"] > (1000 if name == "long segment" else 30)
    else:
        assert g["walk_segments"] == (7 if name == "long segment" else 3072 // int(name.split()[-1]))
        # (the long segment spans chunks: statuses read mid-round may decide a few more than the first)
        assert 1024 < g["walk_longest"] <= 1665 if name == "long segment" else g["walk_longest"] == 0


# ---- the window sweep's head table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tier", [False, True])
def test_window_sweep_table(tier, engines, reference):
    """1536 segment heads in one window sweep (SW_CAP = 1024 live in LDS, the rest in global memory):
    asked for (window-early), and where the walkers give way to it, in the [2^62, 2^63) tier.  (Both
    sweep after the first round: with 512 segments and more every round decides 512 units, each
    segment's first, so "auto" goes on with rounds to the end.)"""
    engine = engines(bounds_sweep="early" if tier else "window-early")
    g = commit_case(engine, lc.table_case(tier=tier), reference)[-1]
    assert g["bounds_passes"] == 1 and g["walk_segments"] == 0 and g["bounds_swept"] >= 1500 and g["sweep_u64_passes"] == 0


# ---- rounds exhausted ---------------------------------------------------------------------------------------------------
def test_abandoned_bounds_leave_no_trace(engines, reference):
    """Rounds alone on an alternating segment of 4300 checks: FLOW_BOUNDS_ROUNDS_MAX rounds decide
    about one check each, the pass takes the ordered run with nothing changed; the next pass on the
    same accounts converges."""
    long, after = commit_case(engines(bounds_sweep="off"), lc.abandon_case(), reference)
    assert long["bounds_abandoned"] == 1 and long["bounds_passes"] == 0 and long["bounds_swept"] == 0
    assert long["bounds_rounds"] == 4096 and long["flow_passes"] == 1
    assert after["bounds_abandoned"] == 0 and after["bounds_passes"] == 1 and after["bounds_swept"] == 0


# ---- event kinds in a segment ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk_merge", [0, 63])
@pytest.mark.parametrize("heavy", [False, True])
@pytest.mark.parametrize("kind", lc.KINDS)
def test_event_kinds(kind, heavy, walk_merge, engines, reference):
    """Pending legs on either side, units with two open checks, Y legs of undecided units, in light
    and in heavy segments."""
    case = lc.kinds_case(kind, heavy)
    engine = engines(bounds_sweep="early")
    engine.walk_merge_max(walk_merge)
    g = commit_case(engine, case, reference)[-1]
    codes = set(case.passes[-1].expected.tolist())
    assert {lc.EXCEEDS_CREDITS, lc.EXCEEDS_DEBITS} <= codes
    assert g["bounds_passes"] == 1 and g["walk_segments"] >= 2 and (g["walk_heavy"] > 0) == heavy


@pytest.mark.parametrize("form", ["asked", "signed", "u64"])
@pytest.mark.parametrize("kind", lc.KINDS)
def test_event_kinds_in_the_window_sweep(kind, form, engines, reference):
    """The same kinds through the one-wave window sweep: asked for below 2^62 (window-early), and where
    bound + S makes the default build take it, in its signed slack form and in its u64 X / Y form."""
    case = lc.kinds_case(kind, False, target=lc.SWEEP_TARGETS.get(form))
    g = commit_case(engines(bounds_sweep="window-early" if form == "asked" else "early"), case, reference)[-1]
    assert g["bounds_passes"] == 1 and g["walk_segments"] == 0 and g["bounds_swept"] > 50
    assert g["sweep_u64_passes"] == (1 if form == "u64" else 0)


@pytest.mark.parametrize("walk_merge", [0, 63])
@pytest.mark.parametrize("amount", lc.OPEN_Y_AMOUNTS)
def test_open_y_legs_by_amount(amount, walk_merge, engines, reference):
    """Y legs of undecided units in a heavy segment, their amounts at the gates of the walk with
    pending credits (2^22 for a leg, 2^28 for the credits pending) and of the plain walk (2^24)."""
    engine = engines(bounds_sweep="early")
    engine.walk_merge_max(walk_merge)
    g = commit_case(engine, lc.kinds_case("open_y", True, amount), reference)[-1]
    assert g["bounds_passes"] == 1 and g["walk_heavy"] == 2 and g["walk_heavy_positions"] > 0


# ---- on a two-shard node ------------------------------------------------------------------------------------------------------
@pytest.fixture
def node(monkeypatch):
    from tigerbeetle_amd.state_machine import Engine, Options

    monkeypatch.setenv("TBGPU_STALL_MS", "2000")
    made = []

    def make(**kw):
        e = Engine(Options(accounts_max=4096, transfers_max=1 << 17, pass_events_max=8192 * 4, pass_batches_max=64,
                           devices=(0, 0), **kw))
        made.append(e)
        return e

    yield make
    for e in made:
        e.close()


NODE = [lc.tier_case(t, at, w) for t in ("2^62", "2^64") for at in (-1, 0) for w in ("parked", "inside")]
NODE.append(lc.kinds_case("two_check", True))


@pytest.mark.parametrize("case", NODE, ids=[c.name for c in NODE])
def test_on_a_node(case, node, reference):
    oracle, replies = reference(case)
    engine = node()
    for step, want in zip(case.steps, replies):
        assert step.commit(engine) == want, (case.name, step.label)
    assert_same_state(oracle, engine)
