"""tb_flow's late balance adds against its in-kernel sequential replay (csrc/k_flow.h tb_flow,
k_apply.h tb_apply_late, k_replay.h rp_create_transfer<false>).

tb_flow applies the independent ok transfers that are not balance legs itself, with atomic adds.  The
sequential replay a pass falls back to (a chain longer than FLOW_CHAIN_MAX) loads an account's four
balances, changes them and stores them whole, and a chain's rollback stores its before-image: an add
that lands on the same account in between is lost — one field of one account short by one amount,
every reply still right.  The adds must therefore all be ordered before the replay: only workgroups
admitted to the pass's grid apply them, before the first grid barrier (k_flow.h).

tests/harness/late_apply.py builds the pass (its claims are held to the oracle in
tests/test_late_apply_scenarios.py): 64 x 8190 events over 8 accounts, every prepare headed by a
dependent chain of 70, half of them rolled back, every other event an independent transfer between
the same accounts.  Each variant is committed as ONE pass — from host buffers with the balance legs
off, for `postvoid` also with them on (the late set is then its posts / voids), and in place in the
log window — with the default launch and with tb_flow launched with 2048 workgroups, eight times what
the device holds at once (test_gpu_liveness.py): the events from pass index 262,144 on then belong to
workgroups that can only start once others have left, i.e. while workgroup 0 replays.  Before the adds
were ordered, 11 of these 14 cases failed, default launches included (eight accounts take so many
adds that admission closed while most were still queued): the first differing field was off by
19,933 to 5,854,176, thousands of lost amounts.

The last test carries DESIGN.md §7f's report: after plain per-prepare commits of
test_gpu_balances.py::test_unordered_log's half A, about once in twenty runs one debits_pending
differed from the oracle's by 20."""
import numpy as np
import pytest

from tests.harness.balances import pack, replay_rows, select
from tests.harness.dependence import dependent_count
from tests.harness.late_apply import BATCH, CHAIN, EVENTS, PREPARES, VARIANTS, LateApply
from tests.harness.oracle import OracleEngine
from tests.harness.workload import make_scenario
from tests.test_gpu_differential import assert_same_state
from tests.test_gpu_query import commit_all
from tigerbeetle_amd import _lib
from tigerbeetle_amd.state_machine import Engine, Options

pytestmark = pytest.mark.gpu

LEGS_OFF, LEGS_ON = 2**32 - 1, 0

PLACEMENTS = [(v, p) for v in VARIANTS
              for p in (("many", "many_legs", "inplace") if v == "postvoid" else ("many", "inplace"))]


@pytest.fixture(scope="module")
def scenario():
    """variant -> the pass, the oracle that committed it, its replies, the model's dependent count and
    account 0's balance history over the last prepare (computed once, never changed)."""
    _made = {}

    def get(variant):
        if variant not in _made:
            sc = LateApply(variant)
            oracle = OracleEngine(64, 1 << 20)
            sc.commit_setup(oracle)
            replies = oracle.commit_many(129, sc.timestamps, sc.bodies)
            assert replies == sc.expected_replies()
            account = sc.account_ids[0]
            t = oracle.export_transfers()
            lo = account & (2**64 - 1)
            # Account 0's balances follow from its own records alone (a post / void's record names its
            # pending transfer's accounts).
            rows = replay_rows(t[(t["debit_account_id_lo"] == lo) | (t["credit_account_id_lo"] == lo)])
            window = dict(timestamp_min=sc.timestamps[-1] - BATCH + 1, timestamp_max=sc.timestamps[-1])
            want, matched = select(pack(rows[account]), **window)
            assert matched == len(want) > 1000
            _made[variant] = dict(sc=sc, oracle=oracle, replies=replies, window=window, rows=want,
                                  dependent=dependent_count(sc.bodies, sc.accounts, sc.existing_ids))
        return _made[variant]

    yield get
    for made in _made.values():
        made["oracle"].close()


def commit_pass(engine, sc, placement):
    """The pass as one call; returns the prepares' replies."""
    if placement != "inplace":
        return engine.commit_many(129, sc.timestamps, sc.bodies)
    window = engine.log_window(EVENTS)
    engine.to_device(window, sc.events.view(np.uint8))
    res, rb = engine.alloc(EVENTS * 8), engine.alloc(PREPARES * 4)
    try:
        engine.commit_device_async(129, sc.timestamps, sc.lens, window, res, rb)
        engine.sync()
        nbytes = engine.to_host(rb, PREPARES * 4).view(np.uint32)
        out = engine.to_host(res, EVENTS * 8)
        return [bytes(out[k * BATCH * 8:k * BATCH * 8 + int(nbytes[k])]) for k in range(PREPARES)]
    finally:
        engine.free(res)
        engine.free(rb)


@pytest.mark.parametrize("launch", ["default", "overlaunched"])
@pytest.mark.parametrize("variant,placement", PLACEMENTS)
def test_late_adds_and_the_sequential_replay(variant, placement, launch, scenario, gpu_engine_factory, monkeypatch):
    made = scenario(variant)
    sc, oracle = made["sc"], made["oracle"]
    if launch == "overlaunched":
        monkeypatch.setenv("TBGPU_STALL_MS", "1000")  # read by tbgpu_init: every wait bounded at 1 s
    engine = gpu_engine_factory(accounts_max=4096, transfers_max=1 << 20, pass_events_max=EVENTS,
                                pass_batches_max=PREPARES)
    engine.legs_min_events(LEGS_ON if placement == "many_legs" else LEGS_OFF)
    if launch == "overlaunched":
        _lib.check(engine.lib.tbgpu_bench_flow_launch(engine.h, 2048))  # 8x the MI355X's 256 CUs
    sc.commit_setup(engine)
    before = engine.stats()
    replies = commit_pass(engine, sc, placement)
    after = engine.stats()
    for k, (want, got) in enumerate(zip(made["replies"], replies)):
        assert got == want, "reply of prepare %d differs" % k
    # The balances before the whole-state comparison, so a lost add reads as one: account, field, difference.
    want, got = oracle.export_accounts(), engine.export_accounts()
    assert len(want) == len(got)
    for a, b in zip(want, got):
        for name in a.dtype.names:
            assert a[name] == b[name], "account %x %s: engine - oracle = %d" % (
                int(a["id_lo"]), name, int(b[name]) - int(a[name]))
    assert_same_state(oracle, engine)
    # An engine with flow enabled counted the chains dependent and no flow pass: the pass took tb_flow's
    # in-kernel sequential replay.
    assert after["passes"] - before["passes"] == 1
    assert after["dependent_events"] - before["dependent_events"] == made["dependent"] == PREPARES * CHAIN
    assert after["flow_passes"] == before["flow_passes"]
    # The history is derived from the balances: it agrees.
    rows, matched, complete = engine.get_account_balances(sc.account_ids[0], limit=8190, **made["window"])
    assert rows.tobytes() == made["rows"].tobytes() and matched == len(made["rows"]) and complete


UNORDERED = dict(n_accounts=8, n_transfer_batches=40, batch_len=(100, 400), p_pending=0.3, p_dup=0.05, p_linked=0.05,
                 p_limit=0.0, p_balancing=0.0, p_invalid=0.05, id_space=1 << 40, p_post_void=0.25)


def test_plain_commits_of_the_unordered_log_a_hundred_times():
    """test_unordered_log's half A (seed 31), one commit per prepare, on a hundred fresh engines: the
    accounts are the oracle's every time.  The report was one debits_pending off by 20 about once in
    twenty runs, so a hundred clean runs leave under 1 % (0.95^100) for that defect to have hidden."""
    sa = make_scenario(31, **UNORDERED)
    oracle = OracleEngine(64, 1 << 15)
    expected = commit_all(sa, oracle)
    want = oracle.export_accounts()
    oracle.close()
    assert sum(len(s[3]) for s in sa.steps if s[1] == 129) > 5000
    for run in range(100):
        engine = Engine(Options(accounts_max=4096, transfers_max=1 << 15, pass_events_max=8192 * 4, pass_batches_max=64))
        try:
            assert commit_all(sa, engine) == expected, "run %d: replies differ" % run
            got = engine.export_accounts()
        finally:
            engine.close()
        if got.tobytes() == want.tobytes():
            continue
        assert len(got) == len(want), "run %d" % run
        for a, b in zip(want, got):
            for name in a.dtype.names:
                assert a[name] == b[name], "run %d, account %x %s: engine - oracle = %d" % (
                    run, int(a["id_lo"]), name, int(b[name]) - int(a[name]))
