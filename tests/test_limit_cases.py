"""The claims of tests/harness/limit_cases.py's builder, checked on the oracle (no GPU): what
tests/test_gpu_limit_edges.py relies on to reach the tier, window and segment boundaries of tb_flow's
limit-check path.  These are conditions on the inputs, met by the reference alone."""
import numpy as np
import pytest

from tests.harness import limit_cases as lc
from tests.harness.oracle import OracleEngine
from tigerbeetle_amd.types import TRANSFER_DTYPE

CASES = lc.all_cases()
LIMIT_CODES = (lc.OK, lc.EXCEEDS_CREDITS, lc.EXCEEDS_DEBITS)


def balances(oracle, account):
    a = oracle.export_accounts()
    a = a[a["id_lo"] == account][0]
    return [int(a[n + "_lo"]) + (int(a[n + "_hi"]) << 64)
            for n in ("debits_pending", "debits_posted", "credits_pending", "credits_posted")]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_fulfils_its_intent(case):
    oracle = OracleEngine(4096, 1 << 16)
    try:
        bound, codes = 0, None
        seen = set()
        for step in case.steps:
            if step.label == "test" and case.name.startswith("carry 2^64"):
                src, full = 1, 3
                assert balances(oracle, src)[1] == balances(oracle, full)[3] == lc.U64 - 1
                assert case.slack(full) >= 0 and ("hovering" in case.name) == (balances(oracle, full)[1] == lc.U64 - 1)
            replies = step.commit(oracle)  # (an oracle panic raises)
            if step.op == 128:
                assert all(r == b"" for r in replies)
                continue
            assert 1 <= len(step.events) <= 6500
            codes = lc.codes_of(step, replies)
            # The model of the two limit checks is the reference's behaviour on these inputs.
            assert np.array_equal(codes, step.expected), step.label
            assert replies == step.expected_replies()
            assert set(codes.tolist()) <= set(LIMIT_CODES)  # nothing rejected statically
            # bound and S again, from the bytes committed and the oracle's replies: S sums the events
            # the static checks let through — here the ok ones and the limit failures.
            ev = np.frombuffer(b"".join(step.bodies), dtype=TRANSFER_DTYPE)
            through = np.isin(codes, LIMIT_CODES)
            S = sum(int(lo) + (int(hi) << 64) for lo, hi in zip(ev["amount_lo"][through], ev["amount_hi"][through]))
            assert (step.bound, step.S) == (bound, S)
            bound = min(bound + S, lc.U128 - 1)
            assert oracle.balance_bound() <= bound  # what `bound` is for
            if step.label not in ("park", "fund", "draw", "fill"):
                seen |= set(codes.tolist())
                # Outcomes mix in every pass under test.
                assert lc.OK in codes and (codes != lc.OK).any(), step.label
        last = case.passes[-1]
        if "target" in case.intent:
            assert last.bound + last.S == case.intent["target"]
        assert case.intent["codes"] <= seen
        if "closed_form" in case.intent:
            assert codes.tolist() == case.intent["closed_form"]
            # The amounts under test begin on a window boundary of the undecided segment (position 0
            # is the second event after the funding: the blocker) and both outcomes occur among them.
            start, n = case.intent["start"], len(case.intent["amounts"])
            assert len(codes) == 2 + start + n and [e[2] for e in last.events[-n:]] == case.intent["amounts"]
            assert len(set(codes[-n:].tolist())) == 2
        for account, want in case.intent.get("closed_form_by_account", {}).items():
            mine = [k for k, e in enumerate(last.events) if account in e[:2]]
            assert codes[mine].tolist() == want
        if "units" in case.intent:
            (d, c), want = case.intent["units"]
            mine = [k for k, e in enumerate(last.events) if e[:2] == (d, c)]
            assert codes[mine].tolist() == want
            assert lc.EXCEEDS_CREDITS in want and lc.EXCEEDS_DEBITS in want
        if case.intent.get("cert64") is False:
            assert last.bound < lc.U64 <= last.bound + last.S
            assert balances(oracle, 1)[1] >= lc.U64 and balances(oracle, 3)[3] >= lc.U64  # the words carried
    finally:
        oracle.close()


def test_alternating_closed_form():
    """Y X X ... gives strictly alternating ok / failure, on either flag, also from 2^62."""
    for flag, big in ((lc.DLIM, 0), (lc.CLIM, 0), (lc.DLIM, 1 << 62)):
        case = lc.Case("alternating")
        src, sink = case.accounts(2)
        seg = lc.Seg(case, case.account(flag), src, sink)
        if big:
            case.transfers([seg.y(big)])
            case.transfers([seg.x(big)])
        step = case.transfers(lc.alternating(seg, 50))
        assert step.expected.tolist() == lc.alternating_codes(seg, 50)
        oracle = OracleEngine()
        assert case.run(oracle)[-1] == step.expected_replies()
        oracle.close()


def test_tier_targets():
    """The tier cases sit exactly at T - 1 and T, and the inside variant's limit account holds about
    T / 2 on both sides."""
    for tier, T in lc.TIERS.items():
        for at in (-1, 0):
            for where in lc.WHERE:
                case = lc.tier_case(tier, at, where)
                last = case.passes[-1]
                assert last.bound + last.S == T + at and last.label == "test" and 300 < len(last.events) < 6000
                if where == "inside":
                    heavy = last.events[0][1]  # the first event pays the heavy account
                    assert case.flags[heavy] == lc.DLIM
                    b = case.balance[heavy]
                    assert b[1] > T // 2 - 1000 and b[3] > T // 2 - 1000 and case.slack(heavy) == 0
                if where == "wide":
                    assert max(max(b) for b in case.balance.values()) >= 400 * (T // 1024) and last.S > T // 2
    for at in (-1, 0):
        last = lc.global_case(at).passes[-1]
        assert last.bound + last.S == lc.U128 + at
