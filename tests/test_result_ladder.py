"""CPU: the result-ladder scenarios (tests/harness/ladder.py) are what they claim, judged by the
oracle alone — every family runs without a panic, every mutation alone gives the code it is named
for, every non-ok code of create_transfers (55) and create_accounts (21) wins somewhere, also on a
chained (ordered-path) event, and every exists* code appears in each same-pass placement.  The GPU
side is tests/test_gpu_result_ladder.py."""
import collections

import pytest

from tests.harness import ladder
from tests.harness.oracle import OracleEngine
from tests.harness.workload import run_oracle
from tigerbeetle_amd.types import CreateTransferResult as CT

FAMILIES = sorted(ladder.FAMILIES)
_replies = {}


def _oracle_replies(name):
    """The oracle's replies to a family, computed once (an OraclePanic propagates: a fixture bug)."""
    if name not in _replies:
        _replies[name] = run_oracle(ladder.family(name), OracleEngine())
    return _replies[name]


def _winning(names, op, chained_only=False):
    got = collections.Counter()
    for name in names:
        sc = ladder.family(name)
        for code, (step, _k, _muts, chained) in ladder.winners(sc, _oracle_replies(name)):
            if sc.steps[step][1] == op and code != 0 and (chained or not chained_only):
                got[code] += 1
    return got


def test_mutation_tables_name_every_code():
    assert {m.code for m in ladder.TRANSFER_MUTATIONS} == ladder.NON_OK_TRANSFER_CODES
    assert {m.code for m in ladder.ACCOUNT_MUTATIONS} == ladder.NON_OK_ACCOUNT_CODES
    assert len(ladder.NON_OK_TRANSFER_CODES) == 55 and len(ladder.NON_OK_ACCOUNT_CODES) == 21
    for table in (ladder.TRANSFER_MUTATIONS, ladder.ACCOUNT_MUTATIONS):
        assert len({m.name for m in table}) == len(table)


@pytest.mark.parametrize("name", FAMILIES)
def test_family_runs_on_the_oracle(name):
    sc = ladder.family(name)
    assert all(step[0] == "commit" for step in sc.steps), "balances are built by committed transfers only"
    assert all(len(step[3]) <= ladder.PREPARE_MAX for step in sc.steps)
    replies = _oracle_replies(name)  # no OraclePanic
    assert len(replies) == len(sc.steps)
    assert sc.marks
    if name in ("late_clock", "ordered_late"):
        assert all(step[2] >= ladder.LATE_START for step in sc.steps)  # account creation included


@pytest.mark.parametrize("name", ["singles", "late_clock"])
def test_each_mutation_alone_gives_its_code(name):
    sc = ladder.family(name)
    seen = set()
    for code, (_step, _k, muts, _chained) in ladder.winners(sc, _oracle_replies(name)):
        if len(muts) == 1:
            assert code == muts[0].code, "%s gave %d" % (muts[0].name, code)
            seen.add((muts[0].op, muts[0].name))
    late = name == "late_clock"
    want = {(m.op, m.name) for m in ladder.TRANSFER_MUTATIONS + ladder.ACCOUNT_MUTATIONS if late or not m.late_only}
    assert want <= seen
    # overflows_timeout is out of reach on the ordinary clock, and only there
    assert ((129, "overflows_timeout") in seen) == late


def test_every_code_wins_somewhere():
    names = ["singles", "pairs", "late_clock"]
    assert set(_winning(names, 129)) == ladder.NON_OK_TRANSFER_CODES
    assert set(_winning(names, 128)) == ladder.NON_OK_ACCOUNT_CODES


def test_every_transfer_code_wins_on_a_chained_event():
    """ordered holds every code but overflows_timeout (ordinary clock); ordered_late every code."""
    assert set(_winning(["ordered"], 129, chained_only=True)) == ladder.NON_OK_TRANSFER_CODES - {CT.overflows_timeout}
    assert set(_winning(["ordered_late"], 129, chained_only=True)) == ladder.NON_OK_TRANSFER_CODES
    for name in ("ordered", "ordered_late"):
        sc = ladder.family(name)
        assert all(chained for _s, _k, _m, chained in sc.marks)
        assert sc.counts["chain_members"] >= 2 * len(sc.marks)


def test_same_pass_exists_covers_every_placement():
    sc = ladder.family("same_pass_exists")
    got = {p: set() for p in ladder.PLACEMENTS}
    for k, (code, _mark) in enumerate(ladder.winners(sc, _oracle_replies("same_pass_exists"))):
        got[sc.placement[k]].add(code)
    for p in ladder.PLACEMENTS:
        assert got[p] == ladder.EXISTS_TRANSFER_CODES, p
    assert sc.counts["colliding"] > 0


def test_pairs_matrix_is_not_empty():
    """Generated 1277 pairs (1090 of transfers, 187 of accounts), skipped 1489 of 2766 = 53.8 %: a pair
    is skipped when its mutations share no base event (a create-ladder edit with a post / void one),
    when they set one field to different values, or when one of them must end its prepare
    (linked_event_chain_open).  The cap of 55 % sits just above that share, so that a later edit
    cannot quietly empty the matrix; the floor of 1200 pairs is the same guard from the other side."""
    counts = ladder.family("pairs").counts
    generated, skipped = counts["pairs_generated"], counts["pairs_skipped"]
    print("pairs generated %d, skipped %d (%.1f %%)" % (generated, skipped, 100.0 * skipped / (generated + skipped)))
    assert generated >= 1200
    assert skipped <= 0.55 * (generated + skipped)
    marked = [m for m in ladder.family("pairs").marks if len(m[2]) == 2]
    assert len(marked) == generated


def test_late_clock_holds_the_timeout_pairs():
    """The two events the overflow certificate's special case is about: a pending transfer that fails
    an overflow check and the timeout check (the overflow code wins), and one that fails the timeout
    check on a limit account it would also exceed (overflows_timeout wins)."""
    sc = ladder.family("late_clock")
    found = {}
    for code, (_step, _k, muts, _chained) in ladder.winners(sc, _oracle_replies("late_clock")):
        found[frozenset(m.name for m in muts)] = code
    assert found[frozenset(["overflows_debits_pending", "overflows_timeout"])] == CT.overflows_debits_pending
    assert found[frozenset(["overflows_timeout", "exceeds_credits"])] == CT.overflows_timeout
    assert found[frozenset(["overflows_timeout", "exceeds_debits"])] == CT.overflows_timeout


def test_failed_events_are_not_stored():
    """The lookups the GPU test compares: no id that only failed events carried is found."""
    import numpy as np

    from tigerbeetle_amd.types import TRANSFER_DTYPE
    sc = ladder.family("pairs")
    oracle = OracleEngine()
    run_oracle(sc, oracle)
    stored = set()
    for op, body in ladder.lookup_requests(sc):
        assert len(body) // 16 <= 8191
        reply = oracle.commit(op, sc.ts + 10, body)
        if op == 131:
            r = np.frombuffer(reply, dtype=TRANSFER_DTYPE)
            stored |= {int(lo) | (int(hi) << 64) for lo, hi in zip(r["id_lo"], r["id_hi"])}
    assert stored == {int(lo) | (int(hi) << 64) for lo, hi in zip(oracle.export_transfers()["id_lo"],
                                                                  oracle.export_transfers()["id_hi"])}
    failed = set()
    for code, (step, k, _muts, _chained) in ladder.winners(sc, _oracle_replies("pairs")):
        id_ = int.from_bytes(sc.steps[step][3][k][:16], "little")
        if sc.steps[step][1] == 129 and code != 0 and id_ > 10**6:  # a fresh id: no other event carries it
            failed.add(id_)
    assert failed and not failed & stored
