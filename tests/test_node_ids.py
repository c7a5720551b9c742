"""CPU: the ids-by-home helper (tests/harness/node_ids.py) and the skewed node workloads of
tests/test_gpu_node_skew.py on the oracle alone — the pools land where they were asked to, the id
renaming of make_scenario leaves every existing seed's bytes alone and keeps a renamed scenario's
references intact, and every skewed workload is well-formed: the oracle answers it without a panic,
with ok and non-ok replies, and with the shape the GPU test relies on (where the duplicates sit, which
balances cross 2^64, what the import gate's rule makes of the fill steps)."""
import hashlib

import numpy as np
import pytest

from tests.harness import node_ids
from tests.harness.node_ids import IdPlan, ids_homed
from tests.harness.oracle import OracleEngine
from tests.harness.shard_double import homes_of
from tests.harness.workload import make_scenario, run_oracle
from tests.test_gpu_differential import CONFIGS
from tigerbeetle_amd.types import RESULT_DTYPE, TRANSFER_DTYPE, CreateTransferResult as R, TransferFlags as TF


def _homes(ids, world):
    ids = np.asarray(ids, dtype=np.uint64)
    return homes_of(np.stack([ids, np.zeros_like(ids)], axis=1), world)


@pytest.mark.parametrize("world", [2, 3, 4])
def test_ids_homed_pools(world):
    pools = [ids_homed(world, s, 500) for s in range(world)]
    for s, p in enumerate(pools):
        assert len(p) == 500 and np.all(np.diff(p.astype(np.int64)) > 0) and p[0] >= 1
        assert np.all(_homes(p, world) == s)
    every = np.concatenate(pools)
    assert len(np.unique(every)) == len(every)
    # The first n at or above start: nothing of that home was skipped, and start is honoured.
    span = np.arange(1, int(every.max()) + 1, dtype=np.uint64)
    for s, p in enumerate(pools):
        assert np.array_equal(span[_homes(span, world) == s][:500], p)
    late = ids_homed(world, world - 1, 40, start=1 << 33)
    assert late[0] >= 1 << 33 and np.all(_homes(late, world) == world - 1)
    assert np.array_equal(ids_homed(world, 0, 10, start=int(pools[0][3])), pools[0][3:13])


def _digest(sc):
    h = hashlib.sha256()
    for s in sc.steps:
        if s[0] == "commit":
            h.update(b"c%d,%d," % (s[1], s[2]))
            for e in s[3]:
                h.update(e)
        else:
            h.update(repr(s).encode())
    return h.hexdigest()


# sha256 over every step of the scenario as make_scenario built it before it took transfer_id_of /
# account_id_of: seeds of test_gpu_differential (mixed, overflow: setup steps) and test_gpu_node.
BEFORE = [
    (7926, "mixed", "abeb0238e26430d7157bdf0289ebdcb948a784fe8f69dfffb77ef1d4b3c9e59a"),
    (5973, "two_phase", "afb4f1cfdfd57e0bed476b135d8d2f167af7a372c94e6d5f3264b7236686f2a1"),
    (24641, "overflow", "32b74027001b05f1a75783087348414275220fc765b90f61ff9e2dbf480eeab5"),
]


@pytest.mark.parametrize("seed,config,digest", BEFORE, ids=[c for _, c, _ in BEFORE])
def test_make_scenario_bytes_unchanged(seed, config, digest):
    assert _digest(make_scenario(seed, **CONFIGS[config])) == digest
    same = make_scenario(seed, transfer_id_of=lambda i: i, account_id_of=lambda i: i, **CONFIGS[config])
    assert _digest(same) == digest


def _codes(replies):
    return np.concatenate([np.frombuffer(r, dtype=RESULT_DTYPE)["result"] for r in replies] + [np.zeros(0, np.uint32)])


def _transfers(sc):
    return np.frombuffer(b"".join(b"".join(s[3]) for s in sc.steps if s[0] == "commit" and s[1] == 129),
                         dtype=TRANSFER_DTYPE)


@pytest.mark.parametrize("variant", ["home", "owner"])
@pytest.mark.parametrize("config", ["limits", "chains", "two_phase"])
def test_dirty_skew_scenarios(config, variant):
    """Renaming is a bijection that keeps 0, and no result depends on an id's value: the renamed
    scenario's replies are the plain one's byte for byte — so every pending_id still names the
    transfer it named (posts and voids succeed and fail where they did), and the mix is non-trivial."""
    sc, plan = node_ids.dirty_skew(CONFIGS[config], variant)
    plain = run_oracle(make_scenario(1, **CONFIGS[config]), OracleEngine())
    replies = run_oracle(sc, OracleEngine())
    assert replies == plain
    t = _transfers(sc)
    n_fail = len(_codes(replies[-8:]))
    assert 0 < n_fail < len(t)
    assert np.all(t["id_hi"] == 0) if variant == "home" else np.all(t["debit_account_id_hi"] == 0)
    if variant == "home":
        assert np.all(_homes(t["id_lo"][t["id_lo"] != 0], 3) == 2)
        assert np.all(_homes(t["pending_id_lo"][t["pending_id_lo"] != 0], 3) == 2)
        assert len(plan.transfer_ids()) > 100 and not plan.account_ids()
    else:
        for side in ("debit_account_id_lo", "credit_account_id_lo"):
            assert np.all(_homes(t[side][t[side] != 0], 3) == 1)
        assert len(plan.account_ids()) >= CONFIGS[config].get("n_accounts", 64)
    if config == "two_phase":  # posts / voids that found their pending transfer under its new id
        resolving = (t["flags"] & int(TF.post_pending_transfer | TF.void_pending_transfer)) != 0
        failed = np.zeros(len(t), dtype=bool)
        off = 0
        for s, r in zip([s for s in sc.steps if s[0] == "commit"][-8:], replies[-8:]):
            failed[off + np.frombuffer(r, dtype=RESULT_DTYPE)["index"]] = True
            off += len(s[3])
        assert np.any(resolving & ~failed) and np.any(resolving & failed)


def _check_mix(sk, replies):
    for call, rep in zip(sk.calls, replies):
        if call.op == node_ids.CREATE_ACCOUNTS:
            assert all(r == b"" for r in rep)
        else:
            assert 0 < len(_codes(rep)) < sum(call.lens)


@pytest.mark.parametrize("target", [0, 3])
def test_home_skew_scenario(target):
    sk = node_ids.home_skew(target)
    replies = node_ids.run_skew_oracle(sk, OracleEngine(6000, 1 << 17))
    _check_mix(sk, replies)
    big = sk.calls[1]
    assert big.lens == [1024] * 32 + [7, 0]
    t = big.events.view(TRANSFER_DTYPE)
    assert np.all(_homes(t["id_lo"], 4) == target)
    P = node_ids.HOME_SKEW_PASS
    assert sum(big.lens) + 2000 <= 40_000  # under the target shard's log
    codes = np.zeros(len(t), dtype=np.uint32)
    off = 0
    for L, r in zip(big.lens, replies[1]):
        pairs = np.frombuffer(r, dtype=RESULT_DTYPE)
        codes[off + pairs["index"]] = pairs["result"]
        off += L
    for base in (0, P):  # a copy in the home's second sub-pass of an id committed in its first
        late = codes[base + 13000:base + 13060]
        first = codes[base + 100:base + 160]
        assert np.sum(first == R.ok) > 40
        assert np.sum(late == R.exists) > 10 and np.sum(late == R.exists_with_different_amount) > 10
    second = codes[P:2 * P]
    assert np.sum(second == R.exists) > 200 and np.sum(second == R.exists_with_different_amount) > 200
    for want in (R.timestamp_must_be_zero, R.debit_account_not_found, R.credit_account_not_found):
        assert np.sum(codes[:P] == want) >= 10 and np.sum(second == want) >= 10
    ok = codes == R.ok
    assert np.sum(ok & (t["amount_hi"] != 0)) >= 40 and np.sum(ok[2 * P:]) == 7
    # Most legs are foreign to the target: its sub-passes import.
    owners = _homes(np.concatenate([t["debit_account_id_lo"], t["credit_account_id_lo"]]), 4)
    assert 0.6 < np.mean(owners != target) < 0.9


@pytest.mark.parametrize("owners", [(0,), (2,), (0, 1)], ids=["all-on-0", "all-on-2", "none-on-2"])
def test_owner_skew_scenario(owners):
    sk = node_ids.owner_skew(owners)
    oracle = OracleEngine(4096, 1 << 17)
    replies = node_ids.run_skew_oracle(sk, oracle)
    _check_mix(sk, replies)
    assert len(sk.account_ids) == 3000 and len(np.unique(sk.account_ids)) == 3000
    assert set(_homes(sk.account_ids, 3).tolist()) == set(owners)
    for call in sk.calls[1:]:
        assert call.lens == [2000] * 9
        ids = call.events.view(TRANSFER_DTYPE)["id_lo"]
        assert len(set(_homes(ids, 3).tolist())) == 3  # even transfer ids: every home receives
    acc = oracle.export_accounts()
    # Balances past 2^64 reached by carry (most wide amounts are below 2^63 with amount_hi = 0).
    assert np.sum(acc["debits_posted_hi"] != 0) >= 20 and np.sum(acc["credits_posted_hi"] != 0) >= 20
    legs = np.concatenate([c.events.view(TRANSFER_DTYPE)[s] for c in sk.calls[1:]
                           for s in ("debit_account_id_lo", "credit_account_id_lo")])
    _, counts = np.unique(legs, return_counts=True)
    assert 0.45 < np.sort(counts)[-20:].sum() / len(legs) < 0.6  # the Zipf-like head


def test_gate_fill_follows_the_rule():
    room = node_ids.GATE_ROOM
    for target in (room - 1, room, room + 1):
        steps = node_ids.gate_fill(target)
        live, flushes = 0, 0
        for n in steps:
            assert 1 <= n <= node_ids.GATE_PASS
            if live + 2 * n > room:
                flushes, live = flushes + 1, 0
            live += n
            assert live <= room
        # room - 1 is the most the rule lets a home hold before a sub-pass; a step past it flushes.
        assert sum(steps) == target and flushes == (0 if target < room else 1)
        assert live == (target if target < room else target - (room - 1))
        assert sum(steps[:-1]) == room - 1 or target < room


@pytest.mark.parametrize("target", [node_ids.GATE_ROOM - 1, node_ids.GATE_ROOM, node_ids.GATE_ROOM + 1])
def test_gate_boundary_scenario(target):
    sk, named = node_ids.gate_boundary(target)
    assert len(named) == len(sk.calls)
    oracle = OracleEngine(16384, 1 << 15)
    replies = node_ids.run_skew_oracle(sk, oracle)
    assert len(oracle.export_accounts()) == node_ids.GATE["accounts_max"]
    seen = set()
    for call, ids, rep in zip(sk.calls, named, replies):
        if call.op == node_ids.CREATE_ACCOUNTS:
            assert ids is None and all(r == b"" for r in rep)
            continue
        t = call.events.view(TRANSFER_DTYPE)
        assert sum(call.lens) <= node_ids.GATE_PASS and max(call.lens) <= 128  # one pass, one sub-pass
        assert np.all(_homes(t["id_lo"], 2) == 0) and np.all(_homes(t["credit_account_id_lo"], 2) == 0)
        assert np.all(_homes(t["debit_account_id_lo"], 2) == 1)
        assert len(np.unique(t["debit_account_id_lo"])) == len(t)  # no two lanes import one id
        codes = _codes(rep)
        if ids:
            assert ids == set(t["debit_account_id_lo"].tolist()) and len(codes) == 0
        else:
            assert len(codes) == len(t) and np.all(codes == R.debit_account_not_found)
        seen |= ids
    assert len(seen) == target + node_ids.GATE_PASS + node_ids.GATE_LATE
