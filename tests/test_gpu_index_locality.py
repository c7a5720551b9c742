"""The clustered transfer index (csrc/tb_device.h tb_xi_home: the ids of a group share a 64-byte
segment, probes stride from segment to segment) under id families that stress it, against the
oracle byte for byte: replies, accounts, transfers, the posted groove, commit_timestamp.

64 accounts, transfers_max = 16384: an index of 32768 entries, 4096 segments of 8.  Families:
sequential, reversed (the benchmark's), k << 3 and k << 16 (every id a group of its own, low bits
constant), lo constant with hi = k, and a 64-bit bijective scramble of k.
"""
import numpy as np
import pytest

from tests.harness.configs import timestamps
from tests.harness.oracle import OracleEngine
from tests.test_gpu_differential import assert_same_state
from tests.test_index_home import FAMILIES, group_size, homes
from tigerbeetle_amd.types import ACCOUNT_DTYPE, RESULT_DTYPE, TRANSFER_DTYPE

pytestmark = pytest.mark.gpu

N_ACCT, T_MAX, CAP, PREP = 64, 16384, 32768, 2048
U64 = (1 << 64) - 1
MAXINT = (1 << 128) - 1
CT_LEDGER_MUST_NOT_BE_ZERO, CT_SAME_LEDGER_AS_ACCOUNTS, CT_EXISTS = 19, 24, 46
CT_EXISTS_WITH_DIFFERENT = range(36, 46)
TF_PENDING = 2


def _mix64(x):
    x &= U64
    x ^= x >> 31
    x = (x * 0x7fb5d329728ea185) & U64
    x ^= x >> 27
    x = (x * 0x81dadef4bc2dd44d) & U64
    return x ^ (x >> 33)


def family_id(family, k):
    """Id k (k >= 0) of a family: never 0, never maxInt."""
    return {
        "sequential": lambda: k + 1,
        "reversed": lambda: MAXINT - (k + 1),
        "shl3": lambda: (k + 1) << 3,
        "shl16": lambda: (k + 1) << 16,
        "hi": lambda: ((k + 1) << 64) | 0x1234567,
        "scramble": lambda: _mix64(k + 0x9e3779b97f4a7c15) or 1,
    }[family]()


def make_transfers(ids, salt=0):
    t = np.zeros(len(ids), dtype=TRANSFER_DTYPE)
    k = np.arange(len(ids), dtype=np.uint64) + np.uint64(salt)
    t["id_lo"] = np.array([i & U64 for i in ids], dtype=np.uint64)
    t["id_hi"] = np.array([i >> 64 for i in ids], dtype=np.uint64)
    t["debit_account_id_lo"] = 1 + k % N_ACCT
    t["credit_account_id_lo"] = 1 + (k + 1 + k // N_ACCT % (N_ACCT - 1)) % N_ACCT
    t["amount_lo"] = 1 + k % 1000
    t["user_data_64"] = k
    t["ledger"] = 1
    t["code"] = 1
    assert not (t["debit_account_id_lo"] == t["credit_account_id_lo"]).any()
    return t


def alter(t):
    """Copies of stored transfers with one field changed each: the exists_with_different_* codes."""
    a = t.copy()
    k = np.arange(len(a))
    a["flags"][k % 8 == 0] = TF_PENDING
    m = k % 8 == 1
    a["debit_account_id_lo"][m] = 1 + (a["debit_account_id_lo"][m] + 1) % N_ACCT
    m = k % 8 == 2
    a["credit_account_id_lo"][m] = 1 + (a["credit_account_id_lo"][m] + 1) % N_ACCT
    a["amount_lo"][k % 8 == 3] += 5
    a["user_data_128_lo"][k % 8 == 4] = 9
    a["user_data_64"][k % 8 == 5] += 1 << 40
    a["user_data_32"][k % 8 == 6] = 3
    a["code"][k % 8 == 7] = 2
    a = a[a["debit_account_id_lo"] != a["credit_account_id_lo"]]
    return a


def setup_pair(factory):
    """A fresh engine and oracle with the 64 accounts created; returns (oracle, engine, next timestamp)."""
    oracle = OracleEngine(N_ACCT, T_MAX)
    engine = factory(accounts_max=N_ACCT, transfers_max=T_MAX, pass_events_max=8192, pass_batches_max=8)
    a = np.zeros(N_ACCT, dtype=ACCOUNT_DTYPE)
    a["id_lo"] = np.arange(1, N_ACCT + 1)
    a["ledger"] = 1
    a["code"] = 1
    t = 10**12
    for e in (oracle, engine):
        assert e.commit(128, t, a.tobytes()) == b""
    return oracle, engine, t


def commit_both(oracle, engine, t, prepares, calls=None):
    """Commit the prepares (record arrays) on both; `calls` groups them into commit_many calls on
    the engine (default: one call, one device pass).  Returns (replies, next timestamp)."""
    lens = [len(p) for p in prepares]
    ts, t_next = timestamps(lens, t + 10)
    bodies = [p.tobytes() for p in prepares]
    expected = oracle.commit_many(129, ts, bodies)
    actual, at = [], 0
    for n in calls or [len(prepares)]:
        actual += engine.commit_many(129, ts[at:at + n], bodies[at:at + n])
        at += n
    assert at == len(prepares)
    for k, (e, a) in enumerate(zip(expected, actual)):
        assert e == a, "reply of prepare %d differs" % k
    return expected, t_next


def codes(reply):
    return np.frombuffer(reply, dtype=RESULT_DTYPE)["result"]


def fill_prepares(family, n_prepares, first=0):
    return [make_transfers([family_id(family, first + p * PREP + k) for k in range(PREP)], salt=p * PREP)
            for p in range(n_prepares)]


def test_layout_is_the_one_under_test():
    assert group_size() == 8 and CAP // group_size() == 4096


@pytest.mark.parametrize("family", FAMILIES)
def test_fill_to_capacity(family, gpu_engine_factory):
    """The log filled to transfers_max (the index at its contract's load of 1/2): four prepares in one
    device pass, then four passes of one prepare, so claims meet entries of their own and of earlier
    passes.  No panic, every reply empty, the oracle's state."""
    oracle, engine, t = setup_pair(gpu_engine_factory)
    replies, _ = commit_both(oracle, engine, t, fill_prepares(family, T_MAX // PREP), calls=[4, 1, 1, 1, 1])
    assert all(r == b"" for r in replies)
    assert engine.stats()["transfers"] == T_MAX
    assert_same_state(oracle, engine)


# Fresh ids whose homes are known, shared by the families: ids no family holds (bit 126 set, bit
# 127 clear: below every reversed id, above every other family's).
_POOL = {}


def pool():
    if not _POOL:
        ids = [(1 << 126) | (_mix64(k) << 20) | k for k in range(400_000)]
        _POOL["ids"], _POOL["homes"] = ids, homes(ids, CAP)
    return _POOL["ids"], _POOL["homes"]


@pytest.mark.parametrize("family", FAMILIES)
def test_exists_and_collisions(family, gpu_engine_factory):
    G = group_size()
    oracle, engine, t = setup_pair(gpu_engine_factory)
    fill = fill_prepares(family, 4)
    stored = [family_id(family, k) for k in range(4 * PREP)]
    stored_set = set(stored)
    # Four segments made full for certain: pool ids added whose homes are the entries of those segments
    # that no stored id has as its home (an id's home entry is occupied once the id is stored, by
    # itself or by an earlier id that it then follows to the next segment).
    occupied = set(homes(stored, CAP))
    p_ids, p_homes = pool()
    by_home = {}
    for i, h in zip(p_ids, p_homes):
        by_home.setdefault(h, []).append(i)
    targets = [seg for seg in sorted({h // G for h in occupied})
               if all(len(by_home.get(e, [])) >= 2 for e in range(seg * G, seg * G + G))][:4]
    assert len(targets) == 4
    fillers, colliders = [], []
    for seg in targets:
        for entry in range(seg * G, seg * G + G):
            cands = by_home[entry]
            if entry not in occupied:
                fillers.append(cands[0])
            colliders.append(cands[1])  # its home is occupied: it probes on, a segment at a time
    replies, t = commit_both(oracle, engine, t, fill + [make_transfers(fillers or [p_ids[0]], salt=77)])
    assert all(r == b"" for r in replies)

    again = fill[0]
    altered = alter(fill[1])
    mates = []
    for i in stored[:256:3] + stored[-64:]:
        mates += [i - 1, i + 1] + [(i & ~(G - 1)) + j for j in range(G)]
    mates = [i for i in dict.fromkeys(mates) if 0 < i < MAXINT and i not in stored_set][:512]
    assert mates, "no fresh group-mates"
    groups = {i >> 3 for i in stored}
    assert all((i >> 3) in groups or i - 1 in stored_set or i + 1 in stored_set for i in mates)
    fresh = make_transfers(mates + colliders, salt=5)
    mixed = np.concatenate([again, altered, fresh])
    rng = np.random.default_rng(11)
    mixed = mixed[rng.permutation(len(mixed))]
    (reply,), _ = commit_both(oracle, engine, t, [mixed])
    got = codes(reply)
    assert len(got) == len(again) + len(altered), "fresh ids were refused, or stored ones accepted"
    assert (got == CT_EXISTS).sum() == len(again)
    different = set(got[got != CT_EXISTS].tolist())
    assert different <= set(CT_EXISTS_WITH_DIFFERENT) and len(different) >= 6, different
    assert_same_state(oracle, engine)


@pytest.mark.parametrize("family", FAMILIES)
def test_same_pass_duplicates_and_withdrawn_claims(family, gpu_engine_factory):
    oracle, engine, t = setup_pair(gpu_engine_factory)
    replies, t = commit_both(oracle, engine, t, fill_prepares(family, 1))
    assert replies == [b""]

    # One prepare, every id twice: adjacent, 7 apart, 2047 apart.
    ids = [family_id(family, 10_000 + k) for k in range(1024 + 1022 + 2047)]
    adjacent = [i for i in ids[:1024] for _ in (0, 1)]
    seven = []
    for b in range(0, 1022, 7):
        seven += ids[1024 + b:1024 + b + 7] * 2
    far = ids[2046:] * 2
    order = adjacent + seven + far
    assert len(order) == 8186 and all(order[k] == order[k + 7] for k in range(2048, 2048 + 7))
    assert order[4092] == order[4092 + 2047]
    # both copies identical (the second returns exists): the fields follow the id, not the position
    first_at = {}
    for k, i in enumerate(order):
        first_at.setdefault(i, k)
    dup = make_transfers(order)
    dup = dup[[first_at[i] for i in order]]
    before = engine.stats()["dependent_events"]
    (reply,), t = commit_both(oracle, engine, t, [dup])
    got = np.frombuffer(reply, dtype=RESULT_DTYPE)
    assert len(got) == len(order) // 2 and (got["result"] == CT_EXISTS).all()
    assert sorted(got["index"].tolist()) == sorted(k for k, i in enumerate(order) if first_at[i] != k)
    assert engine.stats()["dependent_events"] - before == len(order), "a duplicate pair was not made dependent"
    assert_same_state(oracle, engine)

    # Withdrawn claims: the second half of a prepare fails, on ledger = 0 (before its claim) and on a
    # ledger that is not the accounts' (after it: the claim is withdrawn, a tombstone on the chain);
    # a later prepare reuses those ids and is accepted.
    ids = [family_id(family, 30_000 + k) for k in range(PREP)]
    bad = make_transfers(ids)
    bad["ledger"][PREP // 2::2] = 0
    bad["ledger"][PREP // 2 + 1::2] = 7
    (reply,), t = commit_both(oracle, engine, t, [bad])
    got = np.frombuffer(reply, dtype=RESULT_DTYPE)
    assert got["index"].tolist() == list(range(PREP // 2, PREP))
    assert set(got["result"].tolist()) == {CT_LEDGER_MUST_NOT_BE_ZERO, CT_SAME_LEDGER_AS_ACCOUNTS}
    reuse = make_transfers(ids[PREP // 2:], salt=3)
    (reply,), t = commit_both(oracle, engine, t, [reuse])
    assert reply == b"", "a withdrawn id was not accepted again"
    assert_same_state(oracle, engine)


@pytest.mark.parametrize("inplace", [True, False], ids=["in_place", "copied"])
def test_sequential_fill_from_hbm(inplace, gpu_engine_factory):
    """The sequential family to capacity through commit_device_async: in place (tbgpu_log_window) and
    from a separate HBM buffer (the copy commit), two prepares a call."""
    oracle, engine, t = setup_pair(gpu_engine_factory)
    prepares = fill_prepares("sequential", T_MAX // PREP)
    lens = [len(p) for p in prepares]
    ts, _ = timestamps(lens, t + 10)
    expected = oracle.commit_many(129, ts, [p.tobytes() for p in prepares])
    res_dev, rb_dev, buf = engine.alloc(2 * PREP * 8), engine.alloc(8), engine.alloc(2 * PREP * 128)
    for k in range(0, len(prepares), 2):
        body = np.frombuffer(prepares[k].tobytes() + prepares[k + 1].tobytes(), dtype=np.uint8)
        src = engine.log_window(2 * PREP) if inplace else buf
        engine.to_device(src, body)
        engine.commit_device_async(129, ts[k:k + 2], lens[k:k + 2], src, res_dev, rb_dev)
        engine.sync()
        assert not engine.to_host(rb_dev, 8).view(np.uint32).any(), "a reply is not empty"
    assert all(r == b"" for r in expected)
    assert engine.stats()["transfers"] == T_MAX
    assert_same_state(oracle, engine)
