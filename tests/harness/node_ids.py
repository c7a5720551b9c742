"""Ids by home, and the skewed node workloads built from them — TEST INFRASTRUCTURE ONLY (host code,
no device: tbgpu_homes is the library's host restatement of tb_home).

A node places a transfer on home(id) and an account on owner(id), the same hash (csrc/node.h).  Ids
that hash evenly give every shard 1/N of every pass; the pools here put every transfer of a pass on
one home, or every account on one owner, so that a home receives several routed sub-passes (or none),
an owner applies every leg (or none), and a home's import gate is driven to its boundary.
"""
import numpy as np

from tigerbeetle_amd.types import ACCOUNT_DTYPE, TRANSFER_DTYPE

from .configs import timestamps
from .shard_double import homes_of

CREATE_ACCOUNTS, CREATE_TRANSFERS = 128, 129


def ids_homed(world, shard, n, start=1):
    """The first n ids (hi word 0) at or above `start` whose home among `world` shards is `shard`,
    ascending."""
    assert 0 <= shard < world and start >= 1
    out, have, lo = [], 0, int(start)
    while have < n:
        span = max(1024, 2 * world * (n - have))
        ids = np.arange(lo, lo + span, dtype=np.uint64)
        mine = ids[homes_of(np.stack([ids, np.zeros_like(ids)], axis=1), world) == shard]
        out.append(mine)
        have += len(mine)
        lo += span
    return np.concatenate(out)[:n] if out else np.zeros(0, dtype=np.uint64)


class IdPlan:
    """Renames a scenario's ids (workload.make_scenario's transfer_id_of / account_id_of): every
    transfer id onto home `transfer_home`, every account id onto owner `account_owner` (None: left as
    it is).  Each id takes the pool's next id when first seen; 0 stays 0 (the invalid id, and the unset
    pending_id and account ids of a post / void)."""

    def __init__(self, world, transfer_home=None, account_owner=None, n_transfers=4096, n_accounts=512):
        self.world = world
        self._pool = {"t": ids_homed(world, transfer_home, n_transfers) if transfer_home is not None else None,
                      "a": ids_homed(world, account_owner, n_accounts, start=1 << 32)
                      if account_owner is not None else None}
        self._seen = {"t": {}, "a": {}}

    def _of(self, kind, i):
        pool, seen = self._pool[kind], self._seen[kind]
        if pool is None or i == 0:
            return i
        if i not in seen:
            assert len(seen) < len(pool), "IdPlan: pool exhausted"
            seen[i] = int(pool[len(seen)])
        return seen[i]

    def transfer_id_of(self, i):
        return self._of("t", i)

    def account_id_of(self, i):
        return self._of("a", i)

    def transfer_ids(self):
        return sorted(self._seen["t"].values())

    def account_ids(self):
        return sorted(self._seen["a"].values())


# -- skewed workloads ------------------------------------------------------------------------------

class Call:
    """One commit_many / commit_pipelined call: prepares of one operation."""

    def __init__(self, op, ts, lens, events):
        self.op, self.ts, self.lens = op, list(ts), list(lens)
        self.events = np.ascontiguousarray(events).view(np.uint8).reshape(-1)  # the prepares back to back
        assert self.events.nbytes == 128 * sum(self.lens)

    def bodies(self):
        out, off = [], 0
        for L in self.lens:
            out.append(self.events[off * 128:(off + L) * 128].tobytes())
            off += L
        return out


class Skew:
    def __init__(self):
        self.calls = []
        self.account_ids = np.zeros(0, dtype=np.uint64)  # every account created (lo words; hi 0)
        self.t = 10**12

    def add(self, op, lens, events):
        ts, self.t = timestamps(lens, self.t + 10)
        self.calls.append(Call(op, ts, lens, events))
        return self.calls[-1]


def accounts_of(ids, ledger=1):
    a = np.zeros(len(ids), dtype=ACCOUNT_DTYPE)
    a["id_lo"] = ids
    a["ledger"], a["code"] = ledger, 7
    return a


def transfers_of(ids, debits, credits, amounts, ledger=1):
    t = np.zeros(len(ids), dtype=TRANSFER_DTYPE)
    t["id_lo"], t["debit_account_id_lo"], t["credit_account_id_lo"], t["amount_lo"] = ids, debits, credits, amounts
    t["ledger"], t["code"] = ledger, 1
    return t


def _prepares(n, size):
    q, r = divmod(n, size)
    return [size] * q + ([r] if r else [])


def _pairs(rng, pool, n, head=None):
    """n (debit, credit) pairs of distinct accounts from the ascending pool; head: half of the legs go
    to its accounts."""
    def pick():
        ids = rng.choice(pool, n)
        if head is not None:
            ids = np.where(rng.random(n) < 0.5, rng.choice(head, n), ids)
        return ids
    dr, cr = pick(), pick()
    return dr, np.where(cr == dr, pool[(np.searchsorted(pool, dr) + 1) % len(pool)], cr)


HOME_SKEW = dict(world=4, pass_events_max=4096, pass_batches_max=4, accounts_max=6000, transfers_max=1 << 17)
HOME_SKEW_PASS = HOME_SKEW["world"] * HOME_SKEW["pass_events_max"]  # 16384: what the target home receives whole


def home_skew(target, seed=1):
    """Section A: two full passes (16384 events each, prepares of 1024) and a ragged one (7 events and
    an empty prepare) in one call, every transfer homed on `target` of 4 shards, over 3000 accounts
    with even owners; then a call with even ids over the same accounts.  The second pass repeats ids of
    the first (exists, and exists_with_different_amount for half of them); both passes hold duplicate
    ids with one copy in the home's first sub-pass (receipt positions below 8190) and one past it;
    a few events carry a timestamp (answered at the source: the send slots shift against the receipt),
    a few name an account no shard holds, a few have amount_hi != 0."""
    W, P = HOME_SKEW["world"], HOME_SKEW_PASS
    rng = np.random.default_rng(100 * seed + target)
    sk = Skew()
    sk.account_ids = np.arange(1, 3001, dtype=np.uint64)
    sk.add(CREATE_ACCOUNTS, _prepares(3000, 1000), accounts_of(sk.account_ids))
    pool = ids_homed(W, target, 2 * P + 7)
    dr, cr = _pairs(rng, sk.account_ids, 2 * P + 7)
    t = transfers_of(pool, dr, cr, rng.integers(1, 50, 2 * P + 7))
    for base in (0, P):
        k = base + rng.choice(P, 120, replace=False)
        t["timestamp"][k[:40]] = 7
        t["debit_account_id_lo"][k[40:60]] = 900_000 + k[40:60]  # no shard holds it
        t["credit_account_id_lo"][k[60:80]] = 900_000 + k[60:80]
        t["amount_hi"][k[80:120]] = rng.integers(1, 4, 40)
        # Same-pass duplicates across the home's sub-passes: positions 100.. and 13000.. of the pass.
        src, dst = base + 100 + np.arange(60), base + 13000 + np.arange(60)
        t[dst] = t[src]
        t["amount_lo"][dst[:30]] += 1
    # The second pass repeats 600 ids of the first.
    dst = P + 200 + rng.choice(P - 400, 600, replace=False)
    dst = dst[(dst < P + 13000) | (dst >= P + 13060)]
    src = rng.choice(P, len(dst), replace=False)
    t[dst] = t[src]
    t["amount_lo"][dst[:len(dst) // 2]] += 1
    sk.add(CREATE_TRANSFERS, [1024] * 32 + [7, 0], t)
    dr, cr = _pairs(rng, sk.account_ids, 2000)
    back = transfers_of(np.arange(10_000_000, 10_002_000, dtype=np.uint64), dr, cr, rng.integers(1, 50, 2000))
    back[1990:] = t[300:310]  # ids of the skewed call once more
    back["debit_account_id_lo"][50:60] = 900_000
    sk.add(CREATE_TRANSFERS, [1000, 1000], back)
    return sk


OWNER_SKEW = dict(world=3, pass_events_max=4000, pass_batches_max=2, accounts_max=4096, transfers_max=1 << 17)


def owner_skew(owners, seed=1):
    """Section B: 3000 accounts owned by the shards `owners` of 3 only (one owner: it applies every
    leg and the other homes import every account they name; two: the third owns nothing), 36000
    transfers with even ids in prepares of 2000 (two calls of a full pass and a ragged one each).
    Twenty accounts take half the legs; one amount in ten is near 2^62 (the hot balances cross 2^64
    by carry) and a few have amount_hi != 0; a few name a missing account or repeat an id."""
    W = OWNER_SKEW["world"]
    rng = np.random.default_rng(7 * seed + sum(owners))
    sk = Skew()
    per = 3000 // len(owners)
    sk.account_ids = np.sort(np.concatenate([ids_homed(W, o, per) for o in owners]))
    sk.add(CREATE_ACCOUNTS, _prepares(len(sk.account_ids), 1000), accounts_of(sk.account_ids))
    head = rng.choice(sk.account_ids, 20, replace=False)
    n = 36000
    dr, cr = _pairs(rng, sk.account_ids, n, head=head)
    amounts = rng.integers(1, 1000, n).astype(np.uint64)
    wide = rng.random(n) < 0.1
    amounts[wide] += np.uint64(1 << 62)
    t = transfers_of(np.arange(1, n + 1, dtype=np.uint64), dr, cr, amounts)
    k = rng.choice(n, 300, replace=False)
    t["amount_hi"][k[:100]] = rng.integers(1, 3, 100)
    t["debit_account_id_lo"][k[100:150]] = (1 << 40) + k[100:150]
    t["credit_account_id_lo"][k[150:200]] = (1 << 40) + k[150:200]
    dup = k[200:300][k[200:300] >= 4000]
    t[dup] = t[rng.integers(0, 4000, len(dup))]
    t["amount_lo"][dup[:len(dup) // 2]] += 1
    half = n // 2
    for lo in (0, half):
        sk.add(CREATE_TRANSFERS, _prepares(half, 2000), t[lo:lo + half])
    return sk


GATE = dict(world=2, pass_events_max=512, pass_batches_max=4, accounts_max=16384, transfers_max=1 << 15)
GATE_ROOM, GATE_PASS, GATE_LATE = 2048, 1024, 256


def gate_fill(target, room=GATE_ROOM, n_max=GATE_PASS):
    """Sub-pass sizes that raise a home's live imports from 0 towards `target`, one new foreign account
    per event, without a flush under the gate's rule (flush before a sub-pass of n events when
    live + 2 n > room) for as long as that is possible: each step takes min(n_max, what is missing,
    (room - live) / 2).  Past room - 1 no step fits: the last step then adds what is missing and the
    rule flushes before it."""
    steps, live = [], 0
    while live < target:
        n = min(n_max, target - live, (room - live) // 2)
        if n == 0:
            steps.append(target - live)
            break
        steps.append(n)
        live += n
    return steps


def gate_boundary(target, seed=1):
    """Section D: 2 shards, every transfer homed on shard 0, debiting a foreign account (owner 1) that
    no other event of its pass names and crediting an account shard 0 owns.  Steps (one call, one pass,
    one sub-pass of home 0 each; prepares of 128): gate_fill(target), then 1024 foreign accounts never
    named before, then the first 1024 again, then 256 ids no owner holds, then those accounts created
    (every import flushed), then named again.  Returns (Skew, per call the existing foreign ids it
    names or None for the create_accounts calls)."""
    W = GATE["world"]
    rng = np.random.default_rng(seed)
    sk = Skew()
    late = ids_homed(W, 1, GATE_LATE, start=100_000)
    early = np.arange(1, GATE["accounts_max"] - GATE_LATE + 1, dtype=np.uint64)
    owner = homes_of(np.stack([early, np.zeros_like(early)], axis=1), W)
    mine, foreign = early[owner == 0], early[owner == 1]
    sk.account_ids = np.concatenate([early, late])
    named = [None]
    sk.add(CREATE_ACCOUNTS, _prepares(len(early), 1000), accounts_of(early))  # (the sequencer's pass: 1024 events)
    tids = iter(ids_homed(W, 0, 8192))
    used = [0]

    def step(debits, existing=True):
        n = len(debits)
        ids = np.array([next(tids) for _ in range(n)], dtype=np.uint64)
        sk.add(CREATE_TRANSFERS, _prepares(n, 128), transfers_of(ids, debits, rng.choice(mine, n), rng.integers(1, 50, n)))
        named.append(set(int(x) for x in debits) if existing else set())

    def fresh(n):
        used[0] += n
        assert used[0] <= len(foreign)
        return foreign[used[0] - n:used[0]]

    for n in gate_fill(target):
        step(fresh(n))
    step(fresh(GATE_PASS))
    step(foreign[:GATE_PASS])
    step(late, existing=False)
    sk.add(CREATE_ACCOUNTS, [GATE_LATE], accounts_of(late))
    named.append(None)
    step(late)
    return sk, named


DIRTY_SKEW_WORLD = 3


def dirty_skew(config, variant, seed=1):
    """Section C: a dirty workload (make_scenario's kwargs `config`: limit accounts, chains, two-phase)
    on 3 shards with every transfer id homed on shard 2 ("home": the sequencer writes every transfer it
    creates back to one home) or every account owned by shard 1 ("owner")."""
    from .workload import make_scenario
    plan = IdPlan(DIRTY_SKEW_WORLD, transfer_home=2 if variant == "home" else None,
                  account_owner=1 if variant == "owner" else None)
    sc = make_scenario(seed, transfer_id_of=plan.transfer_id_of, account_id_of=plan.account_id_of, **config)
    return sc, plan


def run_skew_oracle(sk, oracle):
    """Every call's replies (one bytes per prepare) from the oracle."""
    return [oracle.commit_many(c.op, c.ts, c.bodies()) for c in sk.calls]
