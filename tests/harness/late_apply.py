"""One create_transfers pass built to race tb_flow's late balance adds against its in-kernel
sequential replay (csrc/k_flow.h tb_flow, k_apply.h tb_apply_late, k_replay.h rp_create_transfer) —
test infrastructure only.

The pass is 64 prepares x 8190 events over 8 plain accounts (no limit flag, no balancing).  Every
prepare starts with one linked chain of 70 transfers — longer than FLOW_CHAIN_MAX = 64, so the planner
declines the pass and one thread replays its dependent events in order with whole-balance loads and
stores.  Member 0 of a chain is a pending transfer and member 35 posts it, which makes the chain
dependent; in every second prepare the last member fails with accounts_must_be_different, so the
replay rolls 69 applied members back from their before-images.  Every other event is an independent
plain transfer between two of the same 8 accounts: the adds tb_flow applies itself ("late").  With
1024 threads a workgroup, a launch of more than 256 workgroups hands the events from pass index
262,144 on to workgroups past the 256 an MI355X holds at once, which start only when others have left
— on a pass that replays sequentially, while the replay runs.

A chain runs between four accounts: 0-3 in prepares 0, 1 (mod 4), 4-7 in prepares 2, 3 (mod 4), so that
committed and rolled-back chains together name every account the independent events name.

Variants:
  small     as above, amounts 1..1000;
  postvoid  an earlier pass creates 200,000 pending transfers, and two of five independent events of
            the main pass post or void one of them (the late set of a legs pass);
  wide      independent amounts 2^70 + 1..1000: the pass keeps the global overflow certificate and
            loses the 64-bit one, so the late adds are two-word adds.
Everything is a pure function of the variant; the only random numbers are the amounts (fixed seed)."""
import numpy as np

from tests.harness.configs import batches, timestamps
from tests.harness.workload import account_id
from tigerbeetle_amd.types import TRANSFER_DTYPE, U64_MAX, CreateTransferResult as R, TransferFlags as TF, pack_account

VARIANTS = ("small", "postvoid", "wide")
PREPARES = 64
BATCH = 8190
CHAIN = 70            # > FLOW_CHAIN_MAX (64)
CHAIN_POST = 35       # the member that posts member 0
N_ACCOUNTS = 8
LATE_FROM = 262_144   # 256 workgroups x 1024 threads: the first pass index of workgroup 256
PENDINGS = 200_000
EVENTS = PREPARES * BATCH
INDEPENDENT = BATCH - CHAIN
AMOUNT_SEED = 20
FIRST_ID = 1_000_000          # main pass: event g has id FIRST_ID + g
FIRST_PENDING_ID = 10_000_000  # postvoid's earlier pass: pending k has id FIRST_PENDING_ID + k
START_TS = 10**12

LINKED, PENDING = int(TF.linked), int(TF.pending)
POST, VOID = int(TF.post_pending_transfer), int(TF.void_pending_transfer)


def _set_accounts(rec, name, index):
    """rec[name] = account_id(index), element-wise (ids U128_MAX - 1 - index: the high word is all ones)."""
    rec[name + "_lo"] = np.uint64(U64_MAX - 1) - np.asarray(index, dtype=np.uint64)
    rec[name + "_hi"] = U64_MAX


def _pair(q):
    """Two different accounts of the 8 for ordinal q: every ordered pair comes up."""
    q = np.asarray(q, dtype=np.uint64)
    dr = q % 8
    return dr, (dr + 1 + (q // 8) % 7) % 8


def _pending_amounts():
    return 1 + (np.arange(PENDINGS, dtype=np.uint64) * 13) % 1000


class LateApply:
    """variant, accounts (one create_accounts prepare), setup (create_transfers prepares committed
    before the pass: postvoid's pending transfers), and the pass: events (TRANSFER_DTYPE[EVENTS]),
    lens, timestamps, bodies; chain / broken / failing: masks over the pass's events."""

    def __init__(self, variant):
        assert variant in VARIANTS
        self.variant = variant
        self.account_ids = [account_id(i) for i in range(N_ACCOUNTS)]
        self.accounts_body = b"".join(pack_account(id=a, ledger=1, code=1) for a in self.account_ids)
        self.accounts_ts = START_TS
        t = START_TS
        self.setup_lens, self.setup_ts, self.setup_bodies = [], [], []
        if variant == "postvoid":
            rec = np.zeros(PENDINGS, dtype=TRANSFER_DTYPE)
            k = np.arange(PENDINGS, dtype=np.uint64)
            rec["id_lo"] = FIRST_PENDING_ID + k
            dr, cr = _pair(k)
            _set_accounts(rec, "debit_account_id", dr)
            _set_accounts(rec, "credit_account_id", cr)
            rec["amount_lo"] = _pending_amounts()
            rec["ledger"], rec["code"], rec["flags"] = 1, 1, PENDING
            self.setup_lens = batches(PENDINGS, BATCH)
            self.setup_ts, t = timestamps(self.setup_lens, t + 10)
            self.setup_bodies = _split(rec, self.setup_lens)
        self.lens = [BATCH] * PREPARES
        self.timestamps, _ = timestamps(self.lens, t + 10)
        self.events = self._pass()
        self.bodies = _split(self.events, self.lens)
        self.first_ts = self.timestamps[0] - BATCH + 1

    def _pass(self):
        rec = np.zeros(EVENTS, dtype=TRANSFER_DTYPE)
        g = np.arange(EVENTS, dtype=np.uint64)
        p, i = g // BATCH, g % BATCH
        rec["id_lo"] = FIRST_ID + g
        rec["ledger"], rec["code"] = 1, 1
        self.chain = i < CHAIN
        self.broken = self.chain & (p % 2 == 1)
        self.failing = self.broken & (i == CHAIN - 1)
        # Independent events: ordinal q over the pass.
        ind = ~self.chain
        q = (p * INDEPENDENT + (i - CHAIN))[ind]
        dr, cr = _pair(q)
        amount = np.random.default_rng(AMOUNT_SEED).integers(1, 1001, size=len(q), dtype=np.uint64)
        lo, hi = amount, np.zeros(len(q), dtype=np.uint64)
        if self.variant == "wide":
            hi[:] = 1 << (70 - 64)
        flags = np.zeros(len(q), dtype=np.uint16)
        pid = np.zeros(len(q), dtype=np.uint64)
        self.postvoid = np.zeros(EVENTS, dtype=bool)
        if self.variant == "postvoid":
            # Two of five independent events settle pending r = their rank among those, each once:
            # even r posts (all of it, or the larger half), odd r voids.
            r = (q // 5) * 2 + q % 5
            pv = (q % 5 < 2) & (r < PENDINGS)
            r = r[pv]
            pamt = _pending_amounts()[r]
            flags[pv] = np.where(r % 2 == 0, POST, VOID).astype(np.uint16)
            pid[pv] = FIRST_PENDING_ID + r
            lo[pv] = np.where(r % 4 == 2, (pamt + 1) // 2, 0)
            self.postvoid[np.flatnonzero(ind)[pv]] = True
        rec["amount_lo"][ind], rec["amount_hi"][ind] = lo, hi
        rec["flags"][ind], rec["pending_id_lo"][ind] = flags, pid
        sub = rec[ind]
        _set_accounts(sub, "debit_account_id", dr)
        _set_accounts(sub, "credit_account_id", cr)
        if self.variant == "postvoid":  # a post / void names its accounts through its pending transfer
            for name in ("debit_account_id_lo", "debit_account_id_hi", "credit_account_id_lo", "credit_account_id_hi",
                         "ledger", "code"):
                sub[name][pv] = 0
        rec[ind] = sub
        # Chains.
        ch = np.flatnonzero(self.chain)
        pc, j = p[ch], i[ch]
        group = 4 * ((pc >> np.uint64(1)) & np.uint64(1))
        sub = rec[ch]
        _set_accounts(sub, "debit_account_id", group + j % 4)
        _set_accounts(sub, "credit_account_id", group + (j % 4 + 1 + (j // 4) % 3) % 4)
        sub["amount_lo"] = 1 + (j * 7 + pc) % 1000
        sub["flags"] = np.where(j == CHAIN - 1, 0, LINKED).astype(np.uint16)
        head, post = j == 0, j == CHAIN_POST
        sub["flags"][head] |= PENDING
        sub["amount_lo"][head] = 20 + pc[head]
        sub["flags"][post] |= POST
        sub["pending_id_lo"][post] = FIRST_ID + (pc[post] * BATCH)
        for name in ("debit_account_id_lo", "debit_account_id_hi", "credit_account_id_lo", "credit_account_id_hi",
                     "amount_lo", "ledger", "code"):
            sub[name][post] = 0
        fail = (j == CHAIN - 1) & (pc % 2 == 1)  # accounts_must_be_different
        sub["credit_account_id_lo"][fail] = sub["debit_account_id_lo"][fail]
        rec[ch] = sub
        return rec

    @property
    def accounts(self):
        """{id: (flags, ledger)} for tests.harness.dependence.dependent_count."""
        return {a: (0, 1) for a in self.account_ids}

    @property
    def existing_ids(self):
        return frozenset(range(FIRST_PENDING_ID, FIRST_PENDING_ID + PENDINGS)) if self.setup_bodies else frozenset()

    def expected_replies(self):
        """The reply of each prepare of the pass, as the builder claims it: a broken chain's members
        linked_event_failed, its last member accounts_must_be_different, every other event ok."""
        out = []
        for k in range(PREPARES):
            if k % 2 == 0:
                out.append(b"")
                continue
            rows = [(j, int(R.linked_event_failed)) for j in range(CHAIN - 1)]
            rows.append((CHAIN - 1, int(R.accounts_must_be_different)))
            out.append(np.array(rows, dtype=np.uint32).tobytes())
        return out

    def commit_setup(self, engine):
        """The accounts and the earlier pass on `engine` (an OracleEngine or an Engine)."""
        assert engine.commit(128, self.accounts_ts, self.accounts_body) == b""
        if self.setup_bodies:
            assert all(r == b"" for r in engine.commit_many(129, self.setup_ts, self.setup_bodies))


def _split(rec, lens):
    out, off = [], 0
    for L in lens:
        out.append(rec[off:off + L].tobytes())
        off += L
    return out
