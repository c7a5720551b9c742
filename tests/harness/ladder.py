"""Deterministic scenarios that reach every create_transfers / create_accounts result code and probe
the ORDER of the reference's checks (state_machine.zig create_account :738-777, create_transfer
:779-905, post_or_void_pending_transfer :907-1077) by breaking two rules in one event.

The engine restates that order three times (k_validate.h, k_replay.h with FLOW = false and true) and
once more as the rule that decides whether kernel 1's code may be trusted (k_resolve.h tb_classify);
the scenarios here put the same events on each of those paths.  No random draws and no balance
writes: every balance is built by committed transfers, so tb_flow stays on.

A *mutation* is a named edit of a valid *base event* that alone yields one result code.  The families:

  singles           every mutation alone, one create_accounts and one create_transfers prepare
  pairs             every pair of mutations that fits one base event, applied together
  late_clock        the singles and the overflow / timeout / limit pairs with every timestamp from
                    2^64 - 10^16 on (bit 63 set), where overflows_timeout is reachable
  ordered           the singles and, per code, a few of the pairs the oracle resolved to it, each in
                    a linked chain with a valid transfer that debits a limit account (dependent, so
                    the chain is judged by k_replay.h's ladder)
  ordered_late      the same for the late_clock events (overflows_timeout on the ordered path)
  same_pass_exists  every exists* code with its first instance stored by an earlier call, in an
                    earlier prepare of the same call, and earlier in the same prepare

overflows_timeout needs a prepare timestamp within 2^32 s of 2^64, so its mutation is `late_only`: it is
left out of the families on the ordinary clock.
"""
import numpy as np

from tests.harness.oracle import OracleEngine
from tests.harness.workload import NS, Scenario, run_oracle
from tigerbeetle_amd.types import (RESULT_DTYPE, AccountFlags as AF, CreateAccountResult as CA,
                                   CreateTransferResult as CT, TransferFlags as TF, U128_MAX, pack_account,
                                   pack_transfer)

PREPARE_MAX = 8190
LATE_START = (1 << 64) - 10**16
LEDGER, LEDGER_2 = 7, 8
HALF, QUARTER = 1 << 127, 1 << 126
TIMEOUT_MAX = (1 << 32) - 1

# -- fixture accounts ------------------------------------------------------------------------------
PLAIN = tuple(range(1, 13))          # a dozen plain accounts
A_LEDGER_2 = 13                      # the one account of the second ledger
A_DEBIT_LIMIT = 14                   # debits_must_not_exceed_credits, funded with FUNDING
A_CREDIT_LIMIT = 15                  # credits_must_not_exceed_debits, never debited
A_USER_DATA = 16                     # non-zero user_data_*: the stored account of the duplicates
A_DP, A_CP = 20, 21                  # debits_pending / credits_pending = 2^127
A_DPOST, A_CPOST = 22, 23            # debits_posted / credits_posted = 2^127
A_DSUM, A_CSUM = 24, 25              # pending = posted = 2^126 (only the sum overflows)
A_SPARE = 17                         # created after the stored transfers (ends the fixture's call)
A_MISSING = 999
FUNDING = 10**6
USER_DATA_ACCOUNT = dict(id=A_USER_DATA, ledger=LEDGER, code=2, user_data_128=5, user_data_64=6, user_data_32=7)


def _fixture_accounts():
    evs = [dict(id=i, ledger=LEDGER, code=1) for i in PLAIN]
    evs.append(dict(id=A_LEDGER_2, ledger=LEDGER_2, code=1))
    evs.append(dict(id=A_DEBIT_LIMIT, ledger=LEDGER, code=1, flags=int(AF.debits_must_not_exceed_credits)))
    evs.append(dict(id=A_CREDIT_LIMIT, ledger=LEDGER, code=1, flags=int(AF.credits_must_not_exceed_debits)))
    evs.append(dict(USER_DATA_ACCOUNT))
    evs += [dict(id=i, ledger=LEDGER, code=1) for i in (A_DP, A_CP, A_DPOST, A_CPOST, A_DSUM, A_CSUM)]
    return evs


# -- stored transfers ------------------------------------------------------------------------------
class Stored:
    """The ids of one set of stored transfers the duplicate / post / void base events refer to, and the
    events that store them.  The fixture's set has base 100; same_pass_exists makes more."""

    def __init__(self, base):
        self.posted = base            # a posted transfer with non-zero user_data_*
        self.pending_0 = base + 10    # pending, timeout 0: the post / void base events name it
        self.pending_1 = base + 11    # pending, timeout 1: expired once the clock has advanced
        self.pending_7 = base + 12    # pending, timeout 7
        self.pending_posted = base + 13   # posted by post_partial with a partial amount
        self.pending_voided = base + 14   # voided by void_1
        self.pending_eq_1 = base + 15     # two pending transfers of equal amount ...
        self.pending_eq_2 = base + 16
        self.post_partial = base + 20
        self.void_1 = base + 21
        self.post_eq_1 = base + 22        # ... and the stored post of the first

    def ev_posted(self):
        return dict(id=self.posted, debit_account_id=1, credit_account_id=2, amount=10, ledger=LEDGER, code=3,
                    user_data_128=11, user_data_64=12, user_data_32=13)

    def _pending(self, id, dr, cr, amount, timeout, code=4):
        return dict(id=id, debit_account_id=dr, credit_account_id=cr, amount=amount, ledger=LEDGER, code=code,
                    flags=int(TF.pending), timeout=timeout, user_data_128=21, user_data_64=22, user_data_32=23)

    def ev_pending_7(self):
        return self._pending(self.pending_7, 3, 4, 70, 7)

    def ev_pendings(self, which=None):
        all_ = {
            "pending_0": self._pending(self.pending_0, 3, 4, 100, 0),
            "pending_1": self._pending(self.pending_1, 3, 4, 50, 1),
            "pending_7": self.ev_pending_7(),
            "pending_posted": self._pending(self.pending_posted, 5, 6, 100, 0),
            "pending_voided": self._pending(self.pending_voided, 5, 6, 100, 0),
            "pending_eq_1": self._pending(self.pending_eq_1, 7, 8, 40, 0),
            "pending_eq_2": self._pending(self.pending_eq_2, 7, 8, 40, 0),
        }
        return [all_[k] for k in (which or all_)]

    def ev_post_partial(self):
        """Amount and user_data_* given, all different from the pending transfer's."""
        return dict(id=self.post_partial, pending_id=self.pending_posted, amount=60, flags=int(TF.post_pending_transfer),
                    user_data_128=91, user_data_64=92, user_data_32=93)

    def ev_void_1(self):
        return dict(id=self.void_1, pending_id=self.pending_voided, flags=int(TF.void_pending_transfer))

    def ev_post_eq_1(self):
        """Every defaulting field zero: stored with the pending transfer's amount and user_data_*."""
        return dict(id=self.post_eq_1, pending_id=self.pending_eq_1, flags=int(TF.post_pending_transfer))


def _fixture_balances():
    """Transfers that build the 2^127 / 2^126 balances and fund the debit-limit account."""
    def t(id, dr, cr, amount, pending=False):
        return dict(id=id, debit_account_id=dr, credit_account_id=cr, amount=amount, ledger=LEDGER, code=1,
                    flags=int(TF.pending) if pending else 0)
    return [t(50, A_DP, A_CP, HALF, pending=True), t(51, A_DPOST, A_CPOST, HALF),
            t(52, A_DSUM, A_CSUM, QUARTER, pending=True), t(53, A_DSUM, A_CSUM, QUARTER),
            t(54, 11, A_DEBIT_LIMIT, FUNDING)]


# -- base events -----------------------------------------------------------------------------------
ALL_T = ("plain", "pending", "post", "void", "dup", "dup_pending", "dup_post", "dup_post_partial")
CREATE = ("plain", "pending", "dup", "dup_pending")
FRESH_CREATE = ("plain", "pending")
POST_VOID = ("post", "void", "dup_post", "dup_post_partial")
ALL_A = ("account", "dup_account")


def base_event(name, st, fresh_id):
    """The valid base event `name` against the stored set `st`; `fresh_id` is used where the base is
    not a duplicate."""
    if name == "plain":
        return dict(id=fresh_id, debit_account_id=9, credit_account_id=10, amount=1, ledger=LEDGER, code=1)
    if name == "pending":
        return dict(id=fresh_id, debit_account_id=9, credit_account_id=10, amount=1, ledger=LEDGER, code=1,
                    flags=int(TF.pending))
    if name == "post":
        return dict(id=fresh_id, pending_id=st.pending_0, flags=int(TF.post_pending_transfer))
    if name == "void":
        return dict(id=fresh_id, pending_id=st.pending_0, flags=int(TF.void_pending_transfer))
    if name == "dup":
        return st.ev_posted()
    if name == "dup_pending":
        return st.ev_pending_7()
    if name == "dup_post":
        return st.ev_post_eq_1()
    if name == "dup_post_partial":
        return st.ev_post_partial()
    if name == "account":
        return dict(id=fresh_id, ledger=LEDGER, code=1)
    if name == "dup_account":
        return dict(USER_DATA_ACCOUNT)
    raise KeyError(name)


class Mutation:
    """`edits`: field -> value, ("or", bits) for flags, ("stored", attr) for an id of the stored set, or
    ("field", other) to copy another field of the event.  `bases`: the base events the edit fits, the
    first being the one it is judged on alone.  `follow`: a failing event is appended and the mutated
    event opens its chain (linked_event_failed).  `last`: the event must end its prepare
    (linked_event_chain_open); such a mutation is not paired."""

    def __init__(self, name, code, bases, edits, follow=False, last=False, late_only=False):
        self.name, self.code, self.bases, self.edits = name, code, tuple(bases), dict(edits)
        self.follow, self.last, self.late_only = follow, last, late_only
        self.op = 128 if self.bases[0] in ALL_A else 129


def _m(code, bases, variant=None, **kw):
    edits = kw.pop("edits")
    return Mutation(code.name + ("/" + variant if variant else ""), code, bases, edits, **kw)


LINKED = ("or", 1)

TRANSFER_MUTATIONS = [
    _m(CT.linked_event_failed, ALL_T, edits=dict(flags=LINKED), follow=True),
    _m(CT.linked_event_chain_open, ALL_T, edits=dict(flags=LINKED), last=True),
    _m(CT.timestamp_must_be_zero, ALL_T, edits=dict(timestamp=1)),
    _m(CT.reserved_flag, ALL_T, edits=dict(flags=("or", 1 << 6))),
    _m(CT.id_must_not_be_zero, ALL_T, edits=dict(id=0)),
    _m(CT.id_must_not_be_int_max, ALL_T, edits=dict(id=U128_MAX)),
    _m(CT.flags_are_mutually_exclusive, POST_VOID, "post_void", edits=dict(flags=("or", int(TF.post_pending_transfer | TF.void_pending_transfer)))),
    _m(CT.flags_are_mutually_exclusive, POST_VOID, "pending", edits=dict(flags=("or", int(TF.pending)))),
    _m(CT.flags_are_mutually_exclusive, POST_VOID, "balancing_debit", edits=dict(flags=("or", int(TF.balancing_debit)))),
    _m(CT.flags_are_mutually_exclusive, POST_VOID, "balancing_credit", edits=dict(flags=("or", int(TF.balancing_credit)))),
    _m(CT.debit_account_id_must_not_be_zero, CREATE, edits=dict(debit_account_id=0)),
    _m(CT.debit_account_id_must_not_be_int_max, CREATE, edits=dict(debit_account_id=U128_MAX)),
    _m(CT.credit_account_id_must_not_be_zero, CREATE, edits=dict(credit_account_id=0)),
    _m(CT.credit_account_id_must_not_be_int_max, CREATE, edits=dict(credit_account_id=U128_MAX)),
    _m(CT.accounts_must_be_different, CREATE, edits=dict(credit_account_id=("field", "debit_account_id"))),
    _m(CT.pending_id_must_be_zero, CREATE, edits=dict(pending_id=5)),
    _m(CT.pending_id_must_not_be_zero, POST_VOID, edits=dict(pending_id=0)),
    _m(CT.pending_id_must_not_be_int_max, POST_VOID, edits=dict(pending_id=U128_MAX)),
    _m(CT.pending_id_must_be_different, POST_VOID, edits=dict(pending_id=("field", "id"))),
    _m(CT.timeout_reserved_for_pending_transfer, ("plain", "dup"), "create", edits=dict(timeout=5)),
    _m(CT.timeout_reserved_for_pending_transfer, POST_VOID, "post_void", edits=dict(timeout=1)),
    _m(CT.amount_must_not_be_zero, CREATE, edits=dict(amount=0)),
    _m(CT.ledger_must_not_be_zero, CREATE, edits=dict(ledger=0)),
    _m(CT.code_must_not_be_zero, CREATE, edits=dict(code=0)),
    _m(CT.debit_account_not_found, CREATE, edits=dict(debit_account_id=A_MISSING)),
    _m(CT.credit_account_not_found, CREATE, edits=dict(credit_account_id=A_MISSING)),
    _m(CT.accounts_must_have_the_same_ledger, CREATE, edits=dict(credit_account_id=A_LEDGER_2)),
    _m(CT.transfer_must_have_the_same_ledger_as_accounts, CREATE, edits=dict(ledger=9)),
    _m(CT.pending_transfer_not_found, POST_VOID, edits=dict(pending_id=9999)),
    _m(CT.pending_transfer_not_pending, POST_VOID, edits=dict(pending_id=("stored", "posted"))),
    _m(CT.pending_transfer_has_different_debit_account_id, POST_VOID, edits=dict(debit_account_id=12)),
    _m(CT.pending_transfer_has_different_credit_account_id, POST_VOID, edits=dict(credit_account_id=12)),
    _m(CT.pending_transfer_has_different_ledger, POST_VOID, edits=dict(ledger=LEDGER_2)),
    _m(CT.pending_transfer_has_different_code, POST_VOID, edits=dict(code=9)),
    _m(CT.exceeds_pending_transfer_amount, POST_VOID, edits=dict(amount=101)),
    _m(CT.pending_transfer_has_different_amount, ("void",), edits=dict(amount=99)),
    _m(CT.pending_transfer_already_posted, ("post", "void"), edits=dict(pending_id=("stored", "pending_posted"))),
    _m(CT.pending_transfer_already_voided, ("post", "void"), edits=dict(pending_id=("stored", "pending_voided"))),
    _m(CT.pending_transfer_expired, ("post", "void"), edits=dict(pending_id=("stored", "pending_1"))),
    # create_transfer's exists ladder (:886-905) against the stored posted / pending transfer
    _m(CT.exists_with_different_flags, ("dup",), "create", edits=dict(flags=("or", int(TF.pending)))),
    _m(CT.exists_with_different_debit_account_id, ("dup", "dup_pending"), edits=dict(debit_account_id=5)),
    _m(CT.exists_with_different_credit_account_id, ("dup", "dup_pending"), edits=dict(credit_account_id=6)),
    _m(CT.exists_with_different_amount, ("dup", "dup_pending"), "create", edits=dict(amount=11)),
    _m(CT.exists_with_different_user_data_128, ("dup", "dup_pending"), "create", edits=dict(user_data_128=77)),
    _m(CT.exists_with_different_user_data_64, ("dup", "dup_pending"), "create", edits=dict(user_data_64=77)),
    _m(CT.exists_with_different_user_data_32, ("dup", "dup_pending"), "create", edits=dict(user_data_32=77)),
    _m(CT.exists_with_different_timeout, ("dup_pending",), edits=dict(timeout=8)),
    _m(CT.exists_with_different_code, ("dup", "dup_pending"), edits=dict(code=5)),
    _m(CT.exists, ("dup",), "create", edits=dict()),
    _m(CT.exists, ("dup_pending",), "create_pending", edits=dict()),
    # post_or_void_pending_transfer's exists ladder (:1016-1077): fields given, then the
    # zero-defaulting variants (a zero field is compared through the pending transfer)
    _m(CT.exists_with_different_flags, ("dup_post",), "void_of_post", edits=dict(flags=int(TF.void_pending_transfer))),
    _m(CT.exists_with_different_amount, ("dup_post",), "post", edits=dict(amount=39)),
    _m(CT.exists_with_different_amount, ("dup_post_partial",), "post_zero", edits=dict(amount=0)),
    _m(CT.exists_with_different_pending_id, ("dup_post",), edits=dict(pending_id=("stored", "pending_eq_2"))),
    _m(CT.exists_with_different_user_data_128, ("dup_post", "dup_post_partial"), "post", edits=dict(user_data_128=77)),
    _m(CT.exists_with_different_user_data_128, ("dup_post_partial",), "post_zero", edits=dict(user_data_128=0)),
    _m(CT.exists_with_different_user_data_64, ("dup_post", "dup_post_partial"), "post", edits=dict(user_data_64=77)),
    _m(CT.exists_with_different_user_data_64, ("dup_post_partial",), "post_zero", edits=dict(user_data_64=0)),
    _m(CT.exists_with_different_user_data_32, ("dup_post", "dup_post_partial"), "post", edits=dict(user_data_32=77)),
    _m(CT.exists_with_different_user_data_32, ("dup_post_partial",), "post_zero", edits=dict(user_data_32=0)),
    _m(CT.exists, ("dup_post",), "post_zero", edits=dict()),
    _m(CT.exists, ("dup_post_partial",), "post", edits=dict()),
    # the six overflow checks (:848-861): each names the one account whose balance makes it the first to fail
    _m(CT.overflows_debits_pending, ("pending",), edits=dict(debit_account_id=A_DP, amount=HALF)),
    _m(CT.overflows_credits_pending, ("pending",), edits=dict(credit_account_id=A_CP, amount=HALF)),
    _m(CT.overflows_debits_posted, FRESH_CREATE, edits=dict(debit_account_id=A_DPOST, amount=HALF)),
    _m(CT.overflows_credits_posted, FRESH_CREATE, edits=dict(credit_account_id=A_CPOST, amount=HALF)),
    _m(CT.overflows_debits, FRESH_CREATE, edits=dict(debit_account_id=A_DSUM, amount=HALF)),
    _m(CT.overflows_credits, FRESH_CREATE, edits=dict(credit_account_id=A_CSUM, amount=HALF)),
    _m(CT.overflows_timeout, ("pending",), edits=dict(timeout=TIMEOUT_MAX), late_only=True),
    _m(CT.exceeds_credits, FRESH_CREATE, edits=dict(debit_account_id=A_DEBIT_LIMIT, amount=FUNDING * 1000)),
    _m(CT.exceeds_credits, FRESH_CREATE, "balancing", edits=dict(flags=("or", int(TF.balancing_debit)))),
    _m(CT.exceeds_debits, FRESH_CREATE, edits=dict(credit_account_id=A_CREDIT_LIMIT)),
    _m(CT.exceeds_debits, FRESH_CREATE, "balancing", edits=dict(flags=("or", int(TF.balancing_credit)))),
]

ACCOUNT_MUTATIONS = [
    _m(CA.linked_event_failed, ALL_A, edits=dict(flags=LINKED), follow=True),
    _m(CA.linked_event_chain_open, ALL_A, edits=dict(flags=LINKED), last=True),
    _m(CA.timestamp_must_be_zero, ALL_A, edits=dict(timestamp=1)),
    _m(CA.reserved_field, ALL_A, edits=dict(reserved=1)),
    _m(CA.reserved_flag, ALL_A, edits=dict(flags=("or", 1 << 3))),
    _m(CA.id_must_not_be_zero, ALL_A, edits=dict(id=0)),
    _m(CA.id_must_not_be_int_max, ALL_A, edits=dict(id=U128_MAX)),
    _m(CA.flags_are_mutually_exclusive, ALL_A, edits=dict(flags=("or", int(AF.debits_must_not_exceed_credits | AF.credits_must_not_exceed_debits)))),
    _m(CA.debits_pending_must_be_zero, ALL_A, edits=dict(debits_pending=1)),
    _m(CA.debits_posted_must_be_zero, ALL_A, edits=dict(debits_posted=1)),
    _m(CA.credits_pending_must_be_zero, ALL_A, edits=dict(credits_pending=1)),
    _m(CA.credits_posted_must_be_zero, ALL_A, edits=dict(credits_posted=1)),
    _m(CA.ledger_must_not_be_zero, ALL_A, edits=dict(ledger=0)),
    _m(CA.code_must_not_be_zero, ALL_A, edits=dict(code=0)),
    _m(CA.exists_with_different_flags, ("dup_account",), edits=dict(flags=("or", int(AF.debits_must_not_exceed_credits)))),
    _m(CA.exists_with_different_user_data_128, ("dup_account",), edits=dict(user_data_128=77)),
    _m(CA.exists_with_different_user_data_64, ("dup_account",), edits=dict(user_data_64=77)),
    _m(CA.exists_with_different_user_data_32, ("dup_account",), edits=dict(user_data_32=77)),
    _m(CA.exists_with_different_ledger, ("dup_account",), edits=dict(ledger=LEDGER_2)),
    _m(CA.exists_with_different_code, ("dup_account",), edits=dict(code=3)),
    _m(CA.exists, ("dup_account",), edits=dict()),
]

NON_OK_TRANSFER_CODES = frozenset(c for c in CT if c != CT.ok)
NON_OK_ACCOUNT_CODES = frozenset(c for c in CA if c != CA.ok)
EXISTS_TRANSFER_CODES = frozenset(c for c in CT if c.name.startswith("exists"))


def _apply(ev, muts, st):
    """`ev` with the edits of `muts`; plain values first, then the ones that copy a field."""
    late = []
    for m in muts:
        for f, v in m.edits.items():
            if isinstance(v, tuple):
                if v[0] == "or":
                    ev[f] = ev.get(f, 0) | v[1]
                elif v[0] == "stored":
                    ev[f] = getattr(st, v[1])
                else:
                    late.append((f, v[1]))
            else:
                ev[f] = v
    for f, src in late:
        ev[f] = ev.get(src, 0)
    return ev


def _conflict(a, b):
    """Would one mutation's edit overwrite the other's?  Flag bits OR-ed in never do; two edits that
    set a field to the same value do not either."""
    for f, v in a.edits.items():
        if f not in b.edits:
            continue
        w = b.edits[f]
        both_or = isinstance(v, tuple) and isinstance(w, tuple) and v[0] == "or" and w[0] == "or"
        if not both_or and v != w:
            return True
    return False


def pair_base(a, b):
    """The base event a pair is applied to, or None when the pair is skipped."""
    if a.last or b.last or _conflict(a, b):
        return None
    for name in a.bases:
        if name in b.bases:
            return name
    return None


def all_pairs(muts, late):
    """(generated [(base, a, b)], skipped count) over the unordered pairs of `muts`."""
    muts = [m for m in muts if late or not m.late_only]
    made, skipped = [], 0
    for i, a in enumerate(muts):
        for b in muts[i + 1:]:
            base = pair_base(a, b)
            if base is None:
                skipped += 1
            else:
                made.append((base, a, b))
    return made, skipped


# -- scenario builder ------------------------------------------------------------------------------
class Ladder(Scenario):
    """A Scenario plus what the tests need to read its replies: `marks` — one (step index, event
    index, mutations, chained) per mutated event; `counts` — pairs_generated / pairs_skipped /
    chain_members / colliding (colliding_same_prepare: those inside one prepare); `account_ids` /
    `transfer_ids` — every id the scenario named."""

    def __init__(self, start_ts=10**12):
        super().__init__()
        self.ts = start_ts
        self.marks = []
        self.counts = dict(pairs_generated=0, pairs_skipped=0, chain_members=0, colliding=0, colliding_same_prepare=0)
        self.account_ids, self.transfer_ids = set(), set()
        self.placement = {}  # same_pass_exists: mark index -> placement name
        self._next_id = 10**6

    def fresh_id(self):
        self._next_id += 1
        return self._next_id

    def commit(self, op, events):
        """One prepare of event dicts; the timestamp advances as the reference's prepare does."""
        assert len(events) <= PREPARE_MAX
        self.ts += 1 + len(events)
        ids = self.account_ids if op == 128 else self.transfer_ids
        for ev in events:
            ids.add(ev["id"])
            if op == 129 and ev.get("pending_id"):
                ids.add(ev["pending_id"])
        pack = pack_account if op == 128 else pack_transfer
        self.steps.append(("commit", op, self.ts, [pack(**ev) for ev in events]))
        return len(self.steps) - 1

    def commit_groups(self, op, groups, prepare_max=PREPARE_MAX, closing=None):
        """Groups of (events, [(offset, mutations, chained)]) packed into prepares of at most
        `prepare_max` events, a group never split; `closing`: a group that must end the last prepare."""
        events, marks = [], []

        def flush():
            if events:
                step = self.commit(op, events)
                self.marks += [(step, k, muts, chained) for k, muts, chained in marks]
                events.clear()
                marks.clear()

        for evs, ms in list(groups) + ([closing] if closing else []):
            if len(events) + len(evs) > prepare_max:
                flush()
            marks.extend((len(events) + off, muts, chained) for off, muts, chained in ms)
            events.extend(evs)
        flush()

    def fixture(self, st):
        self.commit(128, _fixture_accounts())
        self.commit(129, [st.ev_posted()] + st.ev_pendings() + _fixture_balances())
        self.commit(129, [st.ev_post_partial(), st.ev_void_1(), st.ev_post_eq_1()])
        # A create_accounts prepare: run_many starts a new call here, so the family's events meet the
        # fixture as stored state.  (In one pass with it, a post / void naming a fixture id that a
        # duplicate event collides with sends the whole pass to tb_flow's in-kernel sequential replay.)
        self.commit(128, [dict(id=A_SPARE, ledger=LEDGER, code=1)])
        self.ts += 2 * NS  # past pending_1's expiry (timeout 1); pending_7 stays live

    def failing(self, op):
        """An event that fails on its own (closes a linked_event_failed chain)."""
        if op == 128:
            return dict(id=self.fresh_id(), ledger=0, code=1)
        return dict(id=self.fresh_id(), debit_account_id=9, credit_account_id=9, amount=1, ledger=LEDGER, code=1)

    def group(self, st, base, muts, chain=None):
        """The events of one mutated event: alone, or (`chain` = "first" / "second") in a linked chain
        with a valid transfer debiting the debit-limit account."""
        op = muts[0].op
        ev = _apply(base_event(base, st, self.fresh_id()), muts, st)
        evs, at = [ev], 0
        if chain:
            partner = dict(id=self.fresh_id(), debit_account_id=A_DEBIT_LIMIT, credit_account_id=12, amount=1,
                           ledger=LEDGER, code=1)
            # a duplicate keeps its flags (linked would turn every exists* into exists_with_different_flags)
            if chain == "first" and not base.startswith("dup") and not any(m.follow or m.last for m in muts):
                ev["flags"] = ev.get("flags", 0) | 1
                evs = [ev, partner]
            else:
                partner["flags"] = 1
                evs, at = [partner, ev], 1
        if any(m.follow for m in muts):
            evs.append(self.failing(op))
        if chain:
            self.counts["chain_members"] += len(evs)
        return evs, [(at, tuple(muts), bool(chain))]


def _singles_groups(sc, st, muts, late, chain=False):
    groups, closing = [], None
    for k, m in enumerate(muts):
        if m.late_only and not late:
            continue
        g = sc.group(st, m.bases[0], [m], chain=("first", "second")[k % 2] if chain else None)
        if m.last:
            closing = g
        else:
            groups.append(g)
    return groups, closing


def singles(late=False):
    sc = Ladder(LATE_START if late else 10**12)
    st = Stored(100)
    sc.fixture(st)
    groups, closing = _singles_groups(sc, st, ACCOUNT_MUTATIONS, late)
    sc.commit_groups(128, groups, closing=closing)
    groups, closing = _singles_groups(sc, st, TRANSFER_MUTATIONS, late)
    sc.commit_groups(129, groups, closing=closing)
    return sc


PAIRS_PREPARE = 700  # several prepares, so a commit_many call is a multi-prepare pass


def pairs():
    sc = Ladder()
    st = Stored(100)
    sc.fixture(st)
    for op, muts in ((128, ACCOUNT_MUTATIONS), (129, TRANSFER_MUTATIONS)):
        made, skipped = all_pairs(muts, late=False)
        sc.counts["pairs_generated"] += len(made)
        sc.counts["pairs_skipped"] += skipped
        sc.commit_groups(op, [sc.group(st, base, [a, b]) for base, a, b in made], prepare_max=PAIRS_PREPARE)
    return sc


LATE_PAIR_CODES = frozenset(c for c in CT if c.name.startswith("overflows")) | {CT.exceeds_credits, CT.exceeds_debits}


def _late_pairs():
    made, _ = all_pairs(TRANSFER_MUTATIONS, late=True)
    return [(base, a, b) for base, a, b in made if a.code in LATE_PAIR_CODES and b.code in LATE_PAIR_CODES]


def late_clock():
    sc = singles(late=True)
    st = Stored(100)
    made = _late_pairs()
    sc.counts["pairs_generated"] = len(made)
    sc.commit_groups(129, [sc.group(st, base, [a, b]) for base, a, b in made])
    return sc


ORDERED_PER_CODE = 3


def winners(sc, replies):
    """[(code, mark)]: the result code the replies give every marked event (0: ok)."""
    commit_steps = [k for k, step in enumerate(sc.steps) if step[0] == "commit"]
    reply_of = {step: replies[i] for i, step in enumerate(commit_steps)}
    tables, out = {}, []
    for mark in sc.marks:
        step = mark[0]
        if step not in tables:
            r = np.frombuffer(reply_of[step], dtype=RESULT_DTYPE)
            tables[step] = dict(zip(r["index"].tolist(), r["result"].tolist()))
        out.append((tables[step].get(mark[1], 0), mark))
    return out


def _representative(source):
    """Per winning transfer code, up to ORDERED_PER_CODE of the pairs of scenario `source` (as the
    oracle resolved them): [(base, a, b)]."""
    replies = run_oracle(source, OracleEngine())
    taken, out = {}, []
    for code, (step, _k, muts, _c) in winners(source, replies):
        if len(muts) != 2 or source.steps[step][1] != 129 or code == 0:
            continue
        if taken.get(code, 0) < ORDERED_PER_CODE:
            taken[code] = taken.get(code, 0) + 1
            out.append((pair_base(*muts), muts[0], muts[1]))
    return out


def _ordered(late):
    sc = Ladder(LATE_START if late else 10**12)
    st = Stored(100)
    sc.fixture(st)
    groups, closing = _singles_groups(sc, st, TRANSFER_MUTATIONS, late, chain=True)
    for k, (base, a, b) in enumerate(_representative(family("late_clock" if late else "pairs"))):
        groups.append(sc.group(st, base, [a, b], chain=("second", "first")[k % 2]))
    sc.commit_groups(129, groups, closing=closing)
    return sc


def ordered():
    return _ordered(False)


def ordered_late():
    return _ordered(True)


PLACEMENTS = ("earlier_call", "earlier_prepare", "same_prepare")
_EXISTS_MUTATIONS = [m for m in TRANSFER_MUTATIONS if m.code in EXISTS_TRANSFER_CODES]


def same_pass_exists():
    """Each exists* mutation three times, against three stored sets whose first instances (the posted
    transfer, pending_7, post_eq_1, post_partial) are committed by an earlier call, by the prepare
    before in the same call, and at the head of the same prepare.  The pending transfers the posts
    name are always stored by an earlier call.  A create_accounts prepare separates two calls
    (run_many groups consecutive prepares of one operation into one commit_many call)."""
    sc = Ladder()
    sc.fixture(Stored(100))
    sets = {p: Stored(1000 * (k + 2)) for k, p in enumerate(PLACEMENTS)}
    which = ("pending_posted", "pending_eq_1", "pending_eq_2")
    sc.commit(129, [ev for st in sets.values() for ev in st.ev_pendings(which)])

    def firsts(st):
        return [st.ev_posted(), st.ev_pending_7(), st.ev_post_eq_1(), st.ev_post_partial()]

    def seconds(st, placement, head=()):
        groups = [(list(head), [])] if head else []
        for m in _EXISTS_MUTATIONS:
            groups.append(sc.group(st, m.bases[0], [m]))
        n0 = len(sc.marks)
        sc.commit_groups(129, groups)
        for k in range(n0, len(sc.marks)):
            sc.placement[k] = placement
        return len(_EXISTS_MUTATIONS)

    def new_call():
        sc.commit(128, [dict(id=sc.fresh_id(), ledger=LEDGER, code=1)])

    new_call()
    st = sets["earlier_call"]
    sc.commit(129, firsts(st))
    new_call()
    seconds(st, "earlier_call")
    new_call()
    st = sets["earlier_prepare"]
    sc.commit(129, firsts(st))
    sc.counts["colliding"] += len(firsts(st)) + seconds(st, "earlier_prepare")
    new_call()
    st = sets["same_prepare"]
    sc.counts["colliding_same_prepare"] = len(firsts(st)) + seconds(st, "same_prepare", head=firsts(st))
    sc.counts["colliding"] += sc.counts["colliding_same_prepare"]
    return sc


FAMILIES = {
    "singles": singles,
    "pairs": pairs,
    "late_clock": late_clock,
    "ordered": ordered,
    "ordered_late": ordered_late,
    "same_pass_exists": same_pass_exists,
}

_built = {}


def family(name):
    """The scenario of one family, built once (scenarios are never modified by a run)."""
    if name not in _built:
        _built[name] = FAMILIES[name]()
    return _built[name]


def lookup_requests(sc):
    """[(operation, body)] looking up every account and transfer id the scenario named — failed
    events' ids included — plus 0 and maxInt(u128), at most 8191 ids a request."""
    out = []
    for op, ids in ((130, sc.account_ids | {A_MISSING}), (131, sc.transfer_ids)):
        ids = sorted(ids | {0, U128_MAX})
        for k in range(0, len(ids), 8191):
            out.append((op, b"".join(i.to_bytes(16, "little") for i in ids[k:k + 8191])))
    return out
