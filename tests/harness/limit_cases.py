"""Deterministic create_transfers passes aimed at the thresholds of tb_flow's limit-check path
(csrc/k_flow.h fl_bounds, fl_sweep, fl_walk*; csrc/pass.h tb_pass_cert) — test infrastructure only.

Pure Python / numpy: no GPU, no device generator, no random numbers.  A Case is a list of steps —
create_accounts prepares and create_transfers PASSES (each committed with one commit_many call: one
device pass) — with, per pass, what the builder claims about it:

  bound, S   the engine's overflow certificate in Python ints.  S is the sum of the amounts of the
             pass's events that the static checks let through (every event here), `bound` the sum of
             S over the create_transfers passes before it; the path a pass takes follows bound + S
             (< 2^62 walkers, < 2^63 the signed window sweep, < 2^64 the u64 sweep, else the ordered
             run; >= 2^128 no global certificate).
  expected   the result code of every event, from a model of the two limit checks alone
             (exceeds_credits before exceeds_debits), which is all these passes exercise.

The segments.  The scan rounds of fl_bounds decide a check when it decides the same way with every
undecided unit before it counted and with none counted; what they leave is walked in event order.
The builders below give a limit account a sequence of legs that the first round leaves undecided from
the second check on, with outcomes that mix:

  alternating  Y(a) X(a) X(a) Y(a) X(a) X(a) ... from slack 0: the checks go ok, fail, ok, fail, ...
               (X: a leg on the checked side — a debit of a debits_must_not_exceed_credits account, a
               credit of a credits_must_not_exceed_debits one; Y: a posted leg on the other side, from
               or to a free account: a unit with no open check.)
  blocked      funded to B + room with B = room + 1, then X(B) X(B) X(a_1) X(a_2) ...: the first X(B)
               passes in round 1, the second one fails but only once the first is known, and until
               then it keeps every later check undecided (2B exceeds the funding).  The a_i then walk
               down `room` exactly: an ok run while they fit, failures after.
  two_check    units that debit a hovering debits-limited account and credit a hovering credits-limited
               one: both checks open, every combination of verdicts, both failing included (the code
               is then exceeds_credits).
  open_y       units that debit one hovering debits-limited account and credit another: the second
               account's Y legs belong to units that are themselves undecided.
  mesh         many short segments linked by two-check units.

Pending legs: a pending X leg counts on the checked side like a posted one; a pending leg on the other
side does not count at all."""
import numpy as np

from tests.harness.configs import timestamps
from tigerbeetle_amd.types import (ACCOUNT_DTYPE, RESULT_DTYPE, TRANSFER_DTYPE, AccountFlags, CreateTransferResult as R,
                                   TransferFlags)

DLIM = int(AccountFlags.debits_must_not_exceed_credits)
CLIM = int(AccountFlags.credits_must_not_exceed_debits)
PENDING = int(TransferFlags.pending)
OK, EXCEEDS_CREDITS, EXCEEDS_DEBITS = int(R.ok), int(R.exceeds_credits), int(R.exceeds_debits)
U64, U128 = 1 << 64, 1 << 128
START_TS = 10**12
FIRST_TRANSFER_ID = 10**9
NARROW = (1 << 24) - 1  # the largest amount the walkers' 32-bit chain takes (fl_walk_run)


class Step:
    """One commit: op 128 (create_accounts) or 129 (create_transfers: one pass)."""

    def __init__(self, op, timestamps, bodies, label=None):
        self.op, self.timestamps, self.bodies, self.label = op, timestamps, bodies, label
        self.events = []      # pass: (debit account, credit account, amount, pending) per event
        self.expected = None  # pass: the result code per event
        self.bound = self.S = None

    def commit(self, engine):
        return engine.commit_many(self.op, self.timestamps, self.bodies)

    def expected_replies(self):
        """The replies as the model claims them, one per prepare."""
        out, off = [], 0
        for body in self.bodies:
            n = len(body) // 128
            codes = self.expected[off:off + n]
            bad = np.flatnonzero(codes)
            rows = np.zeros(len(bad), dtype=RESULT_DTYPE)
            rows["index"], rows["result"] = bad, codes[bad]
            out.append(rows.tobytes())
            off += n
        return out


class Case:
    def __init__(self, name, **intent):
        self.name = name
        self.intent = dict(intent)  # what the case is for: checked on the oracle (tests/test_limit_cases.py)
        self.steps = []
        self.flags = {}     # account id -> flags
        self.balance = {}   # account id -> [debits_pending, debits_posted, credits_pending, credits_posted]
        self.bound = 0      # the engine's `bound` after the steps so far
        self._fresh = []
        self._t = START_TS
        self._next_id = FIRST_TRANSFER_ID

    # -- accounts ---------------------------------------------------------------------------------
    def account(self, flags=0):
        a = len(self.flags) + 1
        self.flags[a] = flags
        self.balance[a] = [0, 0, 0, 0]
        self._fresh.append(a)
        return a

    def accounts(self, n, flags=0):
        return [self.account(flags) for _ in range(n)]

    def _commit_accounts(self):
        if not self._fresh:
            return
        rec = np.zeros(len(self._fresh), dtype=ACCOUNT_DTYPE)
        rec["id_lo"] = self._fresh
        rec["flags"] = [self.flags[a] for a in self._fresh]
        rec["ledger"], rec["code"] = 1, 1
        ts, self._t = timestamps([len(rec)], self._t + 10)
        self.steps.append(Step(128, ts, [rec.tobytes()]))
        self._fresh = []

    # -- passes -----------------------------------------------------------------------------------
    def transfers(self, events, prepare=8190, label=None):
        """One pass of `events` ((debit, credit, amount[, pending]) each), split into prepares of
        `prepare` events.  Returns its Step."""
        self._commit_accounts()
        events = [(e[0], e[1], int(e[2]), bool(e[3]) if len(e) > 3 else False) for e in events]
        n = len(events)
        assert 0 < n and all(0 < e[2] < U128 and e[0] != e[1] for e in events)
        rec = np.zeros(n, dtype=TRANSFER_DTYPE)
        rec["id_lo"] = self._next_id + np.arange(n, dtype=np.uint64)
        self._next_id += n
        rec["debit_account_id_lo"] = [e[0] for e in events]
        rec["credit_account_id_lo"] = [e[1] for e in events]
        rec["amount_lo"] = np.array([e[2] % U64 for e in events], dtype=np.uint64)
        rec["amount_hi"] = np.array([e[2] >> 64 for e in events], dtype=np.uint64)
        rec["flags"] = [PENDING if e[3] else 0 for e in events]
        rec["ledger"], rec["code"] = 1, 1
        lens = [prepare] * (n // prepare) + ([n % prepare] if n % prepare else [])
        ts, self._t = timestamps(lens, self._t + 10)
        bodies, off = [], 0
        for L in lens:
            bodies.append(rec[off:off + L].tobytes())
            off += L
        step = Step(129, ts, bodies, label)
        step.events = events
        step.expected = np.array([self._apply(*e) for e in events], dtype=np.uint32)
        step.bound, step.S = self.bound, sum(e[2] for e in events)
        self.bound = min(self.bound + step.S, U128 - 1)  # saturating, as the engine's
        self.steps.append(step)
        return step

    def _apply(self, dr, cr, amount, pending):
        """The reference's create_transfer for a plain or pending transfer between existing accounts
        of one ledger: the limit checks in their order, then the balances."""
        D, C = self.balance[dr], self.balance[cr]
        assert max(D[0] + D[1], C[2] + C[3]) + amount < U128, "the cases stay clear of the overflow checks"
        if self.flags[dr] & DLIM and D[0] + D[1] + amount > D[3]:
            return EXCEEDS_CREDITS
        if self.flags[cr] & CLIM and C[2] + C[3] + amount > C[1]:
            return EXCEEDS_DEBITS
        D[0 if pending else 1] += amount
        C[2 if pending else 3] += amount
        return OK

    def slack(self, a):
        """How much the checked side of limit account `a` may still take."""
        b = self.balance[a]
        return b[3] - b[0] - b[1] if self.flags[a] & DLIM else b[1] - b[2] - b[3]

    @property
    def passes(self):
        return [s for s in self.steps if s.op == 129]

    def run(self, engine):
        """Every step on `engine` (an OracleEngine or an Engine); the replies per step."""
        return [s.commit(engine) for s in self.steps]


# ---- segments: lists of events ------------------------------------------------------------------------
class Seg:
    """The legs of one limit account: x(a) a leg on its checked side, y(a) a posted (or pending) leg
    on the other side, against the free accounts `src` (pays in) and `sink` (is paid)."""

    def __init__(self, case, account, src, sink):
        self.account, self.src, self.sink = account, src, sink
        self.mirror = bool(case.flags[account] & CLIM)
        assert case.flags[account] & (DLIM | CLIM) and not case.flags[src] and not case.flags[sink]

    def x(self, amount, pending=False):
        return (self.src, self.account, amount, pending) if self.mirror else (self.account, self.sink, amount, pending)

    def y(self, amount, pending=False):
        return (self.account, self.sink, amount, pending) if self.mirror else (self.src, self.account, amount, pending)


def alternating(seg, checks, amount=1, pend_x=False, pend_y=False):
    """Y X X Y X X ... with `checks` X legs, from slack 0: ok, fail, ok, fail, ...  pend_y adds a
    pending leg on the unchecked side after every posted one (it must not count)."""
    out = []
    for k in range(checks):
        if k % 2 == 0:
            out.append(seg.y(amount))
            if pend_y:
                out.append(seg.y(amount, True))
        out.append(seg.x(amount, pend_x))
    return out


def alternating_codes(seg, checks, pend_y=False):
    """alternating()'s result codes in closed form."""
    fail = EXCEEDS_DEBITS if seg.mirror else EXCEEDS_CREDITS
    out = []
    for k in range(checks):
        if k % 2 == 0:
            out += [OK, OK] if pend_y else [OK]
        out.append(OK if k % 2 == 0 else fail)
    return out


def blocked(seg, amounts, room, fund=True, pend_x=False):
    """Funding of B + room (B = room + 1; fund=False: the account already has that slack), X(B) X(B),
    then X(a) for a in amounts: undecided from the second X(B) on, and the a_i walk `room` down."""
    B = room + 1
    assert all(0 < a <= B + room for a in amounts)
    return ([seg.y(B + room)] if fund else []) + [seg.x(B, pend_x), seg.x(B, pend_x)] + [seg.x(a, pend_x) for a in amounts]


def blocked_codes(seg, amounts, room, fund=True):
    fail = EXCEEDS_DEBITS if seg.mirror else EXCEEDS_CREDITS
    out = ([OK] if fund else []) + [OK, fail]
    for a in amounts:
        out.append(OK if a <= room else fail)
        room -= a if a <= room else 0
    return out


def two_check(dseg, cseg, units):
    """`units` transfers of 1 from dseg's account (debits-limited) to cseg's (credits-limited), both
    hovering: per six units ok, both checks fail, the credit side alone fails, ok, the debit side
    alone fails, ok."""
    assert not dseg.mirror and cseg.mirror
    T = (dseg.account, cseg.account, 1, False)
    cycle = [dseg.y(1), cseg.y(1), T, T, dseg.y(1), T, cseg.y(1), T, cseg.y(1), T, dseg.y(1), T]
    out, n = [], 0
    while n < units:
        for e in cycle:
            if e is T:
                if n == units:
                    break
                n += 1
            out.append(e)
    return out


def two_check_codes(units):
    """The codes of two_check()'s units (its other events are ok)."""
    cycle = [OK, EXCEEDS_CREDITS, EXCEEDS_DEBITS, OK, EXCEEDS_CREDITS, OK]
    return [cycle[k % 6] for k in range(units)]


def open_y(seg1, seg2, cycles, a=1):
    """Per cycle: Y(a) for seg2's account, two transfers of a from seg2's account to seg1's (ok, fail),
    two X(a) of seg1's account (ok, fail).  seg1's Y legs are X legs of seg2: undecided units."""
    assert not seg1.mirror and not seg2.mirror
    U = (seg2.account, seg1.account, a, False)
    return [e for _ in range(cycles) for e in (seg2.y(a), U, U, seg1.x(a), seg1.x(a))]


def mesh(case, dl, cl, src, sink, fan=4):
    """Every debits-limited account of `dl` pays 1 to `fan` credits-limited accounts of `cl`, round by
    round (len(dl) == len(cl)); each account is topped up by 1, 2 or 3 first, so its segment has `fan`
    checks and runs out of slack at a different round than its partners'."""
    n = len(dl)
    assert n == len(cl)
    out = []
    assert n % 5 and len(set((r * 13 + r * r // 2) % n for r in range(fan))) == fan  # a new partner every round
    for i, a in enumerate(dl):
        out.append(Seg(case, a, src, sink).y(1 + i % 3))
    for j, b in enumerate(cl):
        out.append(Seg(case, b, src, sink).y(3 - j % 3))
    for r in range(fan):
        for i, a in enumerate(dl):
            out.append((a, cl[(i * 5 + r * 13 + r * r // 2) % n], 1, False))
    return out


def interleave(*lists):
    """Round-robin merge: each list keeps its order."""
    out, its = [], [iter(x) for x in lists]
    while its:
        for it in list(its):
            try:
                out.append(next(it))
            except StopIteration:
                its.remove(it)
    return out


# ---- tier placement -------------------------------------------------------------------------------------
def place(case, target, S, park=None, inside=None):
    """One or two earlier passes after which the next pass, of sum S, has bound + S == target.
    park=(f1, f2): a single transfer between two free accounts.  inside=(seg, f1, f2): the limit
    account of `seg` is paid A and pays A back (its slack is 0 again and both its sides are about
    target / 2), plus a filler between f1 and f2 for the exact value."""
    need = target - S - case.bound
    if inside is None:
        assert need > 0
        case.transfers([(park[0], park[1], need)], label="park")
        return
    seg, f1, f2 = inside
    A = need // 2 - 1
    assert A > 0 and case.slack(seg.account) == 0
    case.transfers([seg.y(A), (f1, f2, need - 2 * A)], label="fund")
    case.transfers([seg.x(A)], label="draw")


def codes_of(step, replies):
    """The result code per event of a pass from its replies."""
    out, off = np.zeros(len(step.events), dtype=np.uint32), 0
    for body, reply in zip(step.bodies, replies):
        rows = np.frombuffer(reply, dtype=RESULT_DTYPE)
        out[off + rows["index"].astype(np.int64)] = rows["result"]
        off += len(body) // 128
    return out


# ---- the cases ---------------------------------------------------------------------------------------------
TIERS = {"2^62": 1 << 62, "2^63": 1 << 63, "2^64": 1 << 64}
WHERE = ("parked", "inside", "wide")


def hover_pass(case, heavy, light, src, sink, amount=1):
    """The pass the tier cases share: a heavy alternating segment on a debits-limited account (300
    checks), a light one on a credits-limited account (100), interleaved."""
    return interleave(alternating(heavy, 300, amount), alternating(light, 100, amount))


def tier_case(tier, at, where):
    """bound + S == TIERS[tier] - 1 (at = -1) or == TIERS[tier] (at = 0) on the hovering pass; the
    big amount parked on free accounts (where = "parked"), inside the heavy limit account ("inside"),
    or mostly in the pass itself ("wide": every leg moves target / 1024, so the sums of the checks
    climb to about a quarter of the target within the pass)."""
    target = TIERS[tier] + at
    case = Case("tier %s%+d %s" % (tier, at, where), target=target, codes={EXCEEDS_CREDITS, EXCEEDS_DEBITS})
    src, sink, f1, f2 = case.accounts(4)
    heavy, light = Seg(case, case.account(DLIM), src, sink), Seg(case, case.account(CLIM), src, sink)
    events = hover_pass(case, heavy, light, src, sink, amount=target // 1024 if where == "wide" else 1)
    S = sum(e[2] for e in events)
    if where == "inside":
        place(case, target, S, inside=(heavy, f1, f2))
    else:
        place(case, target, S, park=(f1, f2))
    case.transfers(events, prepare=250, label="test")
    return case


def global_case(at):
    """bound + S == 2^128 - 1 or 2^128: the pass keeps or loses the global overflow certificate, with
    limit accounts hovering in it.  (No balance comes near 2^128: the parked amount sits on two free
    accounts the pass does not touch.)"""
    target = U128 + at
    case = Case("global 2^128%+d" % at, target=target, codes={EXCEEDS_CREDITS, EXCEEDS_DEBITS})
    src, sink, f1, f2 = case.accounts(4)
    heavy, light = Seg(case, case.account(DLIM), src, sink), Seg(case, case.account(CLIM), src, sink)
    events = hover_pass(case, heavy, light, src, sink)
    place(case, target, sum(e[2] for e in events), park=(f1, f2))
    case.transfers(events, prepare=250, label="test")
    return case


def carry_case(hover=False):
    """The pass that loses the 64-bit certificate carries balance words: the free account `src` has
    debits_posted 2^64 - 1 and the debits-limited account `full` credits_posted 2^64 - 1 when it
    starts (bound = 2^64 - 1: it is the first pass without the certificate), and its first event moves
    1 from src to full.  A second limit account hovers with small balances, paid from src too.
    hover: instead, `full` is drawn down to slack 0 first, so it hovers itself with both its sides at
    2^64 - 1 and its credits_posted carries under the checks (bound is then about 2^65 already)."""
    case = Case("carry 2^64" + (" hovering" if hover else ""), codes={EXCEEDS_CREDITS})
    src, sink = case.accounts(2)
    full, small = Seg(case, case.account(DLIM), src, sink), Seg(case, case.account(DLIM), src, sink)
    case.transfers([full.y(U64 - 1)], label="fill")  # src.debits_posted = full.credits_posted = 2^64 - 1
    if hover:
        case.transfers([full.x(U64 - 1)], label="draw")
        events = interleave(alternating(full, 120), alternating(small, 300))
    else:
        case.intent["cert64"] = False
        events = [full.y(1), full.x(5)] + interleave(alternating(small, 300), [full.x(3)] * 50, [full.y(2)] * 20)
    step = case.transfers(events, prepare=200, label="test")
    case.intent["target"] = step.bound + step.S
    return case


def _filled(seg, amounts, room, length, **kw):
    """blocked() with X(1) legs padded in front of `amounts` (and the room they use), so that the
    segment has `length` undecided positions — the blocker, the pad, the amounts — and the amounts
    begin at position length - len(amounts).  Returns the events and their codes."""
    pad = length - 1 - len(amounts)
    assert pad >= 0
    return blocked(seg, [1] * pad + list(amounts), room + pad, **kw), blocked_codes(seg, [1] * pad + list(amounts), room + pad)


def walk_case(name, amounts, room, heavy, mirror=False, pend_x=False):
    """One limit account whose undecided segment is: the blocker (position 0), 63 X(1) legs (the rest
    of the first 64-position window), then `amounts` from position 64 on — window-aligned — walking
    `room` down; heavy: 192 more X(1) legs behind the blocker first, so the segment has at least
    WALK_HEAVY = 256 positions and `amounts` begin at position 256.  The walk's result codes are
    known in closed form (blocked_codes)."""
    case = Case(name, heavy=heavy, amounts=list(amounts))
    src, sink = case.accounts(2)
    seg = Seg(case, case.account(CLIM if mirror else DLIM), src, sink)
    start = 256 if heavy else 64
    events, codes = _filled(seg, amounts, room, start + len(amounts), pend_x=pend_x)
    case.intent["codes"] = {EXCEEDS_DEBITS if mirror else EXCEEDS_CREDITS}
    case.intent["closed_form"] = codes
    case.intent["start"] = start
    case.transfers(events, label="test")
    return case


def walk_cases(heavy):
    """The 32-bit / 64-bit walk (fl_walk_run: 32 bits iff every |delta| of the run is below 2^24, the
    running value clamped to +-2^30), each case's amounts starting on a window boundary."""
    N, W = NARROW, 1 << 24
    tag = "heavy" if heavy else "light"
    out = []
    # Whole windows of the largest narrow amount: 128 fit the room, 16 more fail.
    out.append(walk_case("narrow windows " + tag, [N] * 144, 128 * N, heavy))
    out.append(walk_case("narrow windows mirror " + tag, [N] * 144, 128 * N, heavy, mirror=True))
    # One amount of 2^24 among them: the run takes the 64-bit walk.
    for lane in (0, 31, 63):
        amounts = [N] * 64
        amounts[lane] = W
        out.append(walk_case("one wide amount at lane %d %s" % (lane, tag), amounts + [N] * 8, 66 * N, heavy))
    # Whole windows of wide amounts of 2^24, 2^25 and 2^26 - 1: 64 ok lanes move the sum by 2^30 and more.
    for a in (W, 1 << 25, (1 << 26) - 1):
        out.append(walk_case("wide windows of %d %s" % (a, tag), [a] * 72, 68 * a + 5, heavy))
    # The slack at the last narrow check equal to its amount, one less, one more (then 1s: one passes at most).
    for delta in (-1, 0, 1):
        out.append(walk_case("slack = amount%+d %s" % (delta, tag), [N] * 63 + [N, 1, 1], 64 * N + delta, heavy))
        out.append(walk_case("slack = amount%+d of 1 %s" % (delta, tag), [1] * 63 + [3, 1, 1], 63 + 3 + delta, heavy))
    # Slack minus amount at 2^30 - 1, 2^30, 2^30 + 1 on lane 0, then 63 maximal narrow debits (they
    # all fit: 63 (2^24 - 1) < 2^30), and in the next window two more of which one fits.
    for delta in (-1, 0, 1):
        room = N + (1 << 30) + delta
        out.append(walk_case("clamp 2^30%+d %s" % (delta, tag), [N] * 66, room, heavy))
    # ... and the value far above the clamp with narrow amounts.
    out.append(walk_case("clamp 2^40 %s" % tag, [N] * 64 + [1 << 40, N], (1 << 40) + 64 * N, heavy))
    return out


LENGTHS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 319, 320, 321, 511, 512, 513, 577)


def lengths_case(lengths=LENGTHS):
    """One pass per length L on fresh accounts: one debits-limited account with L undecided positions
    — alternating for odd L (L + 1 checks, the first decided in round 1), blocked for even L."""
    case = Case("segment lengths", lengths=list(lengths), codes={EXCEEDS_CREDITS})
    for L in lengths:
        src, sink = case.accounts(2)
        seg = Seg(case, case.account(DLIM), src, sink)
        if L % 2:
            events = alternating(seg, L + 1)
        else:
            events = blocked(seg, [1] * (L - 1), L // 2)
        case.transfers(events, label="L=%d" % L)
    return case


def dispatch_case(nh, linked):
    """`nh` heavy segments (300 undecided positions each) and two light ones in a pass of at most
    2048 events (tb_flow then launches 4 workgroups).  linked: the heavy accounts come in pairs of a
    debits-limited and a credits-limited one joined by two-check units (units with legs on two heavy
    segments); else each hovers on its own."""
    case = Case("dispatch nh=%d%s" % (nh, " linked" if linked else ""), nh=nh,
                codes={EXCEEDS_CREDITS, EXCEEDS_DEBITS})
    src, sink = case.accounts(2)
    parts = []
    if linked:
        d = [Seg(case, case.account(DLIM), src, sink) for _ in range((nh + 1) // 2)]
        c = [Seg(case, case.account(CLIM), src, sink) for _ in range(nh // 2)]
        for k in range(len(c)):
            parts.append(two_check(d[k], c[k], 330))
        if nh % 2:  # the odd one: linked to a light credits-limited account
            parts.append(two_check(d[-1], Seg(case, case.account(CLIM), src, sink), 40) + alternating(d[-1], 300))
    else:
        for k in range(nh):
            seg = Seg(case, case.account(CLIM if k % 2 else DLIM), src, sink)
            parts.append(alternating(seg, 301))
    parts.append(alternating(Seg(case, case.account(DLIM), src, sink), 40))
    parts.append(alternating(Seg(case, case.account(CLIM), src, sink), 30))
    events = interleave(*parts)
    assert len(events) <= 2048
    case.transfers(events, prepare=500, label="test")
    return case


def mesh_case(n=48):
    """2n = 96 light segments of 4 checks each, linked by two-check units, in a pass of under 2048
    events: more segments than the 64 light waves of 4 workgroups."""
    case = Case("mesh", codes={EXCEEDS_CREDITS, EXCEEDS_DEBITS})
    src, sink = case.accounts(2)
    dl, cl = case.accounts(n, DLIM), case.accounts(n, CLIM)
    events = mesh(case, dl, cl, src, sink)
    assert len(events) <= 2048
    case.transfers(events, label="test")
    return case


def equal_segments_case(positions):
    """Limit accounts with exactly `positions` legs each (alternating, Y legs included: the scan's
    positions are all the legs), 3072 positions in all: three 1024-position tiles, and every wave,
    chunk and tile boundary of the scan is a segment start."""
    case = Case("equal segments of %d" % positions, codes={EXCEEDS_CREDITS, EXCEEDS_DEBITS})
    src, sink = case.accounts(2)
    parts = []
    for k in range(3072 // positions):
        seg = Seg(case, case.account(CLIM if k % 2 else DLIM), src, sink)
        legs = alternating(seg, positions)[:positions]
        parts.append(legs)
    events = interleave(*parts)
    assert len(events) == 3072
    case.transfers(events, prepare=1000, label="test")
    return case


def long_segment_case():
    """One segment of 2499 positions (1666 checks) and six short ones, about 3000 events: the long
    one covers a whole 1024-position tile, which then holds no segment start."""
    case = Case("long segment", codes={EXCEEDS_CREDITS, EXCEEDS_DEBITS})
    src, sink = case.accounts(2)
    shorts = [Seg(case, case.account(CLIM if k % 2 else DLIM), src, sink) for k in range(3)]
    long = Seg(case, case.account(DLIM), src, sink)
    shorts += [Seg(case, case.account(CLIM if k % 2 else DLIM), src, sink) for k in range(3)]
    events = interleave(alternating(long, 1666), *[alternating(s, 50 + 7 * k) for k, s in enumerate(shorts)])
    case.transfers(events, prepare=1000, label="test")
    return case


def table_case(n=1536, tier=None):
    """n hovering limit accounts of 3 positions each in one pass (Y X X: the second check undecided):
    more segment heads than the window sweep's LDS table holds (SW_CAP = 1024).  tier: bound + S
    placed at 2^62 + 2^61 first, where the default build takes the window sweep."""
    case = Case("sweep table" + (" in [2^62, 2^63)" if tier else ""), codes={EXCEEDS_CREDITS, EXCEEDS_DEBITS})
    src, sink, f1, f2 = case.accounts(4)
    segs = [Seg(case, a, src, sink) for a in case.accounts(n // 2, DLIM) + case.accounts(n // 2, CLIM)]
    events = interleave(*[alternating(s, 2, amount=1 + k % 3) for k, s in enumerate(segs)])
    if tier:
        case.intent["target"] = (1 << 62) + (1 << 61)
        place(case, case.intent["target"], sum(e[2] for e in events), park=(f1, f2))
    case.transfers(events, prepare=1500, label="test")
    return case


ABANDON_CHECKS = 4300  # > FLOW_BOUNDS_ROUNDS_MAX = 4096: a round decides one check of an alternating segment


def abandon_case():
    """An alternating segment of 4300 checks, then a normal hovering pass on the same accounts."""
    case = Case("abandon", codes={EXCEEDS_CREDITS, EXCEEDS_DEBITS})
    src, sink = case.accounts(2)
    heavy, light = Seg(case, case.account(DLIM), src, sink), Seg(case, case.account(CLIM), src, sink)
    case.transfers(alternating(heavy, ABANDON_CHECKS), prepare=2000, label="long")
    case.transfers(hover_pass(case, heavy, light, src, sink), prepare=250, label="after")
    return case


def kinds_case(kind, heavy, amount=1, target=None):
    """The event kinds in a segment: pending legs on either side, two-check units, Y legs of open units
    (these with legs of `amount`: a heavy walker that takes an open Y leg as a pending credit walks on
    in 32 bits while the amounts stay below 2^22 and the pending credits below 2^28).  target: bound + S
    of the pass, placed by an amount parked on free accounts (else the pass is the first: walkers)."""
    n = 300 if heavy else 60
    case = Case("%s %s%s%s" % (kind, "heavy" if heavy else "light", " of %d" % amount if amount != 1 else "",
                               " at %d" % target if target else ""), heavy=heavy)
    src, sink = case.accounts(2)
    d1, d2 = Seg(case, case.account(DLIM), src, sink), Seg(case, case.account(DLIM), src, sink)
    c1, c2 = Seg(case, case.account(CLIM), src, sink), Seg(case, case.account(CLIM), src, sink)
    both = {EXCEEDS_CREDITS, EXCEEDS_DEBITS}
    if kind == "pending_x":
        events = interleave(alternating(d1, n, pend_x=True), alternating(c1, n, pend_x=True))
        case.intent["codes"] = both
    elif kind == "pending_y":
        events = interleave(alternating(d1, n, pend_y=True), alternating(c1, n, pend_y=True))
        case.intent["codes"] = both
        case.intent["closed_form_by_account"] = {d1.account: alternating_codes(d1, n, True),
                                                 c1.account: alternating_codes(c1, n, True)}
    elif kind == "two_check":
        events = interleave(two_check(d1, c1, n), alternating(d2, 20), alternating(c2, 20))
        case.intent["codes"] = both
        case.intent["units"] = ((d1.account, c1.account), two_check_codes(n))
    else:
        assert kind == "open_y"
        # (the credits-limited account stays light: two heavy segments get a wave each of 4 workgroups)
        events = interleave(open_y(d1, d2, n // 2 + 1, amount), alternating(c1, 60))
        case.intent["codes"] = both
    if target:
        case.intent["target"] = target
        place(case, target, sum(e[2] for e in events), park=case.accounts(2))
    case.transfers(events, prepare=400, label="test")
    return case


SWEEP_TARGETS = {"signed": (1 << 62) + (1 << 61), "u64": (1 << 63) + (1 << 62)}  # inside the window sweep's two tiers
KINDS = ("pending_x", "pending_y", "two_check", "open_y")
OPEN_Y_AMOUNTS = ((1 << 22) - 1, 1 << 22, NARROW, 1 << 24, (1 << 28) - 1, 1 << 28, 1 << 40)


def all_cases():
    """Every case, for the oracle's check of the builder's claims."""
    out = [tier_case(t, at, w) for t in TIERS for at in (-1, 0) for w in WHERE]
    out += [global_case(-1), global_case(0), carry_case(), carry_case(hover=True)]
    out += walk_cases(False) + walk_cases(True)
    out += [lengths_case()]
    out += [dispatch_case(nh, linked) for nh in (1, 2, 3) for linked in (False, True)]
    out += [mesh_case(), equal_segments_case(64), equal_segments_case(128), long_segment_case()]
    out += [table_case(), table_case(tier=True), abandon_case()]
    out += [kinds_case(k, h) for k in KINDS for h in (False, True)]
    out += [kinds_case("open_y", True, a) for a in OPEN_Y_AMOUNTS]
    out += [kinds_case(k, False, target=t) for k in KINDS for t in SWEEP_TARGETS.values()]
    return out
