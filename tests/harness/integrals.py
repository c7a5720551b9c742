"""The checker for get_account_balance_integrals (include/tbgpu.h tbgpu_get_account_balance_integrals) —
test infrastructure only.  `Integrals` is the header's first-principles definition over a resident
export and the current accounts, in Python ints:
  integral[c] = the sum over t = t_open .. t_end - 1 of balance_at(a, t).c, modulo 2^192,
  balance_at(a, t) = current(a) - the effects on a of every resident record above t, modulo 2^128,
with t_end = t_close, or commit_timestamp where t_close is 0.  balance_at is constant between two
records of the account, so the sum is taken a stretch at a time: the balance of the stretch (each one
computed from the anchor, as the definition says) times its length.  Nothing here multiplies an effect
by a weight: the engine's order-free form is what this is held against.  opening and closing are
balance_at(t_open) and balance_at(t_end).  A post whose pending transfer is not resident is summed with
P = its own amount.  It shares nothing with the engine, and with the other checkers only the field
helpers."""
import bisect

import numpy as np

from tests.harness.balances import COLUMNS, MOD, PENDING, POST, VOID, balances_of, u128
from tigerbeetle_amd.types import INTEGRAL_DTYPE, U64_MAX

INTEGRALS_MAX = 4095
MOD192 = 1 << 192


def period_end(t_open, t_close, commit_timestamp):
    """t_end of a valid period, None of an invalid one."""
    if t_open == U64_MAX or t_close == U64_MAX:
        return None
    t_end = t_close if t_close else commit_timestamp
    return t_end if t_end >= t_open else None


def balances(row, when):
    return tuple(u128(row, when + "_" + c) for c in COLUMNS)


def integrals(row):
    """The four integrals of a row as Python ints."""
    return tuple(sum(int(row["integral_%s_w%d" % (c, k)]) << (64 * k) for k in range(3)) for c in COLUMNS)


class Integrals:
    """resident: the engine's exported (live, resident) transfers; accounts: its exported accounts;
    commit_timestamp: the engine's, the end of a period whose t_close is 0."""

    def __init__(self, resident, accounts, commit_timestamp):
        self.commit_timestamp = int(commit_timestamp)
        amount_of = {u128(t, "id"): u128(t, "amount") for t in resident}
        self.current = {u128(a, "id"): balances_of(a) for a in accounts}
        self.created = {u128(a, "id"): int(a["timestamp"]) for a in accounts}
        # Per account, oldest first: (timestamp, (d debits_pending, d debits_posted, d credits_pending, d credits_posted), orphan).
        mine = {i: [] for i in self.current}
        for t in resident[np.argsort(resident["timestamp"], kind="stable")]:
            kind, amount = int(t["flags"]), u128(t, "amount")
            orphan = False
            if kind & PENDING:
                moved = (amount, 0)
            elif kind & POST:
                held = amount_of.get(u128(t, "pending_id"))
                if held is None:
                    held, orphan = amount, True
                moved = (-held, amount)
            elif kind & VOID:
                moved = (-amount, 0)  # a void stores its pending transfer's amount
            else:
                moved = (0, amount)
            for side, name in enumerate(("debit_account_id", "credit_account_id")):
                records = mine.get(u128(t, name))
                if records is not None:
                    records.append((int(t["timestamp"]), (moved + (0, 0)) if side == 0 else ((0, 0) + moved), orphan))
        self.stamps = {i: [r[0] for r in records] for i, records in mine.items()}
        # above[i][k]: the effects of records[k:] summed, so balance_at(t) = current - above[first record above t].
        self.above, self.orphans = {}, {}
        for i, records in mine.items():
            sums, total = [(0, 0, 0, 0)], (0, 0, 0, 0)
            for _, moved, _ in reversed(records):
                total = tuple(a + b for a, b in zip(total, moved))
                sums.append(total)
            self.above[i] = sums[::-1]
            self.orphans[i] = [ts for ts, _, orphan in records if orphan]

    def balance_at(self, account, t):
        k = bisect.bisect_right(self.stamps[account], t)
        return tuple((cur - s) % MOD for cur, s in zip(self.current[account], self.above[account][k]))

    def one(self, account, t_open, t_end):
        """(opening, closing, the four integrals) of one account over (t_open, t_end]."""
        stamps = self.stamps[account]
        # The stretches of constant balance: [t_open, r1), [r1, r2), ..., [rk, t_end), r the record timestamps inside.
        cuts = [t_open] + sorted(set(stamps[bisect.bisect_right(stamps, t_open):bisect.bisect_left(stamps, t_end)])) + [t_end]
        total = [0, 0, 0, 0]
        for start, stop in zip(cuts, cuts[1:]):
            for c, v in enumerate(self.balance_at(account, start)):
                total[c] += v * (stop - start)
        return self.balance_at(account, t_open), self.balance_at(account, t_end), tuple(v % MOD192 for v in total)

    def order_free(self, account, t_open, t_end):
        """The header's order-free form, opening * L + the sum of effect(r) * (t_end - t_r) over the
        records in (t_open, t_end], modulo 2^192: equal to one()'s integrals wherever no balance_at in
        the period falls below zero, and what the header specifies where one does (the engine after a
        setup action or a device panic that left a balance below what the later records move)."""
        stamps, above = self.stamps[account], self.above[account]
        total = [v * (t_end - t_open) for v in self.balance_at(account, t_open)]
        for k in range(bisect.bisect_right(stamps, t_open), bisect.bisect_right(stamps, t_end)):
            for c in range(4):
                total[c] += (above[k][c] - above[k + 1][c]) * (t_end - stamps[k])
        return tuple(v % MOD192 for v in total)

    def of(self, ids, t_open, t_close, cap=None):
        """(rows, matched, orphan): the header's answer for the request `ids`; orphan: a post without
        its resident pending transfer entered a sum (`complete` is then 0, as it is once the engine
        has evicted anything)."""
        empty = np.zeros(0, dtype=INTEGRAL_DTYPE)
        t_end = period_end(t_open, t_close, self.commit_timestamp)
        if len(ids) == 0 or t_end is None:
            return empty, 0, False
        found = [i for i in ids if i in self.current and self.created[i] <= t_end]
        orphan = any(ts > t_open for i in set(found) for ts in self.orphans[i])
        k = len(found) if cap is None else min(len(found), cap)
        out = np.zeros(k, dtype=INTEGRAL_DTYPE)
        answers = {}
        for n, i in enumerate(found[:k]):
            if i not in answers:
                answers[i] = self.one(i, t_open, t_end)
            opening, closing, sums = answers[i]
            out["id_lo"][n], out["id_hi"][n] = i & U64_MAX, i >> 64
            for c, name in enumerate(COLUMNS):
                for when, v in (("opening", opening[c]), ("closing", closing[c])):
                    out["%s_%s_lo" % (when, name)][n], out["%s_%s_hi" % (when, name)][n] = v & U64_MAX, v >> 64
                for w in range(3):
                    out["integral_%s_w%d" % (name, w)][n] = (sums[c] >> (64 * w)) & U64_MAX
            out["t_open"][n], out["t_end"][n] = t_open, t_end
        return out, len(found), orphan


def ids_body(ids):
    return b"".join(int(i).to_bytes(16, "little") for i in ids)
