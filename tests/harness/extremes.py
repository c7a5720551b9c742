"""The checker for get_account_balance_extremes (include/tbgpu.h tbgpu_get_account_balance_extremes) —
test infrastructure only.  `Extremes` follows the header's definition over a resident export and the
current accounts, in Python ints: the measured value v(a, t) is the measure's combination of
lookup_accounts_at's balance_at(a, t) — tests/harness/asof.py's effects, anchored at the current
balance, each column modulo 2^128 — and the records of the period are walked in timestamp order, the
value recomputed from the anchor after each, the least and the greatest kept with the first timestamp
that reaches them.  Nothing here composes segments or adds steps: the engine's ordered reduction is
what this is held against.  It shares nothing with the engine, and with the other checkers only
asof.py's effect list and the field helpers."""
import bisect

import numpy as np

from tests.harness.asof import AsOf
from tests.harness.balances import MOD
from tests.harness.integrals import period_end
from tigerbeetle_amd.types import EXTREME_DTYPE, U64_MAX, pack_balance_measure

EXTREMES_MAX = 4095
MOD192 = 1 << 192


def ids_body(ids):
    return b"".join(int(i).to_bytes(16, "little") for i in ids)


class Extremes:
    """resident: the engine's exported (live, resident) transfers; accounts: its exported accounts;
    commit_timestamp: the engine's, the end of a period whose t_close is 0."""

    def __init__(self, resident, accounts, commit_timestamp):
        self.commit_timestamp = int(commit_timestamp)
        self.asof = AsOf(resident, accounts)
        # Per account, oldest first: (timestamp, the four columns' change, orphan).
        self.mine = {i: [] for i in self.asof.current}
        for ts, debit, credit, d_pending, d_posted, orphan in reversed(self.asof.effects):
            for account, moved in ((debit, (d_pending, d_posted, 0, 0)), (credit, (0, 0, d_pending, d_posted))):
                if account in self.mine:
                    self.mine[account].append((ts, moved, orphan))
        # above[a][k]: the effects of a's records k and later summed (a table of the definition's sums, so
        # that a hot account's walk stays linear).
        self.stamps = {i: [r[0] for r in records] for i, records in self.mine.items()}
        self.above = {}
        for i, records in self.mine.items():
            sums, total = [(0, 0, 0, 0)], (0, 0, 0, 0)
            for _, moved, _ in reversed(records):
                total = tuple(a + b for a, b in zip(total, moved))
                sums.append(total)
            self.above[i] = sums[::-1]

    def balance_at(self, account, t):
        """lookup_accounts_at's formula: the current balances less every effect above t, modulo 2^128."""
        sums = self.above[account][bisect.bisect_right(self.stamps[account], t)]
        return tuple((cur - s) % MOD for cur, s in zip(self.asof.current[account], sums))

    def value(self, account, t, measure):
        return sum(k * b for k, b in zip(measure, self.balance_at(account, t)))

    def one(self, account, t_open, t_end, measure):
        """(opening, closing, low, high, t_low, t_high, records) of one account over [t_open, t_end]."""
        opening = self.value(account, t_open, measure)
        low = high = opening
        t_low = t_high = t_open
        stamps = sorted({ts for ts, _, _ in self.mine[account] if t_open < ts <= t_end})
        records = sum(1 for ts, _, _ in self.mine[account] if t_open < ts <= t_end)
        for ts in stamps:
            v = self.value(account, ts, measure)
            if v < low:
                low, t_low = v, ts
            if v > high:
                high, t_high = v, ts
        return opening, self.value(account, t_end, measure), low, high, t_low, t_high, records

    def of(self, ids, t_open, t_close, measure, cap=None):
        """(rows, matched, orphan): the header's answer for the request `ids`; orphan: a post without
        its resident pending transfer entered a value (`complete` is then 0, as it is once the engine
        has evicted anything)."""
        empty = np.zeros(0, dtype=EXTREME_DTYPE)
        t_end = period_end(t_open, t_close, self.commit_timestamp)
        if len(ids) == 0 or t_end is None or t_end == 0:
            return empty, 0, False
        found = [i for i in ids if i in self.asof.current and self.asof.created[i] <= t_end]
        orphan = any(ts > t_open and orph for i in set(found) for ts, _, orph in self.mine[i])
        k = len(found) if cap is None else min(len(found), cap)
        out = np.zeros(k, dtype=EXTREME_DTYPE)
        answers = {}
        word = int.from_bytes(pack_balance_measure(measure), "little")
        for n, i in enumerate(found[:k]):
            if i not in answers:
                answers[i] = self.one(i, t_open, t_end, measure)
            opening, closing, low, high, t_low, t_high, records = answers[i]
            out["id_lo"][n], out["id_hi"][n] = i & U64_MAX, i >> 64
            for name, v in (("opening", opening), ("closing", closing), ("low", low), ("high", high)):
                for w in range(3):
                    out["%s_w%d" % (name, w)][n] = ((v % MOD192) >> (64 * w)) & U64_MAX
            out["t_low"][n], out["t_high"][n], out["records"][n] = t_low, t_high, records
            out["t_open"][n], out["t_end"][n], out["measure"][n] = t_open, t_end, word
        return out, len(found), orphan
