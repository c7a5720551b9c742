"""The checker for get_ledger_balances (include/tbgpu.h tbgpu_get_ledger_balances) — test
infrastructure only.  `LedgerBalances` is the header's definition over a resident export and the
current accounts, anchored at the current balances, like AsOf:
  column(L, T) = the sum of current(a).column over the accounts of ledger L
                 - the effects of every resident record of ledger L above T, modulo 2^128,
once on the debit columns and once on the credit columns; a post whose pending transfer is not
resident is summed with P = its own amount.  It is the record's own ledger field that assigns it to a
row.  Ledger 0 is every ledger together.  `ledgers_body` packs a request."""
import numpy as np

from tests.harness.balances import COLUMNS, MOD, PENDING, POST, balances_of, effect, u128
from tigerbeetle_amd.types import LEDGER_BALANCE_DTYPE, U64_MAX

LEDGERS_MAX = 1024


def ledgers_body(ledgers):
    return np.array([int(x) for x in ledgers], dtype="<u4").tobytes()


def sums_by_ledger(accounts):
    """{ledger: ([four sums modulo 2^128], accounts)} over account records, and the same under 0 for all."""
    out = {0: ([0, 0, 0, 0], 0)}
    for a in accounts:
        for key in (int(a["ledger"]), 0):
            sums, count = out.get(key, ([0, 0, 0, 0], 0))
            out[key] = ([(s + b) % MOD for s, b in zip(sums, balances_of(a))], count + 1)
    return out


class LedgerBalances:
    """resident: the engine's exported (live, resident) transfers; accounts: its exported accounts."""

    def __init__(self, resident, accounts):
        amount_of = {u128(t, "id"): u128(t, "amount") for t in resident}
        self.accounts = [(int(a["ledger"]), int(a["timestamp"]), balances_of(a)) for a in accounts]
        # (timestamp, ledger, d *_pending, d *_posted, orphan) of every resident record.
        self.effects = []
        for t in resident:
            flags, amount = int(t["flags"]), u128(t, "amount")
            pending_amount, orphan = amount, False
            if flags & POST and not flags & PENDING:
                pending_amount = amount_of.get(u128(t, "pending_id"))
                if pending_amount is None:
                    pending_amount, orphan = amount, True
            d_pending, d_posted = effect(flags, amount, pending_amount)
            self.effects.append((int(t["timestamp"]), int(t["ledger"]), d_pending, d_posted, orphan))

    def at(self, ledgers, timestamp, cap=None):
        """(rows, matched, orphan): the header's answer for the request `ledgers` at `timestamp` (0: now);
        orphan: a post without its resident pending transfer entered a sum."""
        ledgers = [int(x) for x in ledgers]
        if timestamp == U64_MAX or len(ledgers) == 0:
            return np.zeros(0, dtype=LEDGER_BALANCE_DTYPE), 0, False
        asked, now = set(ledgers), timestamp == 0
        sums = {L: [0, 0, 0, 0] for L in asked}
        counts = {L: 0 for L in asked}
        for ledger, created, balances in self.accounts:
            for L in (ledger, 0):
                if L in asked:
                    sums[L] = [s + b for s, b in zip(sums[L], balances)]
                    counts[L] += now or created <= timestamp
        orphan = False
        if not now:
            for ts, ledger, d_pending, d_posted, orph in self.effects:
                if ts <= timestamp:
                    continue
                for L in (ledger, 0):
                    if L in asked:
                        s = sums[L]
                        s[0] -= d_pending
                        s[1] -= d_posted
                        s[2] -= d_pending
                        s[3] -= d_posted
                        orphan |= orph
        k = len(ledgers) if cap is None else min(len(ledgers), cap)
        out = np.zeros(k, dtype=LEDGER_BALANCE_DTYPE)
        for i, L in enumerate(ledgers[:k]):
            for c, s in zip(COLUMNS, sums[L]):
                v = s % MOD
                out[c + "_lo"][i], out[c + "_hi"][i] = v & U64_MAX, v >> 64
            out["accounts"][i], out["ledger"][i] = counts[L], L
        return out, len(ledgers), orphan
