"""The checker for lookup_accounts_at (include/tbgpu.h tbgpu_lookup_accounts_at) — test infrastructure
only.  `AsOf` is the header's definition over a resident export and the current accounts, written
backward and anchored at the current balances, like spec_rows / spec_events:
  balance_at(a, T) = current(a) - the effects on a of every resident record above T, modulo 2^128;
a post whose pending transfer is not resident is summed with P = its own amount.  `ids_body` packs a
request."""
import numpy as np

from tests.harness.balances import COLUMNS, MOD, PENDING, POST, balances_of, effect, u128
from tigerbeetle_amd.types import ACCOUNT_DTYPE, U64_MAX

U128_MAX = (1 << 128) - 1
LOOKUP_AT_MAX = 8191


def ids_body(ids):
    return b"".join(int(i).to_bytes(16, "little") for i in ids)


class AsOf:
    """resident: the engine's exported (live, resident) transfers; accounts: its exported accounts."""

    def __init__(self, resident, accounts):
        resident = resident[np.argsort(resident["timestamp"], kind="stable")]
        amount_of = {u128(t, "id"): u128(t, "amount") for t in resident}
        self.record = {u128(a, "id"): a for a in accounts}
        self.current = {i: balances_of(a) for i, a in self.record.items()}
        self.created = {i: int(a["timestamp"]) for i, a in self.record.items()}
        # Newest first: (timestamp, debit account, credit account, d *_pending, d *_posted, orphan).
        self.effects = []
        for t in resident[::-1]:
            flags, amount = int(t["flags"]), u128(t, "amount")
            pending_amount, orphan = amount, False
            if flags & POST and not flags & PENDING:
                pending_amount = amount_of.get(u128(t, "pending_id"))
                if pending_amount is None:
                    pending_amount, orphan = amount, True
            d_pending, d_posted = effect(flags, amount, pending_amount)
            self.effects.append((int(t["timestamp"]), u128(t, "debit_account_id"), u128(t, "credit_account_id"),
                                 d_pending, d_posted, orphan))

    def at(self, ids, timestamp, out_cap_records=None):
        """(records, matched, orphan): the header's answer for the request `ids` at `timestamp` (0: now);
        orphan: a post without its resident pending transfer entered a sum (`complete` is then 0, as it
        is once the engine has evicted anything)."""
        empty = np.zeros(0, dtype=ACCOUNT_DTYPE)
        if timestamp == U64_MAX or len(ids) == 0:
            return empty, 0, False
        now = timestamp == 0
        found = [i for i in ids if i in self.record and (now or self.created[i] <= timestamp)]
        sums = {i: [0, 0, 0, 0] for i in found}
        orphan = False
        if not now:
            for ts, debit, credit, d_pending, d_posted, orph in self.effects:
                if ts <= timestamp:
                    break
                for account, col in ((debit, 0), (credit, 2)):
                    s = sums.get(account)
                    if s is not None:
                        s[col] += d_pending
                        s[col + 1] += d_posted
                        orphan |= orph
        k = len(found) if out_cap_records is None else min(len(found), out_cap_records)
        out = np.zeros(k, dtype=ACCOUNT_DTYPE)
        for n, i in enumerate(found[:k]):
            out[n] = self.record[i]
            for c, cur, s in zip(COLUMNS, self.current[i], sums[i]):
                v = (cur - s) % MOD
                out[c + "_lo"][n], out[c + "_hi"][n] = v & U64_MAX, v >> 64
        return out, len(found), orphan
