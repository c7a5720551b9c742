"""The checker for get_account_counterparties (include/tbgpu.h tbgpu_get_account_counterparties) — test
infrastructure only.  `Counterparties` is the header's definition over a resident export, written
straight from its text:
  a record with t_open < ts (<= t_close unless that is 0) matches when its debit account is the subject
  and DEBITS is wanted — it feeds `to` of the row of its credit account — or when its credit account is
  the subject and CREDITS is wanted — it feeds `from` of the row of its debit account; a record from the
  subject to itself does both; by kind it adds what a flow-matrix cell adds, and one transfer;
  a group is a counterparty id at or above id_min with a matching record; rows come by id ascending, or
  by (to.posted + from.posted) mod 2^128 descending and then by id; the first
  min(limit, cap, 8191, groups) are written.
A post whose pending transfer is not resident is summed with P = its own amount and is an orphan
wherever it matched, whatever id_min and the limit.  No account table is read.  It shares nothing with
the engine and nothing with tests/harness/matrix.py but the field helpers."""
import numpy as np

from tests.harness.balances import MOD, PENDING, POST, VOID, u128
from tigerbeetle_amd.types import COUNTERPARTY_DTYPE, U64_MAX

ROWS_MAX = 8191
DEBITS, CREDITS, REVERSED, BY_VOLUME = 1, 2, 4, 1 << 8
SUMS = ("posted", "pending_in", "pending_out")
ID_MAX = MOD - 1


def valid_filter(account, t_open, t_close, limit, flags, reserved=bytes(8)):
    if account in (0, ID_MAX) or not flags & (DEBITS | CREDITS) or flags & ~(DEBITS | CREDITS | BY_VOLUME):
        return False
    if any(reserved) or t_open == U64_MAX or t_close == U64_MAX or (t_close != 0 and t_close < t_open):
        return False
    return limit != 0


def flow_sums(row, direction):
    """(posted, pending_in, pending_out, transfers) of a row's `to` or `from` half."""
    return tuple(u128(row, direction + "_" + s) for s in SUMS) + (int(row[direction + "_transfers"]),)


def id_of(row):
    return u128(row, "id")


def volume_of(row):
    return (u128(row, "to_posted") + u128(row, "from_posted")) % MOD


class Counterparties:
    """resident: the engine's exported (live, resident) transfers."""

    def __init__(self, resident):
        amount_of = {u128(t, "id"): u128(t, "amount") for t in resident}
        # Per record: (timestamp, debit account, credit account, (posted, pending_in, pending_out), orphan).
        self.records = []
        for t in resident:
            kind, amount = int(t["flags"]), u128(t, "amount")
            orphan = False
            if kind & PENDING:
                add = (0, amount, 0)
            elif kind & POST:
                p = amount_of.get(u128(t, "pending_id"))
                if p is None:
                    p, orphan = amount, True
                add = (amount, 0, p)
            elif kind & VOID:
                add = (0, 0, amount)  # a void stores its pending transfer's amount
            else:
                add = (amount, 0, 0)
            self.records.append((int(t["timestamp"]), u128(t, "debit_account_id"), u128(t, "credit_account_id"), add, orphan))

    def of(self, account, t_open=0, t_close=0, flags=DEBITS | CREDITS, id_min=0, limit=ROWS_MAX, cap=None, reserved=bytes(8)):
        """(rows, matched, orphan): the header's answer; orphan: a post without its resident pending
        transfer matched (`complete` is then 0, as it is once the engine has evicted anything)."""
        if not valid_filter(account, t_open, t_close, limit, flags, reserved):
            return np.zeros(0, dtype=COUNTERPARTY_DTYPE), 0, False
        groups, orphan = {}, False
        for ts, d, c, add, orph in self.records:
            if ts <= t_open or (t_close != 0 and ts > t_close):
                continue
            feeds = []
            if flags & DEBITS and d == account:
                feeds.append((c, 0))
            if flags & CREDITS and c == account:
                feeds.append((d, 1))
            for x, direction in feeds:
                orphan |= orph
                if x < id_min:
                    continue
                s = groups.setdefault(x, [[0, 0, 0, 0], [0, 0, 0, 0]])[direction]
                for k in range(3):
                    s[k] = (s[k] + add[k]) % MOD
                s[3] += 1
        if flags & BY_VOLUME:
            order = sorted(groups, key=lambda x: (-((groups[x][0][0] + groups[x][1][0]) % MOD), x))
        else:
            order = sorted(groups)
        matched = len(order)
        k = min(limit, ROWS_MAX, matched if cap is None else cap, matched)
        out = np.zeros(k, dtype=COUNTERPARTY_DTYPE)
        for n, x in enumerate(order[:k]):
            out["id_lo"][n], out["id_hi"][n] = x & U64_MAX, x >> 64
            for direction, sums in zip(("to", "from"), groups[x]):
                for name, v in zip(SUMS, sums):
                    out[direction + "_" + name + "_lo"][n], out[direction + "_" + name + "_hi"][n] = v & U64_MAX, v >> 64
                out[direction + "_transfers"][n] = sums[3]
        return out, matched, orphan
