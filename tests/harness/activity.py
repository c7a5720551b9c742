"""The checker for get_active_accounts (include/tbgpu.h tbgpu_get_active_accounts) — test infrastructure
only.  `Activity` is the header's definition over a resident export, written straight from its text:
  a record matches when t_open < ts (<= t_close unless that is 0), its ledger is the filter's unless
  that is 0 and its code is the filter's unless that is 0; under DEBITS it feeds `debits` of the row of
  its debit account, under CREDITS `credits` of the row of its credit account (a record from an account
  to itself feeds both halves of one row); by kind it adds what a flow-matrix cell adds, and one
  transfer;
  a group is an account id at or above id_min with a matching record on a wanted side; rows come by id
  ascending, or by (debits.posted + credits.posted) mod 2^128 descending and then by id, or by
  debits.transfers + credits.transfers descending and then by id; the first
  min(limit, cap, 8191, groups) are written.
A post whose pending transfer is not resident is summed with P = its own amount and is an orphan
wherever it matched, whatever the sides, id_min and the limit.  No account table is read.  It shares
nothing with the engine but the field helpers."""
import numpy as np

from tests.harness.balances import MOD, PENDING, POST, VOID, u128
from tigerbeetle_amd.types import ACCOUNT_ACTIVITY_DTYPE, U64_MAX

ROWS_MAX = 8191
DEBITS, CREDITS, REVERSED, BY_VOLUME, BY_TRANSFERS = 1, 2, 4, 1 << 8, 1 << 9
SUMS = ("posted", "pending_in", "pending_out")
HALVES = ("debits", "credits")


def valid_filter(t_open, t_close, limit, flags, reserved0=bytes(2), reserved=bytes(16)):
    if not flags & (DEBITS | CREDITS) or flags & ~(DEBITS | CREDITS | BY_VOLUME | BY_TRANSFERS):
        return False
    if flags & BY_VOLUME and flags & BY_TRANSFERS:
        return False
    if any(reserved0) or any(reserved) or t_open == U64_MAX or t_close == U64_MAX or (t_close != 0 and t_close < t_open):
        return False
    return limit != 0


def half_sums(row, half):
    """(posted, pending_in, pending_out, transfers) of a row's `debits` or `credits` half."""
    return tuple(u128(row, half + "_" + s) for s in SUMS) + (int(row[half + "_transfers"]),)


def id_of(row):
    return u128(row, "id")


def volume_of(row):
    return (u128(row, "debits_posted") + u128(row, "credits_posted")) % MOD


def transfers_of(row):
    return int(row["debits_transfers"]) + int(row["credits_transfers"])


class Activity:
    """resident: the engine's exported (live, resident) transfers."""

    def __init__(self, resident):
        amount_of = {u128(t, "id"): u128(t, "amount") for t in resident}
        # Per record: (timestamp, ledger, code, debit account, credit account, (posted, pending_in, pending_out), orphan).
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
            self.records.append((int(t["timestamp"]), int(t["ledger"]), int(t["code"]), u128(t, "debit_account_id"),
                                 u128(t, "credit_account_id"), add, orphan))

    def of(self, t_open=0, t_close=0, flags=DEBITS | CREDITS, id_min=0, limit=ROWS_MAX, cap=None, ledger=0, code=0,
           reserved0=bytes(2), reserved=bytes(16)):
        """(rows, matched, orphan): the header's answer; orphan: a post without its resident pending
        transfer matched (`complete` is then 0, as it is once the engine has evicted anything)."""
        if not valid_filter(t_open, t_close, limit, flags, reserved0, reserved):
            return np.zeros(0, dtype=ACCOUNT_ACTIVITY_DTYPE), 0, False
        groups, orphan = {}, False
        for ts, led, cod, d, c, add, orph in self.records:
            if ts <= t_open or (t_close != 0 and ts > t_close) or (ledger != 0 and led != ledger) or (code != 0 and cod != code):
                continue
            orphan |= orph
            for x, half, bit in ((d, 0, DEBITS), (c, 1, CREDITS)):
                if not flags & bit or x < id_min:
                    continue
                s = groups.setdefault(x, [[0, 0, 0, 0], [0, 0, 0, 0]])[half]
                for k in range(3):
                    s[k] = (s[k] + add[k]) % MOD
                s[3] += 1
        if flags & BY_VOLUME:
            order = sorted(groups, key=lambda x: (-((groups[x][0][0] + groups[x][1][0]) % MOD), x))
        elif flags & BY_TRANSFERS:
            order = sorted(groups, key=lambda x: (-(groups[x][0][3] + groups[x][1][3]), x))
        else:
            order = sorted(groups)
        matched = len(order)
        k = min(limit, ROWS_MAX, matched if cap is None else cap, matched)
        out = np.zeros(k, dtype=ACCOUNT_ACTIVITY_DTYPE)
        for n, x in enumerate(order[:k]):
            out["id_lo"][n], out["id_hi"][n] = x & U64_MAX, x >> 64
            for half, sums in zip(HALVES, groups[x]):
                for name, v in zip(SUMS, sums):
                    out[half + "_" + name + "_lo"][n], out[half + "_" + name + "_hi"][n] = v & U64_MAX, v >> 64
                out[half + "_transfers"][n] = sums[3]
        return out, matched, orphan
