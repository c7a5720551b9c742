"""The checker for get_account_statement_series (include/tbgpu.h tbgpu_get_account_statement_series)
— test infrastructure only.  `Series` is the header's definition over a resident export and the
current accounts, one brute-force pass over the export per (account, bucket), anchored at the current
balances:
  bucket k is (bounds[k], bounds[k+1]], a last bound of 0 open-ended;
  a record in the bucket adds to its side's *_pending_in / *_pending_out / *_posted_in by kind and one
  to its side's transfer count;
  closing = current(a) - the effects on a of every resident record above bounds[k+1], modulo 2^128;
  opening.x_pending = closing.x_pending - x_pending_in + x_pending_out, opening.x_posted =
  closing.x_posted - x_posted_in.
An account has a row in every bucket once its owner's table holds it and its own timestamp is not above
the last bound.  A post whose pending transfer is not resident is summed with P = its own amount, and
any such post above bounds[0] that names a found account drops `complete`.  It shares nothing with
the engine, and with tests/harness/statements.py only the field helpers."""
import numpy as np

from tests.harness.balances import MOD, PENDING, POST, VOID, balances_of, u128
from tigerbeetle_amd.types import STATEMENT_DTYPE, U64_MAX

SERIES_ROWS_MAX = 4095
SIDES = ("debits", "credits")


def valid_bounds(bounds):
    if len(bounds) < 2 or any(b == U64_MAX for b in bounds):
        return False
    if any(b == 0 for b in bounds[1:-1]):
        return False
    last = len(bounds) - 1
    return all(bounds[k] >= bounds[k - 1] or (k == last and bounds[k] == 0) for k in range(1, len(bounds)))


class Series:
    """resident: the engine's exported (live, resident) transfers; accounts: its exported accounts."""

    def __init__(self, resident, accounts):
        amount_of = {u128(t, "id"): u128(t, "amount") for t in resident}
        self.current = {u128(a, "id"): balances_of(a) for a in accounts}
        self.created = {u128(a, "id"): int(a["timestamp"]) for a in accounts}
        # Per account and side, its records: (timestamp, pending_in, pending_out, posted_in, orphan).
        self.by_account = {i: ([], []) for i in self.current}
        for t in resident:
            kind, amount = int(t["flags"]), u128(t, "amount")
            held, orphan = amount, False  # a void stores its pending transfer's amount
            if kind & PENDING:
                sums = (amount, 0, 0)
            elif kind & POST:
                held = amount_of.get(u128(t, "pending_id"))
                if held is None:
                    held, orphan = amount, True
                sums = (0, held, amount)
            elif kind & VOID:
                sums = (0, held, 0)
            else:
                sums = (0, 0, amount)
            for side, field in enumerate(("debit_account_id", "credit_account_id")):
                account = u128(t, field)
                if account in self.by_account:
                    self.by_account[account][side].append((int(t["timestamp"]),) + sums + (orphan,))

    def row(self, account, t_open, t_close):
        """The values of one (account, period): a dict of STATEMENT_DTYPE's 128-bit fields and the two counts."""
        values = {}
        for side, name in enumerate(SIDES):
            p_in = p_out = posted = count = above_pending = above_posted = 0
            for ts, r_in, r_out, r_posted, _ in self.by_account[account][side]:
                if ts <= t_open:
                    continue
                if t_close != 0 and ts > t_close:
                    above_pending += r_in - r_out
                    above_posted += r_posted
                else:
                    p_in, p_out, posted, count = p_in + r_in, p_out + r_out, posted + r_posted, count + 1
            # Above t_close counts whatever t_open is: the records at or below t_open are below t_close too.
            close_pending = (self.current[account][2 * side] - above_pending) % MOD
            close_posted = (self.current[account][2 * side + 1] - above_posted) % MOD
            values.update({"closing_%s_pending" % name: close_pending, "closing_%s_posted" % name: close_posted,
                           "opening_%s_pending" % name: (close_pending - p_in + p_out) % MOD,
                           "opening_%s_posted" % name: (close_posted - posted) % MOD,
                           name + "_pending_in": p_in % MOD, name + "_pending_out": p_out % MOD, name + "_posted_in": posted % MOD,
                           name[:-1] + "_transfers": count})
        return values

    def of(self, ids, bounds, cap=None):
        """(rows, matched, orphan): the header's answer for the request `ids` over the buckets of `bounds`."""
        bounds = [int(b) for b in bounds]
        empty = np.zeros(0, dtype=STATEMENT_DTYPE)
        if len(ids) == 0 or not valid_bounds(bounds):
            return empty, 0, False
        n_buckets, last = len(bounds) - 1, bounds[-1]
        found = [i for i in ids if i in self.current and (last == 0 or self.created[i] <= last)]
        orphan = any(r[4] and r[0] > bounds[0] for i in set(found) for side in self.by_account[i] for r in side)
        matched = len(found) * n_buckets
        count = matched if cap is None else min(matched, cap)
        out = np.zeros(count, dtype=STATEMENT_DTYPE)
        for n in range(count):
            account, k = found[n // n_buckets], n % n_buckets
            out["id_lo"][n], out["id_hi"][n] = account & U64_MAX, account >> 64
            for field, v in self.row(account, bounds[k], bounds[k + 1]).items():
                if field.endswith("_transfers"):
                    out[field][n] = v
                else:
                    out[field + "_lo"][n], out[field + "_hi"][n] = v & U64_MAX, v >> 64
        return out, matched, orphan


def bounds_sweep(steps, transfers, commit_timestamp):
    """Bounds lists over one scenario: prepare boundaries and timestamps inside prepares, 1, 2, 3, 7 and
    64 buckets, a first bound of 0, a last bound of 0 and one above commit_timestamp, equal
    neighbours, a bound at a record's timestamp and one below it."""
    stamps = [int(t) for t in np.sort(transfers["timestamp"])]
    b = [ts for _, _, ts, _ in steps]
    inside = [t for t in stamps[::97] if t not in b]
    assert len(inside) > 10 and len(b) > 12 and len(stamps) > 700
    at, below = stamps[len(stamps) // 2], stamps[len(stamps) // 3] - 1
    sweep = [
        [0, 0], [b[2], b[9]], [inside[1], 0], [0, inside[4]],                                  # one bucket
        [0, b[5], 0], [inside[0], inside[3]], [b[3], b[3], b[8]],                              # two
        [b[1], inside[2], b[7], commit_timestamp + 5],                                         # three, the last above commit_timestamp
        [0, b[1], b[2], b[2], b[2], inside[5], b[10], 0],                                      # seven, equal neighbours, open
        [below, below + 1, at - 1, at, at + 1, stamps[-1], stamps[-1], commit_timestamp + 1],  # seven, at and below a record
        [0] + stamps[10:650:10],                                                               # 64 buckets from before every record
        stamps[100:740:10] + [0],                                                              # 64 buckets, the last open
        inside[:8],
    ]
    # Around the accounts' own timestamps: accounts younger than the early buckets.
    created = [ts for _, op, ts, _ in steps if op == 128]
    marks = sorted({created[0] - 1, created[0], created[-1] - 1, created[-1]})
    sweep.append([0] + marks + [max(stamps[50], marks[-1]), 0])
    assert [len(s) - 1 for s in sweep].count(64) == 2 and all(valid_bounds(s) for s in sweep)
    return sweep
