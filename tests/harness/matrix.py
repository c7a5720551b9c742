"""The checker for get_account_flow_matrix (include/tbgpu.h tbgpu_get_account_flow_matrix) — test
infrastructure only.  `FlowMatrix` is the header's definition over a resident export and the current
accounts, written straight from its text:
  a list position is found when the table holds its id and the account is not younger than a non-zero
  t_close; found debit position of rank r and found credit position of rank q give cell r * found_credit + q;
  a record with t_open < ts (<= t_close unless that is 0) whose debit account is d and whose credit
  account is c adds to cell (d, c), wherever d and c stand in the lists, by kind, and one transfer.
A post whose pending transfer is not resident is summed with P = its own amount, and is an orphan only
where it entered a cell.  It shares nothing with the engine and nothing with
tests/harness/statements.py but the field helpers."""
import numpy as np

from tests.harness.balances import MOD, PENDING, POST, VOID, u128
from tigerbeetle_amd.types import FLOW_CELL_DTYPE, U64_MAX

CELLS_MAX = 4095
SUMS = ("posted", "pending_in", "pending_out")


def valid_period(t_open, t_close):
    return t_open != U64_MAX and t_close != U64_MAX and (t_close == 0 or t_close >= t_open)


def cell_sums(cell):
    """(posted, pending_in, pending_out, transfers) of a cell."""
    return tuple(u128(cell, s) for s in SUMS) + (int(cell["transfers"]),)


def pair_of(cell):
    return u128(cell, "debit_id"), u128(cell, "credit_id")


class FlowMatrix:
    """resident: the engine's exported (live, resident) transfers; accounts: its exported accounts."""

    def __init__(self, resident, accounts):
        amount_of = {u128(t, "id"): u128(t, "amount") for t in resident}
        self.created = {u128(a, "id"): int(a["timestamp"]) for a in accounts}
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

    def of(self, debit_ids, credit_ids, t_open, t_close, cap=None):
        """(cells, matched, orphan): the header's answer; orphan: a post without its resident pending
        transfer entered a cell of the matrix, under the cap or not (`complete` is then 0, as it is once
        the engine has evicted anything)."""
        empty = np.zeros(0, dtype=FLOW_CELL_DTYPE)
        if len(debit_ids) == 0 or len(credit_ids) == 0 or not valid_period(t_open, t_close):
            return empty, 0, False
        found = lambda ids: [i for i in ids if i in self.created and (t_close == 0 or self.created[i] <= t_close)]
        rows, cols = found(debit_ids), found(credit_ids)
        row_set, col_set = set(rows), set(cols)
        sums, orphan = {}, False
        for ts, d, c, add, orph in self.records:
            if ts <= t_open or (t_close != 0 and ts > t_close) or d not in row_set or c not in col_set:
                continue
            orphan |= orph
            s = sums.setdefault((d, c), [0, 0, 0, 0])
            for k in range(3):
                s[k] += add[k]
            s[3] += 1
        matched = len(rows) * len(cols)
        k = matched if cap is None else min(matched, cap)
        out = np.zeros(k, dtype=FLOW_CELL_DTYPE)
        for n in range(k):
            d, c = rows[n // len(cols)], cols[n % len(cols)]
            out["debit_id_lo"][n], out["debit_id_hi"][n] = d & U64_MAX, d >> 64
            out["credit_id_lo"][n], out["credit_id_hi"][n] = c & U64_MAX, c >> 64
            s = sums.get((d, c), (0, 0, 0, 0))
            for name, v in zip(SUMS, s):
                out[name + "_lo"][n], out[name + "_hi"][n] = (v % MOD) & U64_MAX, (v % MOD) >> 64
            out["transfers"][n] = s[3]
        return out, matched, orphan
