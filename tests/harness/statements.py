"""The checker for get_account_statements (include/tbgpu.h tbgpu_get_account_statements) — test
infrastructure only.  `Statements` is the header's definition over a resident export and the current
accounts, written straight from its table and anchored at the current balances:
  a record in (t_open, t_close] adds to its side's *_pending_in / *_pending_out / *_posted_in by kind
  and one to its side's transfer count;
  closing = current(a) - the effects on a of every resident record above t_close, modulo 2^128;
  opening.x_pending = closing.x_pending - x_pending_in + x_pending_out, opening.x_posted =
  closing.x_posted - x_posted_in.
A post whose pending transfer is not resident is summed with P = its own amount.  It shares nothing
with the engine and nothing with tests/harness/asof.py but the field helpers."""
import numpy as np

from tests.harness.balances import COLUMNS, MOD, PENDING, POST, VOID, balances_of, u128
from tigerbeetle_amd.types import STATEMENT_DTYPE, U64_MAX

STATEMENTS_MAX = 4095
SUMS = ("pending_in", "pending_out", "posted_in")
SIDES = ("debits", "credits")


def valid_period(t_open, t_close):
    return t_open != U64_MAX and t_close != U64_MAX and (t_close == 0 or t_close >= t_open)


def flows(flags, amount, pending_amount):
    """(pending_in, pending_out, posted_in) of one record on its side: the header's table."""
    if flags & PENDING:
        return amount, 0, 0
    if flags & POST:
        return 0, pending_amount, amount
    if flags & VOID:
        return 0, pending_amount, 0
    return 0, 0, amount


def balances(row, when):
    return tuple(u128(row, when + "_" + c) for c in COLUMNS)


def sums(row):
    """The six sums and two counts of a row: ((debit side), (credit side)), each (in, out, posted, n)."""
    return tuple(tuple(u128(row, side + "_" + s) for s in SUMS) + (int(row[side[:-1] + "_transfers"]),) for side in SIDES)


class Statements:
    """resident: the engine's exported (live, resident) transfers; accounts: its exported accounts."""

    def __init__(self, resident, accounts):
        amount_of = {u128(t, "id"): u128(t, "amount") for t in resident}
        self.current = {u128(a, "id"): balances_of(a) for a in accounts}
        self.created = {u128(a, "id"): int(a["timestamp"]) for a in accounts}
        # Per record: (timestamp, (debit account, credit account), (pending_in, pending_out, posted_in), orphan).
        self.records = []
        for t in resident:
            kind, amount = int(t["flags"]), u128(t, "amount")
            pending_amount, orphan = amount, False  # a void stores its pending transfer's amount
            if kind & POST and not kind & PENDING:
                pending_amount = amount_of.get(u128(t, "pending_id"))
                if pending_amount is None:
                    pending_amount, orphan = amount, True
            self.records.append((int(t["timestamp"]), (u128(t, "debit_account_id"), u128(t, "credit_account_id")),
                                 flows(kind, amount, pending_amount), orphan))

    def of(self, ids, t_open, t_close, cap=None):
        """(rows, matched, orphan): the header's answer for the request `ids` over (t_open, t_close];
        orphan: a post without its resident pending transfer entered a sum (`complete` is then 0, as
        it is once the engine has evicted anything)."""
        empty = np.zeros(0, dtype=STATEMENT_DTYPE)
        if len(ids) == 0 or not valid_period(t_open, t_close):
            return empty, 0, False
        found = [i for i in ids if i in self.current and (t_close == 0 or self.created[i] <= t_close)]
        # Per found account and side: above = [pending, posted] effects above t_close; inside = [in, out, posted, n].
        above = {i: [[0, 0], [0, 0]] for i in found}
        inside = {i: [[0, 0, 0, 0], [0, 0, 0, 0]] for i in found}
        orphan = False
        for ts, pair, (p_in, p_out, posted), orph in self.records:
            if ts <= t_open:
                continue
            later = t_close != 0 and ts > t_close
            for side, account in enumerate(pair):
                if account not in above:
                    continue
                orphan |= orph
                if later:
                    above[account][side][0] += p_in - p_out
                    above[account][side][1] += posted
                else:
                    s = inside[account][side]
                    s[0] += p_in
                    s[1] += p_out
                    s[2] += posted
                    s[3] += 1
        k = len(found) if cap is None else min(len(found), cap)
        out = np.zeros(k, dtype=STATEMENT_DTYPE)
        for n, i in enumerate(found[:k]):
            out["id_lo"][n], out["id_hi"][n] = i & U64_MAX, i >> 64
            for side, name in enumerate(SIDES):
                p_in, p_out, posted, count = inside[i][side]
                close_pending = (self.current[i][2 * side] - above[i][side][0]) % MOD
                close_posted = (self.current[i][2 * side + 1] - above[i][side][1]) % MOD
                values = {"closing_%s_pending" % name: close_pending, "closing_%s_posted" % name: close_posted,
                          "opening_%s_pending" % name: (close_pending - p_in + p_out) % MOD,
                          "opening_%s_posted" % name: (close_posted - posted) % MOD,
                          name + "_pending_in": p_in % MOD, name + "_pending_out": p_out % MOD, name + "_posted_in": posted % MOD}
                for field, v in values.items():
                    out[field + "_lo"][n], out[field + "_hi"][n] = v & U64_MAX, v >> 64
                out[name[:-1] + "_transfers"][n] = count
        return out, len(found), orphan


def ids_body(ids):
    return b"".join(int(i).to_bytes(16, "little") for i in ids)


def request_of(accounts, absent):
    """Every account reversed, absent ids, the reserved ids and repeats (tests/test_asof_checkers.py's shape)."""
    ids = [u128(a, "id") for a in accounts]
    return ids[::-1] + [absent[0], 0, (1 << 128) - 1] + ids[:5] + [absent[1]] + ids[3:4]


def sweep_pairs(steps, transfers, commit_timestamp):
    """(t_open, t_close) pairs over one scenario: prepare boundaries, timestamps inside prepares, 0, 1,
    commit_timestamp and commit_timestamp + 1 at either end, t_open == t_close and (0, 0)."""
    stamps = np.sort(transfers["timestamp"])
    boundaries = [ts for _, _, ts, _ in steps]
    inside = [int(t) for t in stamps[::97] if int(t) not in boundaries]
    assert len(inside) > 10
    b = boundaries
    pairs = [(0, 0), (0, 1), (1, 0), (1, 1), (0, commit_timestamp), (commit_timestamp, 0), (commit_timestamp, commit_timestamp + 1),
             (commit_timestamp + 1, 0), (0, b[0]), (b[0], b[1]), (b[1], b[2]), (b[1], 0), (b[len(b) // 2], b[len(b) // 2])]
    pairs += [(b[i], b[i + 1]) for i in range(2, len(b) - 1, 3)]
    pairs += [(b[i], b[j]) for i, j in ((2, len(b) - 1), (5, 12), (len(b) // 2, len(b) - 2))]
    pairs += list(zip(inside[:-1:2], inside[1::2]))
    pairs += [(inside[0], inside[0]), (inside[3], 0), (0, inside[4]), (inside[1], b[len(b) // 2]), (b[3], inside[-1])]
    assert all(valid_period(o, c) for o, c in pairs)
    return pairs
