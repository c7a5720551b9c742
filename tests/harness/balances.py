"""Checkers for get_account_balances (include/tbgpu.h tbgpu_get_account_balances) — test
infrastructure only.  Each builds, per account, the list of (timestamp, side, balances) of its
transfers in timestamp order, where balances = (debits_pending, debits_posted, credits_pending,
credits_posted) right after that transfer:
  oracle_rows  the reference restatement's own answer: every event committed on its own and both
               accounts fetched after each ok transfer (chain-free scenarios only);
  replay_rows  a forward replay from zero over exported transfers (any scenario, whole ledger);
  spec_rows    the backward definition of tbgpu.h over a resident export and the current balances
               (after eviction; orphan posts).
`pack` turns a list into ACCOUNT_BALANCE_DTYPE rows and `select` cuts them the way a filter does."""
import numpy as np

from tests.harness.oracle import OracleEngine
from tigerbeetle_amd.types import ACCOUNT_BALANCE_DTYPE, BATCH_MAX, U64_MAX, TransferFlags

COLUMNS = ("debits_pending", "debits_posted", "credits_pending", "credits_posted")
MOD = 1 << 128
PENDING = int(TransferFlags.pending)
POST = int(TransferFlags.post_pending_transfer)
VOID = int(TransferFlags.void_pending_transfer)


def u128(record, name):
    return (int(record[name + "_hi"]) << 64) | int(record[name + "_lo"])


def balances_of(account):
    return tuple(u128(account, c) for c in COLUMNS)


def effect(flags, amount, pending_amount):
    """(d *_pending, d *_posted) of one record on its side (src/state_machine.zig:872-878, :997-1007)."""
    if flags & PENDING:
        return amount, 0
    if flags & POST:
        return -pending_amount, amount
    if flags & VOID:
        return -pending_amount, 0
    return 0, amount


def oracle_rows(steps, accounts_hint=4096, transfers_hint=1 << 15):
    """{account: [(timestamp, side, balances)]} from a second oracle that commits one event per
    prepare at the timestamp the event has inside its prepare (ts - len + j + 1)."""
    oracle = OracleEngine(accounts_hint, transfers_hint)
    rows = {}
    for step in steps:
        if step[0] == "setup":
            oracle.set_balances(*step[1:])
            continue
        _, op, ts, events = step
        for j, event in enumerate(events):
            t = ts - len(events) + j + 1
            if oracle.commit(op, t, event) or op != 129:
                continue
            ident = np.frombuffer(event, dtype=np.uint64, count=2)
            stored, state = oracle.fetch_transfers(ident)
            assert state[0] and int(stored["timestamp"][0]) == t
            ids = [u128(stored[0], "debit_account_id"), u128(stored[0], "credit_account_id")]
            accounts, found = oracle.fetch_accounts([[i & U64_MAX, i >> 64] for i in ids])
            assert found.all()
            for side, i, account in zip("dc", ids, accounts):
                rows.setdefault(i, []).append((t, side, balances_of(account)))
    oracle.close()
    return rows


def replay_rows(transfers):
    """Forward from zero over a whole ledger's exported transfers, in timestamp order."""
    transfers = transfers[np.argsort(transfers["timestamp"], kind="stable")]
    amount_of = {u128(t, "id"): u128(t, "amount") for t in transfers if int(t["flags"]) & PENDING}
    balances, rows = {}, {}
    for t in transfers:
        flags, amount = int(t["flags"]), u128(t, "amount")
        pending_amount = amount_of[u128(t, "pending_id")] if flags & (POST | VOID) else 0
        d_pending, d_posted = effect(flags, amount, pending_amount)
        for side, name, at in (("d", "debit_account_id", 0), ("c", "credit_account_id", 2)):
            account = u128(t, name)
            b = balances.setdefault(account, [0, 0, 0, 0])
            b[at] += d_pending
            b[at + 1] += d_posted
            assert min(b) >= 0 and max(b) < MOD
            rows.setdefault(account, []).append((int(t["timestamp"]), side, tuple(b)))
    return rows


def spec_rows(resident, accounts):
    """tbgpu.h's definition: balance_after(r) = current - the effects of the resident records above r,
    modulo 2^128; a post whose pending transfer is not resident is summed with P = its own amount.
    Returns (rows, orphans): orphans[account] = timestamps of its orphan posts."""
    resident = resident[np.argsort(resident["timestamp"], kind="stable")]
    amount_of = {u128(t, "id"): u128(t, "amount") for t in resident}
    current = {u128(a, "id"): list(balances_of(a)) for a in accounts}
    rows, orphans = {}, {}
    for t in resident[::-1]:
        flags, amount, ts = int(t["flags"]), u128(t, "amount"), int(t["timestamp"])
        pending_amount = amount
        if flags & POST and not flags & PENDING:
            pending_amount = amount_of.get(u128(t, "pending_id"))
            if pending_amount is None:
                pending_amount = amount
                for name in ("debit_account_id", "credit_account_id"):
                    orphans.setdefault(u128(t, name), []).append(ts)
        d_pending, d_posted = effect(flags, amount, pending_amount)
        for side, name, at in (("d", "debit_account_id", 0), ("c", "credit_account_id", 2)):
            account = u128(t, name)
            b = current[account]
            rows.setdefault(account, []).append((ts, side, tuple(b)))
            b[at] = (b[at] - d_pending) % MOD
            b[at + 1] = (b[at + 1] - d_posted) % MOD
    return {a: r[::-1] for a, r in rows.items()}, orphans


def pack(items):
    """An account's list as (ACCOUNT_BALANCE_DTYPE rows, is-debit-side mask), for `select`."""
    rows = np.zeros(len(items), dtype=ACCOUNT_BALANCE_DTYPE)
    for i, (ts, _, balances) in enumerate(items):
        rows["timestamp"][i] = ts
        for c, v in zip(COLUMNS, balances):
            rows[c + "_lo"][i], rows[c + "_hi"][i] = v & U64_MAX, v >> 64
    return rows, np.array([side == "d" for _, side, _ in items], dtype=bool)


def select(packed, debits=True, credits=True, reversed=False, timestamp_min=0, timestamp_max=0, limit=8190,
           out_cap_records=None):
    """(rows, matched): an account's packed list cut as get_account_transfers cuts its transfers."""
    rows, debit_side = packed
    m = (debit_side & debits) | (~debit_side & credits)
    m &= rows["timestamp"] >= timestamp_min
    if timestamp_max:
        m &= rows["timestamp"] <= timestamp_max
    sel = rows[m]
    if reversed:
        sel = sel[::-1]
    k = min(limit, BATCH_MAX, limit if out_cap_records is None else out_cap_records)
    return sel[:k], len(sel)
