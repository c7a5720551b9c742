"""Checkers for get_change_events (include/tbgpu.h tbgpu_get_change_events) — test infrastructure
only.  Each builds the ledger's events as CHANGE_EVENT_DTYPE records in timestamp order: the stored
transfer and its debit and credit account right after it:
  oracle_events  the reference restatement's own answer: every event committed on its own and the
                 stored transfer and both accounts fetched after each ok transfer (chain-free
                 scenarios only);
  spec_events    the backward definition of tbgpu.h over a resident export and the current accounts
                 (chains, eviction, orphan posts, anchors, missing accounts).
`select` cuts the events the way a filter does."""
import numpy as np

from tests.harness.balances import COLUMNS, MOD, POST, PENDING, balances_of, effect, u128
from tests.harness.oracle import OracleEngine
from tigerbeetle_amd.types import CHANGE_EVENT_DTYPE, CHANGE_EVENTS_MAX, U64_MAX

SIDES = (("debit_account", "debit_account_id", 0), ("credit_account", "credit_account_id", 2))


def oracle_events(steps, accounts_hint=4096, transfers_hint=1 << 15):
    """Events from a second oracle that commits one event per prepare at the timestamp the event has
    inside its prepare (ts - len + j + 1); ("setup", account, *balances) steps set balances."""
    oracle = OracleEngine(accounts_hint, transfers_hint)
    events = []
    for step in steps:
        if step[0] == "setup":
            oracle.set_balances(*step[1:])
            continue
        _, op, ts, batch = step
        for j, event in enumerate(batch):
            t = ts - len(batch) + j + 1
            if oracle.commit(op, t, event) or op != 129:
                continue
            ident = np.frombuffer(event, dtype=np.uint64, count=2)
            stored, state = oracle.fetch_transfers(ident)
            assert state[0] and int(stored["timestamp"][0]) == t
            ids = [u128(stored[0], "debit_account_id"), u128(stored[0], "credit_account_id")]
            accounts, found = oracle.fetch_accounts([[i & U64_MAX, i >> 64] for i in ids])
            assert found.all()
            ev = np.zeros(1, dtype=CHANGE_EVENT_DTYPE)
            ev["transfer"], ev["debit_account"], ev["credit_account"] = stored[0], accounts[0], accounts[1]
            events.append(ev)
    oracle.close()
    return np.concatenate(events) if events else np.zeros(0, dtype=CHANGE_EVENT_DTYPE)


def spec_events(resident, accounts):
    """tbgpu.h's definition: a block is the account's current record with balance_after(r, a) =
    current(a) - the effects on a of the resident records above r, modulo 2^128; a post whose pending
    transfer is not resident is summed with P = its own amount; an account that is not among
    `accounts` yields an all-zero block.  Returns (events, incomplete): incomplete[i] is True when an
    orphan post entered event i's sums (itself or a newer record naming one of its accounts — the
    engine reports any orphan of a page's scan) or one of its accounts is missing."""
    resident = resident[np.argsort(resident["timestamp"], kind="stable")]
    amount_of = {u128(t, "id"): u128(t, "amount") for t in resident}
    record = {u128(a, "id"): a for a in accounts}
    current = {i: list(balances_of(a)) for i, a in record.items()}
    events = np.zeros(len(resident), dtype=CHANGE_EVENT_DTYPE)
    incomplete = np.zeros(len(resident), dtype=bool)
    for i in range(len(resident) - 1, -1, -1):
        t = resident[i]
        flags, amount = int(t["flags"]), u128(t, "amount")
        pending_amount = amount
        if flags & POST and not flags & PENDING:
            pending_amount = amount_of.get(u128(t, "pending_id"))
            if pending_amount is None:
                pending_amount = amount
                incomplete[i] = True
        d_pending, d_posted = effect(flags, amount, pending_amount)
        events["transfer"][i] = t
        for block, name, at in SIDES:
            account = u128(t, name)
            if account not in record:
                incomplete[i] = True
                continue
            b = current[account]
            events[block][i] = record[account]
            for c, v in zip(COLUMNS, b):
                events[block][c + "_lo"][i], events[block][c + "_hi"][i] = v & U64_MAX, v >> 64
            b[at] = (b[at] - d_pending) % MOD
            b[at + 1] = (b[at + 1] - d_posted) % MOD
    return events, incomplete


def select(events, timestamp_min=0, timestamp_max=0, limit=CHANGE_EVENTS_MAX, out_cap_events=None):
    """(events, matched): the events cut as tbgpu_get_change_events cuts them."""
    ts = events["transfer"]["timestamp"]
    m = ts >= timestamp_min
    if timestamp_max:
        m &= ts <= timestamp_max
    sel = events[m]
    k = min(limit, CHANGE_EVENTS_MAX, limit if out_cap_events is None else out_cap_events)
    return sel[:k], len(sel)
