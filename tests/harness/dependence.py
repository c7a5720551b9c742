"""Host model of the engine's dependence classification (which events of a create_transfers pass the
ordered fallback commits): a restatement of the rules of tigerbeetle_amd/csrc/k_validate.h (hazard
bits) and k_resolve.h (tb_classify, chain propagation), for one pass over a known pre-pass state.

It is not the reference's logic — the reference has no notion of dependence — but the engine's own
rule, written independently, so a GPU test can assert that `stats["dependent_events"]` is exactly
this count (VERDICT r3 What's weak #1: the classification must not depend on scheduling).

Model limits: the pass's global overflow certificate must hold (bound + S < 2^128; true of every
workload without near-overflow balances), balances must never have been set directly (no `setup`
steps), and 32-bit fingerprint collisions of distinct ids are ignored.
"""
from tigerbeetle_amd.types import TRANSFER_DTYPE, AccountFlags as AF, TransferFlags as TF, U128_MAX

import numpy as np

LIMITS = int(AF.debits_must_not_exceed_credits) | int(AF.credits_must_not_exceed_debits)
PADDING = 0xFFC0  # TransferFlags bits 6..15
# Plain ints: an IntFlag operand makes every `&` below build an enum member (most of the model's time).
LINKED, PENDING = int(TF.linked), int(TF.pending)
POST, VOID = int(TF.post_pending_transfer), int(TF.void_pending_transfer)
BAL_DEBIT, BAL_CREDIT = int(TF.balancing_debit), int(TF.balancing_credit)


_COLUMNS = ("id_lo", "id_hi", "debit_account_id_lo", "debit_account_id_hi", "credit_account_id_lo",
            "credit_account_id_hi", "amount_lo", "amount_hi", "pending_id_lo", "pending_id_hi", "timeout", "ledger", "code",
            "flags", "timestamp")


def _u128(lo, hi):
    return int(lo) | (int(hi) << 64)


def dependent_count(prepares, accounts, existing_ids=frozenset()):
    """prepares: list of transfer bodies (bytes) of ONE device pass, in order; accounts: {id: (flags,
    ledger)} live before the pass; existing_ids: transfer ids stored before the pass (a post / void
    of such a pending transfer is not modelled: the pass must hold every pending it names).
    Returns the number of events the engine classifies dependent."""
    evs = []  # per event: dict
    for p, body in enumerate(prepares):
        rec = np.frombuffer(body, dtype=TRANSFER_DTYPE)
        L = len(rec)
        # Columns as Python ints at once (a pass of half a million events: field reads per record
        # took ten seconds).
        c = {name: rec[name].tolist() for name in _COLUMNS}
        for j in range(L):
            evs.append(dict(p=p, j=j, L=L, id=_u128(c["id_lo"][j], c["id_hi"][j]),
                            dr=_u128(c["debit_account_id_lo"][j], c["debit_account_id_hi"][j]),
                            cr=_u128(c["credit_account_id_lo"][j], c["credit_account_id_hi"][j]),
                            amount=_u128(c["amount_lo"][j], c["amount_hi"][j]),
                            pid=_u128(c["pending_id_lo"][j], c["pending_id_hi"][j]), timeout=c["timeout"][j],
                            ledger=c["ledger"][j], code=c["code"][j], flags=c["flags"][j], ts=c["timestamp"][j]))
    # -- kernel 1 (k_validate.h): who claims its id, pv keys, hazard bits ---------------------------
    for e in evs:
        f = e["flags"]
        e.update(claims=False, pv_key=False, accts=False, limit=False, bal=False, ok=False, selfdep=False)
        if (f & LINKED) and e["j"] == e["L"] - 1:
            continue  # linked_event_chain_open
        if e["ts"] != 0:
            continue  # timestamp_must_be_zero
        if f & PADDING or e["id"] in (0, U128_MAX):
            continue
        if f & (POST | VOID):
            if (f & POST) and (f & VOID):
                continue
            if f & (PENDING | BAL_DEBIT | BAL_CREDIT):
                continue
            if e["pid"] in (0, U128_MAX) or e["pid"] == e["id"] or e["timeout"] != 0:
                continue
            e["pv"] = True
            e["pv_key"] = True
            e["claims"] = True
            continue
        if e["dr"] in (0, U128_MAX) or e["cr"] in (0, U128_MAX) or e["dr"] == e["cr"] or e["pid"] != 0:
            continue
        if not (f & PENDING) and e["timeout"] != 0:
            continue
        if not (f & (BAL_DEBIT | BAL_CREDIT)) and e["amount"] == 0:
            continue
        if e["ledger"] == 0 or e["code"] == 0:
            continue
        e["claims"] = True  # the id's home entry is claimed with the account probes (:211-232)
        da, ca = accounts.get(e["dr"]), accounts.get(e["cr"])
        if da is None or ca is None or da[1] != ca[1] or e["ledger"] != da[1]:
            continue
        e["accts"] = True
        e["limit"] = bool((da[0] | ca[0]) & LIMITS)
        e["bal"] = bool(f & (BAL_DEBIT | BAL_CREDIT))
    # Claims: an id claimed by two or more events of the pass, and stored before by none, collides.
    claimers = {}
    for e in evs:
        if e["claims"]:
            claimers.setdefault(e["id"], []).append(e)
    collided = {i for i, c in claimers.items() if len(c) >= 2 and i not in existing_ids}
    claimed_in_pass = {i for i in claimers if i not in existing_ids}
    pv_keys = {}
    for e in evs:
        if e["pv_key"]:
            pv_keys[e["pid"]] = pv_keys.get(e["pid"], 0) + 1
    any_dup = bool(collided) or any(n >= 2 for n in pv_keys.values())
    any_pv = bool(pv_keys)
    marked = set()
    # Intrinsic ok-ness of an event that reached the account checks (create_transfer): the exists
    # check (id stored before) and the timeout overflow are the failures left after them.
    for e in evs:
        if e.get("pv"):
            e["selfdep"] = e["id"] in collided
            continue
        if not e["accts"]:
            continue
        if e["bal"]:  # marks before the id check (k_validate.h: balancing accounts marked up front)
            if e["flags"] & BAL_DEBIT:
                marked.add(e["dr"])
            if e["flags"] & BAL_CREDIT:
                marked.add(e["cr"])
        exists = e["id"] in existing_ids
        e["selfdep"] = e["id"] in collided
        e["ok"] = not exists  # timeouts in workloads never overflow u64 nanoseconds
    any_bal = bool(marked)
    # -- kernel 2 (k_resolve.h tb_classify) ----------------------------------------------------------
    for e in evs:
        dep = e["selfdep"]
        if not dep and any_dup:
            if e["claims"] and not e.get("pv") and e["id"] in collided:
                dep = True
            if e["pv_key"] and pv_keys.get(e["pid"], 0) >= 2:
                dep = True
        if not dep and any_pv:
            if (e["accts"] or e["pv_key"]) and e["id"] in pv_keys:
                dep = True
            if e["pv_key"] and e["pid"] in claimed_in_pass:
                dep = True
        if not dep and e["accts"] and e["ok"]:
            if e["bal"] or e["limit"]:
                dep = True
            elif any_bal and (e["dr"] in marked or e["cr"] in marked):
                dep = True
        e["dep"] = dep
    # Linked chains: a chain with a dependent member is dependent as a whole (execute :628-692).
    total = 0
    i = 0
    while i < len(evs):
        j = i
        while j + 1 < len(evs) and evs[j + 1]["p"] == evs[i]["p"] and (evs[j]["flags"] & LINKED):
            j += 1
        members = evs[i:j + 1]
        if evs[i]["flags"] & LINKED and len(members) >= 1:
            if any(m["dep"] for m in members):
                total += len(members)
        else:
            total += sum(1 for m in members if m["dep"])
        i = j + 1
    return total
