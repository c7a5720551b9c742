"""The checker for get_pending_transfers (include/tbgpu.h tbgpu_get_pending_transfers) — test
infrastructure only.  `PendingTransfers` is the header's definition over an engine's exported resident
transfers, its exported posted pairs ({pending timestamp, voided}) and a `now`:
  state(p)      = POSTED / VOIDED where the posted pairs say so; else EXPIRED when p.timeout != 0 and
                  min(p.timestamp + p.timeout * 10^9, 2^64-1) <= now; else OPEN;
  resolution(p) = the resident record with the post or void flag, and not `pending`, whose pending_id
                  is p.id, for a POSTED / VOIDED row; zero otherwise, and zero when none is resident.
`at` answers one filter as the call does: (rows, states, matched, resolved) — `resolved` is False when
a returned POSTED / VOIDED row lacks its resolution."""
import numpy as np

from tests.harness.balances import PENDING, POST, VOID, u128
from tigerbeetle_amd.types import (PENDING_EXPIRED, PENDING_OPEN, PENDING_POSTED, PENDING_ROW_DTYPE, PENDING_ROWS_MAX,
                                   PENDING_STATES, PENDING_VOIDED, U64_MAX)

NS = 10**9
U128_MAX = (1 << 128) - 1


def state_of(record, posted, now):
    """The single PENDING_* bit of the pending record at `now`; posted: {pending timestamp: voided}."""
    ts = int(record["timestamp"])
    if ts in posted:
        return PENDING_VOIDED if posted[ts] else PENDING_POSTED
    timeout = int(record["timeout"])
    if timeout and min(ts + timeout * NS, U64_MAX) <= now:
        return PENDING_EXPIRED
    return PENDING_OPEN


class PendingTransfers:
    """resident: the engine's exported (live, resident) transfers; posted: its exported posted pairs;
    commit_timestamp: what now = 0 stands for."""

    def __init__(self, resident, posted, commit_timestamp):
        self.commit_timestamp = int(commit_timestamp)
        self.posted = {int(ts): int(v) for ts, v in posted}
        order = np.argsort(resident["timestamp"], kind="stable")
        self.pending = [t for t in resident[order] if int(t["flags"]) & PENDING]
        self.resolving = {}
        self._states = {}  # by `now`
        for t in resident:
            flags = int(t["flags"])
            if flags & (POST | VOID) and not flags & PENDING:
                assert u128(t, "pending_id") not in self.resolving
                self.resolving[u128(t, "pending_id")] = t

    def states(self, now=0):
        """[(record, state)] of every resident pending record, by timestamp."""
        now = now or self.commit_timestamp
        if now not in self._states:
            self._states[now] = [(p, state_of(p, self.posted, now)) for p in self.pending]
        return self._states[now]

    def at(self, account_id=0, *, states=PENDING_STATES, debits=True, credits=True, reversed=False, timestamp_min=0,
           timestamp_max=0, now=0, limit=PENDING_ROWS_MAX, out_cap_rows=None, flags_extra=0):
        empty = (np.zeros(0, dtype=PENDING_ROW_DTYPE), np.zeros(0, dtype=np.uint8), 0, True)
        named = account_id != 0
        if (account_id == U128_MAX or (named and not (debits or credits)) or not states & PENDING_STATES
                or states & ~PENDING_STATES or flags_extra or U64_MAX in (timestamp_min, timestamp_max, now)
                or (timestamp_max and timestamp_max < timestamp_min) or limit == 0):
            return empty
        hits = []
        for p, st in self.states(now):
            ts = int(p["timestamp"])
            if ts < timestamp_min or (timestamp_max and ts > timestamp_max) or not st & states:
                continue
            if named and not ((debits and u128(p, "debit_account_id") == account_id)
                              or (credits and u128(p, "credit_account_id") == account_id)):
                continue
            hits.append((p, st))
        matched = len(hits)
        if reversed:
            hits.reverse()
        cap = min(limit, PENDING_ROWS_MAX) if out_cap_rows is None else out_cap_rows
        hits = hits[:min(limit, cap, PENDING_ROWS_MAX)]
        rows = np.zeros(len(hits), dtype=PENDING_ROW_DTYPE)
        out_states = np.zeros(len(hits), dtype=np.uint8)
        resolved = True
        for i, (p, st) in enumerate(hits):
            rows["pending"][i] = p
            out_states[i] = st
            if st & (PENDING_POSTED | PENDING_VOIDED):
                r = self.resolving.get(u128(p, "id"))
                if r is None:
                    resolved = False
                else:
                    rows["resolution"][i] = r
        return rows, out_states, matched, resolved
