"""The checker of tests/harness/pending.py against the oracle, before any GPU answer is held to it: the
posted state against the oracle's posted groove and its resident post / void records, expiry against
the replies the oracle gives to voids that arrive at a later timestamp.  No GPU."""
import numpy as np
import pytest

from tests.harness.balances import PENDING, POST, VOID, u128
from tests.harness.oracle import OracleEngine
from tests.harness.pending import NS, PendingTransfers, state_of
from tests.harness.workload import make_scenario
from tests.test_balance_checkers import CHAIN_FREE, QUERY_SCENARIO
from tigerbeetle_amd.types import (PENDING_EXPIRED, PENDING_OPEN, PENDING_POSTED, PENDING_ROW_DTYPE, PENDING_VOIDED, RESULT_DTYPE,
                                   U64_MAX, CreateTransferResult, pack_account, pack_transfer)

EXPIRED = int(CreateTransferResult.pending_transfer_expired)
SCENARIOS = {7: lambda: make_scenario(7, **CHAIN_FREE), 2025: lambda: make_scenario(2025, **QUERY_SCENARIO)}
# Counted on the CPU at now = commit_timestamp: open, expired, posted, voided; the open rows with
# timeout 0; partial posts; rows that expire between commit_timestamp and 3 s later.
COUNTS = {7: ((26, 12, 11, 4), 14, None, 3), 2025: ((286, 177, 73, 39), 211, 12, 20)}


def committed(seed):
    sc = SCENARIOS[seed]()
    oracle = OracleEngine(4096, 1 << 15)
    for _, op, ts, events in sc.steps:
        oracle.commit(op, ts, b"".join(events))
    return sc, oracle


def counts(checker, now=0):
    states = [st for _, st in checker.states(now)]
    return tuple(states.count(s) for s in (PENDING_OPEN, PENDING_EXPIRED, PENDING_POSTED, PENDING_VOIDED))


@pytest.mark.parametrize("seed", sorted(SCENARIOS))
def test_posted_state_equals_the_oracle(seed):
    _, oracle = committed(seed)
    transfers, posted = oracle.export_transfers(), oracle.export_posted()
    checker = PendingTransfers(transfers, posted, oracle.commit_timestamp)
    got = {(int(p["timestamp"]), 1 if st == PENDING_VOIDED else 0) for p, st in checker.states()
           if st in (PENDING_POSTED, PENDING_VOIDED)}
    assert got == {(int(ts), int(v)) for ts, v in posted} and len(got) == len(posted)
    # ... and the resident post / void records say the same: nothing was evicted, so every resolved
    # row has exactly its record and no unresolved row has one.
    rows, states, matched, resolved = checker.at()
    assert matched == len(rows) == len(checker.pending) and resolved
    for row, st in zip(rows, states):
        flags = int(row["resolution"]["flags"])
        if st == PENDING_POSTED:
            assert flags & POST and not flags & (PENDING | VOID)
        elif st == PENDING_VOIDED:
            assert flags & VOID and not flags & (PENDING | POST)
        else:
            assert row["resolution"].tobytes() == bytes(128)
        if st in (PENDING_POSTED, PENDING_VOIDED):
            assert u128(row["resolution"], "pending_id") == u128(row["pending"], "id")
            assert int(row["resolution"]["timestamp"]) > int(row["pending"]["timestamp"])
    oracle.close()


@pytest.mark.parametrize("seed", sorted(SCENARIOS))
def test_not_vacuous(seed):
    _, oracle = committed(seed)
    transfers = oracle.export_transfers()
    checker = PendingTransfers(transfers, oracle.export_posted(), oracle.commit_timestamp)
    by_state, open_without_timeout, partial, later = COUNTS[seed]
    assert counts(checker) == by_state and min(by_state) > 0
    assert sum(1 for p, st in checker.states() if st == PENDING_OPEN and int(p["timeout"]) == 0) == open_without_timeout
    after = counts(checker, oracle.commit_timestamp + 3 * NS)
    assert after[1] - by_state[1] == by_state[0] - after[0] == later and after[2:] == by_state[2:]
    if partial is not None:
        rows, states, _, _ = checker.at(states=PENDING_POSTED)
        assert sum(1 for r in rows if u128(r["resolution"], "amount") < u128(r["pending"], "amount")) == partial
    # `now` is the clock for expiry alone.
    assert counts(checker, 1)[1] == 0 and counts(checker, 1)[2:] == by_state[2:]
    assert counts(checker, U64_MAX - 1)[0] == open_without_timeout
    oracle.close()


@pytest.mark.parametrize("seed", sorted(SCENARIOS))
def test_expiry_equals_the_oracles_replies(seed):
    """One more prepare, 3 s after the last: a void per unresolved pending transfer.  The void that is
    event j arrives at ts - len + j + 1; the checker at that `now` says EXPIRED exactly where the reply
    says pending_transfer_expired and OPEN exactly where the void went through."""
    sc, oracle = committed(seed)
    checker = PendingTransfers(oracle.export_transfers(), oracle.export_posted(), oracle.commit_timestamp)
    unresolved = [p for p, st in checker.states(1) if st == PENDING_OPEN]
    assert len(unresolved) == sum(counts(checker)[:2])
    ts = sc.steps[-1][2] + 3 * NS
    body = b"".join(pack_transfer(id=(1 << 100) + j, pending_id=u128(p, "id"), flags=VOID) for j, p in enumerate(unresolved))
    reply = np.frombuffer(oracle.commit(129, ts, body), dtype=RESULT_DTYPE)
    assert set(reply["result"].tolist()) == {EXPIRED}
    failed = set(reply["index"].tolist())
    seen = {PENDING_OPEN: 0, PENDING_EXPIRED: 0}
    for j, p in enumerate(unresolved):
        now = ts - len(unresolved) + j + 1
        st = state_of(p, checker.posted, now)
        assert st == (PENDING_EXPIRED if j in failed else PENDING_OPEN), j
        seen[st] += 1
    assert seen[PENDING_OPEN] > 0 and seen[PENDING_EXPIRED] == len(failed) > 0
    # The voids that went through are the posted groove's new entries.
    after = PendingTransfers(oracle.export_transfers(), oracle.export_posted(), oracle.commit_timestamp)
    assert counts(after)[3] == counts(checker)[3] + seen[PENDING_OPEN]
    oracle.close()


def hand_made(void_at):
    """A pending transfer with timeout 2 s at timestamp 1000 and a void that arrives at `void_at`."""
    oracle = OracleEngine(64, 1 << 10)
    assert oracle.commit(128, 100, b"".join(pack_account(id=i, ledger=1, code=1) for i in (1, 2))) == b""
    assert oracle.commit(129, 1000, pack_transfer(id=10, debit_account_id=1, credit_account_id=2, amount=5, ledger=1, code=1,
                                                  timeout=2, flags=PENDING)) == b""
    pending = oracle.export_transfers()[0]
    reply = np.frombuffer(oracle.commit(129, void_at, pack_transfer(id=11, pending_id=10, flags=VOID)), dtype=RESULT_DTYPE)
    return oracle, pending, reply


def test_the_expiry_edge():
    edge = 1000 + 2 * NS
    oracle, pending, reply = hand_made(edge)
    assert reply["result"].tolist() == [EXPIRED]
    assert state_of(pending, {}, edge) == PENDING_EXPIRED
    checker = PendingTransfers(oracle.export_transfers(), oracle.export_posted(), oracle.commit_timestamp)
    rows, states, matched, resolved = checker.at(now=edge)
    assert states.tolist() == [PENDING_EXPIRED] and matched == 1 and resolved and rows.dtype == PENDING_ROW_DTYPE
    assert rows["resolution"].tobytes() == bytes(128)
    assert checker.at(now=edge - 1)[1].tolist() == [PENDING_OPEN]
    oracle.close()
    oracle, pending, reply = hand_made(edge - 1)
    assert len(reply) == 0
    assert state_of(pending, {}, edge - 1) == PENDING_OPEN
    checker = PendingTransfers(oracle.export_transfers(), oracle.export_posted(), oracle.commit_timestamp)
    rows, states, matched, resolved = checker.at(now=edge)  # voided whatever the clock says
    assert states.tolist() == [PENDING_VOIDED] and resolved
    assert u128(rows[0]["resolution"], "id") == 11 and int(rows[0]["resolution"]["timestamp"]) == edge - 1
    oracle.close()
    # A sum that would wrap saturates and never expires.
    late = np.zeros(1, dtype=pending.dtype)[0]
    late["timestamp"], late["timeout"] = U64_MAX - 5, 1
    assert state_of(late, {}, U64_MAX - 1) == PENDING_OPEN


def test_filters_of_the_checker():
    _, oracle = committed(7)
    checker = PendingTransfers(oracle.export_transfers(), oracle.export_posted(), oracle.commit_timestamp)
    every, states, matched, _ = checker.at()
    assert (np.diff(every["pending"]["timestamp"].astype(np.int64)) > 0).all()
    account = u128(every[0]["pending"], "debit_account_id")
    d = checker.at(account, credits=False)[2]
    c = checker.at(account, debits=False)[2]
    assert d > 0 and d + c == checker.at(account)[2] < matched
    assert checker.at(account, debits=False, credits=False)[2] == 0 and checker.at(0, debits=False, credits=False)[2] == matched
    rev = checker.at(reversed=True, limit=3)
    assert rev[0].tobytes() == every[::-1][:3].tobytes() and rev[2] == matched
    mid = int(every[len(every) // 2]["pending"]["timestamp"])
    assert checker.at(timestamp_min=mid)[2] + checker.at(timestamp_max=mid - 1)[2] == matched
    for bad in (dict(states=0), dict(limit=0), dict(now=U64_MAX), dict(timestamp_min=U64_MAX), dict(timestamp_max=U64_MAX),
                dict(timestamp_min=5, timestamp_max=4), dict(account_id=(1 << 128) - 1), dict(flags_extra=8)):
        assert checker.at(**bad)[2] == 0
    assert len(checker.at(out_cap_rows=2)[0]) == 2 and len(checker.at(limit=5, out_cap_rows=9)[0]) == 5
    oracle.close()
