"""The claims of tests/harness/late_apply.py's builder, checked on the oracle (no GPU): what
tests/test_gpu_late_apply.py relies on to reach tb_flow's sequential replay with late balance adds on
the same accounts."""
import numpy as np
import pytest

from tests.harness.balances import u128
from tests.harness.dependence import dependent_count
from tests.harness.late_apply import (BATCH, CHAIN, EVENTS, LATE_FROM, N_ACCOUNTS, PENDINGS, PREPARES, VARIANTS, LateApply)
from tests.harness.oracle import OracleEngine
from tigerbeetle_amd.types import RESULT_DTYPE, CreateTransferResult as R

COLUMNS = ("debits_pending", "debits_posted", "credits_pending", "credits_posted")


@pytest.mark.parametrize("variant", VARIANTS)
def test_builder_claims(variant):
    sc = LateApply(variant)
    assert len(sc.events) == EVENTS == 64 * 8190 and len(sc.bodies) == PREPARES and len(sc.account_ids) == 8
    oracle = OracleEngine(64, 1 << 20)
    sc.commit_setup(oracle)
    replies = oracle.commit_many(129, sc.timestamps, sc.bodies)
    # linked_event_failed exactly on the broken chains' members, and the member that broke them.
    failed = np.zeros(EVENTS, dtype=bool)
    other = np.zeros(EVENTS, dtype=bool)
    for k, reply in enumerate(replies):
        rows = np.frombuffer(reply, dtype=RESULT_DTYPE)
        at = k * BATCH + rows["index"].astype(np.int64)
        failed[at[rows["result"] == R.linked_event_failed]] = True
        other[at[rows["result"] != R.linked_event_failed]] = True
        assert set(rows["result"].tolist()) <= {int(R.linked_event_failed), int(R.accounts_must_be_different)}
    assert np.array_equal(failed, sc.broken & ~sc.failing) and np.array_equal(other, sc.failing)
    assert int(sc.broken.sum()) == 32 * CHAIN and replies == sc.expected_replies()
    # The dependent events are the chains, whole, and nothing else.
    assert dependent_count(sc.bodies, sc.accounts, sc.existing_ids) == PREPARES * CHAIN
    # The independent ok events past what 256 workgroups of 1024 threads take.
    ok = ~failed & ~other
    late = ok & ~sc.chain & (np.arange(EVENTS) >= LATE_FROM)
    assert int(late.sum()) > 200_000
    transfers = oracle.export_transfers()
    mine = transfers[transfers["timestamp"] >= sc.first_ts]
    mine = mine[np.argsort(mine["timestamp"])]  # the pass's committed records, in event order
    assert np.array_equal(mine["id_lo"], sc.events["id_lo"][ok])
    by_event = np.zeros(EVENTS, dtype=transfers.dtype)
    by_event[ok] = mine
    for account in sc.account_ids:
        lo = account & ((1 << 64) - 1)
        names = (by_event["debit_account_id_lo"] == lo) | (by_event["credit_account_id_lo"] == lo)
        named = (sc.events["debit_account_id_lo"] == lo) | (sc.events["credit_account_id_lo"] == lo)
        assert (named & sc.chain).any() and (names & late).any(), hex(account)
    accounts = oracle.export_accounts()
    assert len(accounts) == N_ACCOUNTS
    if variant == "postvoid":
        assert int(sc.postvoid.sum()) == PENDINGS and int((sc.postvoid & late).sum()) > 50_000
        assert len(oracle.export_posted()) == PENDINGS + PREPARES // 2  # every pending settled once; 32 chains committed
    if variant == "wide":
        # Some balance needs the high word, and every balance is the exact sum of its legs (no wrap).
        wide = mine[mine["amount_hi"] != 0]
        assert len(wide) == int((ok & ~sc.chain).sum())
        for a in accounts:
            got = [u128(a, c) for c in COLUMNS]
            for side, column in (("debit_account_id_lo", 1), ("credit_account_id_lo", 3)):
                legs = wide[wide[side] == a["id_lo"]]
                total = (int(legs["amount_hi"].astype(object).sum()) << 64) + int(legs["amount_lo"].astype(object).sum())
                # the wide legs, exactly, plus the chains' small amounts
                assert total >= 1 << 64 and 0 <= got[column] - total < 1 << 40, (hex(u128(a, "id")), column)
    oracle.close()
