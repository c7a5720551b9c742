"""The checkers of tests/harness/change_events.py against the oracle and against each other, before
any GPU answer is held to them.  No GPU."""
import numpy as np

from tests.harness.balances import balances_of, u128
from tests.harness.change_events import oracle_events, select, spec_events
from tests.test_balance_checkers import CHAIN_FREE, QUERY_SCENARIO, committed
from tests.harness.workload import make_scenario
from tigerbeetle_amd.types import CHANGE_EVENT_DTYPE, TransferFlags

POST = int(TransferFlags.post_pending_transfer)
PENDING = int(TransferFlags.pending)


def test_spec_equals_the_oracle_event_by_event():
    sc = make_scenario(7, **CHAIN_FREE)
    transfers, accounts = committed(sc)
    want = oracle_events(sc.steps)
    got, incomplete = spec_events(transfers, accounts)
    assert len(transfers) == 323 and len(want) == len(transfers)
    assert not incomplete.any()
    for i in range(len(want)):
        assert got[i].tobytes() == want[i].tobytes(), i
    assert np.all(np.diff(want["transfer"]["timestamp"].astype(np.int64)) > 0)
    # Non-vacuity: balances move, and both blocks carry the account's own fields.
    assert want["debit_account"]["debits_posted_lo"].max() > 0 and want["credit_account"]["credits_posted_lo"].max() > 0
    assert np.array_equal(want["debit_account"]["id_lo"], want["transfer"]["debit_account_id_lo"])
    assert np.array_equal(want["credit_account"]["id_lo"], want["transfer"]["credit_account_id_lo"])
    assert want["debit_account"]["timestamp"].min() > 0 and want["debit_account"]["ledger"].min() > 0


def test_spec_newest_event_per_account_is_the_final_balance():
    transfers, accounts = committed(make_scenario(2025, **QUERY_SCENARIO))
    events, incomplete = spec_events(transfers, accounts)
    assert len(transfers) == 1944 and len(accounts) == 62 and not incomplete.any()
    final = {u128(a, "id"): a for a in accounts}
    seen = set()
    for ev in events[::-1]:
        for block in ("debit_account", "credit_account"):
            account = u128(ev[block], "id")
            if account not in seen:
                seen.add(account)
                assert ev[block].tobytes() == final[account].tobytes(), hex(account)
    assert len(seen) > 32
    # The oldest event of an account starts from zero plus its own effect: the backward walk closes.
    first = {}
    for ev in events:
        for block, at in (("debit_account", 0), ("credit_account", 2)):
            first.setdefault(u128(ev[block], "id"), (ev, block, at))
    for account, (ev, block, at) in first.items():
        b = list(balances_of(ev[block]))
        t = ev["transfer"]
        amount, flags = u128(t, "amount"), int(t["flags"])
        assert not flags & POST or flags & PENDING  # an account's first record is never a post
        want = [0, 0, 0, 0]
        want[at + (0 if flags & PENDING else 1)] = amount
        assert b == want, hex(account)
    pending = {u128(t, "id"): u128(t, "amount") for t in transfers if t["flags"] & PENDING}
    assert sum(1 for t in transfers if t["flags"] & POST and u128(t, "amount") < pending[u128(t, "pending_id")]) > 0


def test_select_cuts_as_the_filter_does():
    events = np.zeros(10, dtype=CHANGE_EVENT_DTYPE)
    events["transfer"]["timestamp"] = np.arange(100, 110)
    got, matched = select(events, timestamp_min=103, timestamp_max=107, limit=3)
    assert matched == 5 and got["transfer"]["timestamp"].tolist() == [103, 104, 105]
    got, matched = select(events, limit=8, out_cap_events=2)
    assert matched == 10 and len(got) == 2
    got, matched = select(events, timestamp_min=110)
    assert matched == 0 and len(got) == 0
