"""The checkers of tests/harness/balances.py against the oracle and against each other, before any
GPU answer is held to them.  No GPU."""
import numpy as np

from tests.harness.balances import balances_of, oracle_rows, replay_rows, spec_rows, u128
from tests.harness.oracle import OracleEngine
from tests.harness.workload import make_scenario
from tigerbeetle_amd.types import TransferFlags

QUERY_SCENARIO = dict(n_accounts=64, n_transfer_batches=24, batch_len=(100, 400), p_pending=0.3, p_post_void=0.25,
                      p_dup=0.05, p_linked=0.05, p_limit=0.05, p_balancing=0.02, p_invalid=0.05)  # test_gpu_query.py's
CHAIN_FREE = dict(n_accounts=16, n_transfer_batches=6, batch_len=(100, 300), p_linked=0, p_limit=0.1, p_balancing=0.05)


def committed(sc):
    oracle = OracleEngine(4096, 1 << 15)
    for _, op, ts, events in sc.steps:
        oracle.commit(op, ts, b"".join(events))
    return oracle.export_transfers(), oracle.export_accounts()


def test_replay_reproduces_the_oracles_final_balances():
    transfers, accounts = committed(make_scenario(2025, **QUERY_SCENARIO))
    rows = replay_rows(transfers)
    final = {u128(a, "id"): balances_of(a) for a in accounts}
    touched = 0
    for account, want in final.items():
        if account in rows:
            assert rows[account][-1][2] == want, hex(account)
            touched += 1
        else:
            assert want == (0, 0, 0, 0)
    post = int(TransferFlags.post_pending_transfer)
    pending = {u128(t, "id"): u128(t, "amount") for t in transfers if t["flags"] & int(TransferFlags.pending)}
    partial = sum(1 for t in transfers if t["flags"] & post and u128(t, "amount") < pending[u128(t, "pending_id")])
    assert touched > 32 and len(transfers) > 1500 and partial > 0
    # The backward definition over the whole ledger is the same history.
    spec, orphans = spec_rows(transfers, accounts)
    assert spec == rows and not orphans


def test_replay_equals_the_oracle_row_by_row():
    sc = make_scenario(7, **CHAIN_FREE)
    transfers, _ = committed(sc)
    want = oracle_rows(sc.steps)
    got = replay_rows(transfers)
    assert got == want
    assert sum(len(r) for r in want.values()) == 2 * len(transfers) and len(transfers) > 100
    assert np.all(np.diff(np.sort(transfers["timestamp"])) > 0)
