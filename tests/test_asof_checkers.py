"""The checker of tests/harness/asof.py against the oracle and against the forward replay, before any
GPU answer is held to it.  No GPU."""

from tests.harness.asof import AsOf, ids_body
from tests.harness.balances import PENDING, POST, VOID, balances_of, replay_rows, u128
from tests.harness.oracle import OracleEngine
from tests.harness.workload import account_id, make_scenario
from tests.test_balance_checkers import CHAIN_FREE, QUERY_SCENARIO, committed
from tigerbeetle_amd.types import ACCOUNT_DTYPE


def request_of(accounts):
    """Every account, absent ids, the reserved ids and repeats."""
    ids = [u128(a, "id") for a in accounts]
    return ids[::-1] + [account_id(5000), 0, (1 << 128) - 1] + ids[:5] + [account_id(5001)] + ids[3:4]


def check_scenario(seed, shape):
    """Holds the checker to the oracle and to the replay on one scenario; returns what the sweep met:
    (T inside a prepare, accounts skipped as created after T, T between a pending transfer and its
    partial post, T between a pending transfer and its void)."""
    sc = make_scenario(seed, **shape)
    transfers, accounts = committed(sc)
    checker = AsOf(transfers, accounts)
    ids = request_of(accounts)
    body = ids_body(ids)

    # At every prepare boundary: lookup_accounts on a fresh oracle that committed only that prefix.
    skipped_as_younger = 0
    for k, (_, _, boundary, _) in enumerate(sc.steps):
        oracle = OracleEngine(4096, 1 << 15)
        for _, op, ts, events in sc.steps[:k + 1]:
            oracle.commit(op, ts, b"".join(events))
        want = oracle.commit(130, boundary + 1, body)
        oracle.close()
        got, matched, orphan = checker.at(ids, boundary)
        assert got.tobytes() == want, (k, boundary)
        assert matched == len(got) and not orphan
        skipped_as_younger += sum(1 for a in accounts if int(a["timestamp"]) > boundary)

    # At every transfer's timestamp: the newest row of the forward replay at or before it.
    rows = replay_rows(transfers)
    boundaries = {ts for _, _, ts, _ in sc.steps}
    stamps = sorted(int(t) for t in transfers["timestamp"])
    inside = sum(1 for t in stamps if t not in boundaries)
    at = {a: 0 for a in rows}  # rows of the account at or before T, advanced with T
    for T in stamps:
        got, matched, orphan = checker.at(ids, T)
        assert matched == len(got) == len(ids) - 4 and not orphan  # the accounts all exist by now
        for rec in got:
            a = u128(rec, "id")
            want = (0, 0, 0, 0)
            if a in rows:
                while at[a] < len(rows[a]) and rows[a][at[a]][0] <= T:
                    at[a] += 1
                if at[a]:
                    want = rows[a][at[a] - 1][2]
            assert balances_of(rec) == want, (T, hex(a))

    # A pending transfer's own timestamp is a tested T between it and its post or void.
    pending = {u128(t, "id"): t for t in transfers if int(t["flags"]) & PENDING}
    partial = voided = 0
    for t in transfers:
        flags = int(t["flags"])
        if flags & PENDING or not flags & (POST | VOID):
            continue
        p = pending[u128(t, "pending_id")]
        assert int(p["timestamp"]) in stamps and int(p["timestamp"]) < int(t["timestamp"])
        if flags & POST and u128(t, "amount") < u128(p, "amount"):
            partial += 1
        if flags & VOID:
            voided += 1
    return inside, skipped_as_younger, partial, voided


def test_checker_equals_the_oracle_and_the_replay():
    met = [check_scenario(7, CHAIN_FREE), check_scenario(2025, QUERY_SCENARIO)]
    # Not vacuous: at least one T inside a prepare, one account skipped as created after T, one T between
    # a pending transfer and its partial post, one between a pending transfer and its void.
    inside, skipped, partial, voided = (sum(m[i] for m in met) for i in range(4))
    assert inside > 0 and skipped > 0 and partial > 0 and voided > 0
    assert all(m[0] > 0 and m[1] > 0 for m in met)


def test_now_the_limit_and_the_invalid_timestamp():
    transfers, accounts = committed(make_scenario(7, **CHAIN_FREE))
    checker = AsOf(transfers, accounts)
    ids = request_of(accounts)
    now, matched, _ = checker.at(ids, 0)
    final = {u128(a, "id"): a for a in accounts}
    assert matched == len(ids) - 4 and [r.tobytes() for r in now] == [final[i].tobytes() for i in ids if i in final]
    newest = int(transfers["timestamp"].max())
    assert checker.at(ids, newest)[0].tobytes() == now.tobytes()
    assert checker.at(ids, newest - 1)[0].tobytes() != now.tobytes()
    cut, matched, _ = checker.at(ids, 0, out_cap_records=3)
    assert matched == len(ids) - 4 and cut.tobytes() == now[:3].tobytes()
    assert checker.at(ids, (1 << 64) - 1)[1] == 0 and checker.at([], 5)[1] == 0
    before, matched, _ = checker.at(ids, 1)
    assert matched == 0 and len(before) == 0 and before.dtype == ACCOUNT_DTYPE
    # An orphan post: its pending transfer is not among the resident records.
    posts = [t for t in transfers if int(t["flags"]) & POST and not int(t["flags"]) & PENDING]
    assert posts
    keep = transfers[[u128(t, "id") != u128(posts[-1], "pending_id") for t in transfers]]
    orphaned = AsOf(keep, accounts)
    assert orphaned.at(ids, int(posts[-1]["timestamp"]) - 1)[2] and not orphaned.at(ids, int(posts[-1]["timestamp"]))[2]
