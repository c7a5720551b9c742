"""The checker of tests/harness/matrix.py against get_account_statements' checker and the rules the
header states, before any GPU answer is held to it; and net_positions.  No GPU."""
import numpy as np
import pytest

from tests.harness.balances import PENDING, POST, u128
from tests.harness.matrix import CELLS_MAX, FlowMatrix, cell_sums, pair_of, valid_period
from tests.harness.oracle import OracleEngine
from tests.harness.statements import Statements, request_of, sums, sweep_pairs
from tests.harness.workload import account_id, make_scenario
from tests.test_balance_checkers import QUERY_SCENARIO
from tigerbeetle_amd.state_machine import net_positions
from tigerbeetle_amd.types import FLOW_CELL_DTYPE, U64_MAX

ABSENT = (account_id(5000), account_id(5001))
MOD = 1 << 128


@pytest.fixture(scope="module")
def ledger():
    sc = make_scenario(2025, **QUERY_SCENARIO)
    oracle = OracleEngine(4096, 1 << 15)
    for _, op, ts, events in sc.steps:
        oracle.commit(op, ts, b"".join(events))
    transfers, accounts = oracle.export_transfers(), oracle.export_accounts()
    commit_timestamp = oracle.commit_timestamp
    oracle.close()
    return dict(matrix=FlowMatrix(transfers, accounts), single=Statements(transfers, accounts), transfers=transfers,
                everyone=[u128(a, "id") for a in accounts], request=request_of(accounts, ABSENT),
                sweep=sweep_pairs(sc.steps, transfers, commit_timestamp))


def widest(sweep):
    """The longest period of the sweep with both ends given."""
    return max((p for p in sweep if p[0] and p[1]), key=lambda p: p[1] - p[0])


def halves(ids):
    """The list in pieces that, against the whole list, stay within the call's 4,095 cells."""
    step = CELLS_MAX // len(ids)
    return [ids[k:k + step] for k in range(0, len(ids), step)]


def added(cells):
    return tuple(sum(cell_sums(c)[q] for c in cells) % MOD if q < 3 else sum(cell_sums(c)[q] for c in cells) for q in range(4))


def test_row_and_column_sums_are_the_statements(ledger):
    """Every account against every account (62 x 62 cells; `halves` would cut a longer list to the
    call's limit): a debit row adds up to the account's debits_* of the statement, a credit column to
    its credits_*."""
    matrix, single, everyone = ledger["matrix"], ledger["single"], ledger["everyone"]
    assert len(everyone) > 60
    busy = 0
    for t_open, t_close in ledger["sweep"]:
        statements = {u128(r, "id"): sums(r) for r in single.of(everyone, t_open, t_close)[0]}
        for piece in halves(everyone):
            cells, matched, orphan = matrix.of(piece, everyone, t_open, t_close)
            live = [i for i in piece if i in statements]
            assert matched == len(cells) == len(live) * len(statements) and not orphan
            for r, account in enumerate(live):
                row = cells[r * len(statements):(r + 1) * len(statements)]
                assert all(pair_of(c)[0] == account for c in row)
                p_in, p_out, posted, n = statements[account][0]
                assert added(row) == (posted, p_in, p_out, n)
                busy += n > 0
            cells, matched, _ = matrix.of(everyone, piece, t_open, t_close)
            assert matched == len(cells) == len(statements) * len(live)
            for q, account in enumerate(live):
                column = cells[q::len(live)]
                assert all(pair_of(c)[1] == account for c in column)
                p_in, p_out, posted, n = statements[account][1]
                assert added(column) == (posted, p_in, p_out, n)
    assert busy > 100


def test_direction_repeats_absent_and_reserved_ids(ledger):
    matrix, everyone, transfers = ledger["matrix"], ledger["everyone"], ledger["transfers"]
    pairs = {(u128(t, "debit_account_id"), u128(t, "credit_account_id")) for t in transfers}
    d, c = next((d, c) for d, c in sorted(pairs) if (c, d) not in pairs)  # somebody paid and was never paid back
    cells, matched, _ = matrix.of([d, c], [d, c], 0, 0)
    assert matched == 4 and [pair_of(x) for x in cells] == [(d, d), (d, c), (c, d), (c, c)]
    assert cell_sums(cells[1])[3] > 0 and cell_sums(cells[2]) == cell_sums(cells[0]) == cell_sums(cells[3]) == (0, 0, 0, 0)
    assert matrix.of([c], [d], 0, 0)[0][0]["transfers"] == 0 and matrix.of([d], [c], 0, 0)[0].tobytes() == cells[1].tobytes()
    # Absent and reserved ids are skipped, a repeated id is answered once per occurrence, on either list.
    debit = [ABSENT[0], d, 0, d, (1 << 128) - 1]
    credit = [c, ABSENT[1], c, d, c]
    cells, matched, _ = matrix.of(debit, credit, 0, 0)
    assert matched == 2 * 4 and [pair_of(x) for x in cells] == [(d, c), (d, c), (d, d), (d, c)] * 2
    assert cells[0].tobytes() == cells[1].tobytes() == cells[3].tobytes() == cells[4].tobytes() != cells[2].tobytes()
    assert matrix.of([ABSENT[0], 0], everyone, 0, 0)[1] == 0 and matrix.of(everyone[:3], [ABSENT[1]], 0, 0)[1] == 0
    # An account younger than t_close is not found, on either list.
    created = matrix.created
    young, old = max(created, key=created.get), min(created, key=created.get)
    assert matrix.of([young, old], [old], 0, created[young] - 1)[1] == 1 and matrix.of([old], [old, young], 0, created[young])[1] == 2
    assert matrix.of([old], [young, young], 0, created[young] - 1)[1] == 0


def test_cap_cuts_inside_a_row(ledger):
    matrix, request = ledger["matrix"], ledger["request"]
    debit, credit = request[:9], request[5:40]
    t_open, t_close = widest(ledger["sweep"])
    cells, matched, _ = matrix.of(debit, credit, t_open, t_close)
    width = matched // 9
    assert matched == len(cells) == 9 * width and width > 20 and cells["transfers"].sum() > 0
    for cap in (0, 1, width - 1, width + 3, matched, matched + 3):
        cut, m, _ = matrix.of(debit, credit, t_open, t_close, cap)
        assert m == matched and cut.tobytes() == cells[:cap].tobytes()


def test_the_orphan_rule_is_narrower_than_the_statements(ledger):
    """A post whose pending transfer is left out of the export drops the verdict only where both of
    its sides are asked for, each on its own list, and it lies in the period."""
    transfers, accounts_of = ledger["transfers"], ledger["everyone"]
    post = next(t for t in transfers if int(t["flags"]) & POST and not int(t["flags"]) & PENDING)
    keep = np.array([u128(t, "id") != u128(post, "pending_id") for t in transfers])
    assert keep.sum() == len(transfers) - 1
    accounts = np.zeros(0, dtype=[("id_lo", "<u8"), ("id_hi", "<u8"), ("timestamp", "<u8")])
    accounts = np.array([(i & U64_MAX, i >> 64, 1) for i in accounts_of], dtype=accounts.dtype)
    matrix = FlowMatrix(transfers[keep], accounts)
    d, c, ts = u128(post, "debit_account_id"), u128(post, "credit_account_id"), int(post["timestamp"])
    other = next(i for i in accounts_of if i not in (d, c))
    verdict = lambda debit, credit, t_open, t_close: matrix.of(debit, credit, t_open, t_close)[2]
    assert verdict([d], [c], 0, 0) and verdict([other, d], [c, other], ts - 1, ts) and verdict([d], [c], ts - 1, ts, ) is True
    assert not verdict([c], [d], 0, 0)          # the other direction
    assert not verdict([d], [other], 0, 0)      # one side asked
    assert not verdict([other], [c], 0, 0)
    assert not verdict([d], [c], ts, 0)         # outside the period
    assert not verdict([d], [c], 0, ts - 1)
    cells, _, orphan = matrix.of([d, other], [c], 0, 0, cap=0)  # under the cap or not
    assert orphan and len(cells) == 0
    cell = matrix.of([d], [c], ts - 1, ts)[0][0]
    assert cell_sums(cell) == (u128(post, "amount"), 0, u128(post, "amount"), 1)  # P = its own amount


def test_invalid_periods_and_empty_lists(ledger):
    matrix, everyone = ledger["matrix"], ledger["everyone"]
    t = widest(ledger["sweep"])
    for t_open, t_close in ((U64_MAX, 0), (0, U64_MAX), (t[1], t[0]), (U64_MAX, U64_MAX)):
        assert not valid_period(t_open, t_close)
        cells, matched, orphan = matrix.of(everyone[:5], everyone[:5], t_open, t_close)
        assert len(cells) == 0 and cells.dtype == FLOW_CELL_DTYPE and (matched, orphan) == (0, False)
    assert matrix.of([], everyone, 0, 0)[1] == 0 and matrix.of(everyone, [], 0, 0)[1] == 0
    assert matrix.of(everyone[:5], everyone[:5], t[1], t[1])[1] == 25  # an empty period is a valid one


def test_net_positions_sum_to_zero_over_one_list(ledger):
    matrix, everyone = ledger["matrix"], ledger["everyone"]
    cells = np.concatenate([matrix.of(piece, everyone, 0, 0)[0] for piece in halves(everyone)])
    net = net_positions(cells)
    assert set(net) == set(everyone) and all(type(v) is int for v in net.values())
    assert sum(net.values()) == 0 and any(v < 0 for v in net.values()) and any(v > 0 for v in net.values())
    received = {i: sum(u128(c, "posted") for c in cells if pair_of(c)[1] == i) for i in everyone}
    paid = {i: sum(u128(c, "posted") for c in cells if pair_of(c)[0] == i) for i in everyone}
    assert net == {i: received[i] - paid[i] for i in everyone}
    # A rectangular request names accounts on one side only; a cell (d, d) changes nothing.
    one = np.zeros(2, dtype=FLOW_CELL_DTYPE)
    one["debit_id_lo"], one["credit_id_lo"], one["posted_lo"], one["posted_hi"] = [7, 9], [9, 9], [5, 100], [1, 0]
    assert net_positions(one) == {7: -((1 << 64) + 5), 9: (1 << 64) + 5}
    assert net_positions(one[:0]) == {}
