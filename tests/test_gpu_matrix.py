"""get_account_flow_matrix (include/tbgpu.h tbgpu_get_account_flow_matrix, csrc/k_matrix.h): for a list
of debit accounts, a list of credit accounts and a period, one cell per pair from one scan of the HBM
log.  Cells, `matched` and `complete` are compared byte for byte with the checker of
tests/harness/matrix.py (itself held to get_account_statements' checker in
tests/test_matrix_checkers.py) and with the engine's own get_account_statements rows."""
import ctypes
import random

import numpy as np
import pytest

from tests.harness.balances import u128
from tests.harness.matrix import FlowMatrix, cell_sums, pair_of
from tests.harness.oracle import OracleEngine
from tests.harness.shard_double import homes_of
from tests.harness.statements import ids_body, request_of, sums, sweep_pairs
from tests.harness.workload import account_id, make_scenario
from tests.test_gpu_query import SCENARIO, by_id, commit_all, posted_states
from tigerbeetle_amd import _lib
from tigerbeetle_amd._lib import EnginePanic
from tigerbeetle_amd.state_machine import net_positions
from tigerbeetle_amd.types import FLOW_CELL_DTYPE, U64_MAX, TransferFlags, pack_account, pack_transfer

pytestmark = pytest.mark.gpu

PENDING = int(TransferFlags.pending)
POST = int(TransferFlags.post_pending_transfer)
VOID = int(TransferFlags.void_pending_transfer)
MAX = 4095
CELL = 96
MOD = 1 << 128
ABSENT = (account_id(5000), account_id(5001))


def thinned(ids):
    """request_of's list cut to fit a square request (72 x 72 is over 4,095 cells): every other id, and
    its tail of absent ids, reserved ids and repeats."""
    return ids[:-10:2] + ids[-10:]


def check(engine, checker, debit, credit, t_open, t_close, evicted=False, cap=None):
    """One request: cells, matched and complete as the checker has them."""
    want, matched, orphan = checker.of(debit, credit, t_open, t_close, cap)
    got, got_matched, got_complete = engine.get_account_flow_matrix(debit, credit, t_open, t_close, cap)
    assert len(got) == len(want), (t_open, t_close, len(got), len(want))
    if got.tobytes() != want.tobytes():
        bad = [n for n in range(len(got)) if got[n].tobytes() != want[n].tobytes()]
        raise AssertionError("cells differ: %d of %d, the first %s, period (%d, %d]" % (len(bad), len(got), bad[:8], t_open, t_close))
    assert (got_matched, got_complete) == (matched, not evicted and not orphan), (t_open, t_close)
    return got


def added(cells):
    return tuple(sum(cell_sums(c)[q] for c in cells) % MOD if q < 3 else sum(cell_sums(c)[q] for c in cells) for q in range(4))


def check_statements(engine, everyone, t_open, t_close):
    """With both lists every account, the engine's own row and column sums are its own statements."""
    cells, matched, _ = engine.get_account_flow_matrix(everyone, everyone, t_open, t_close)
    rows = engine.get_account_statements(everyone, t_open, t_close)[0]
    n = len(rows)
    assert matched == len(cells) == n * n
    for k, row in enumerate(rows):
        (d_in, d_out, d_posted, d_n), (c_in, c_out, c_posted, c_n) = sums(row)
        assert added(cells[k * n:(k + 1) * n]) == (d_posted, d_in, d_out, d_n), (t_open, t_close, k)
        assert added(cells[k::n]) == (c_posted, c_in, c_out, c_n), (t_open, t_close, k)
    return cells


def raw_call(engine, t_open, t_close, debit, n_debit, credit, n_credit, cap, fill=b"\xAB"):
    """The C call into a sentinel-filled buffer: (status, result, the buffer's bytes)."""
    cells = max(len(debit) * len(credit), 1)
    d_src = ctypes.create_string_buffer(ids_body(debit), 16 * len(debit))
    c_src = ctypes.create_string_buffer(ids_body(credit), 16 * len(credit))
    out = ctypes.create_string_buffer(fill * (CELL * cells), CELL * cells)
    res = _lib.tbgpu_query_result(count=77, complete=77, matched=77)
    status = engine.lib.tbgpu_get_account_flow_matrix(engine.h, t_open, t_close, d_src, n_debit, c_src, n_credit, out, cap, ctypes.byref(res))
    return status, (res.count, res.complete, res.matched), out.raw


@pytest.fixture(scope="module")
def ledger():
    """test_gpu_query.py's scenario, the oracle that committed all of it, its exports and the checker
    over them (never changed)."""
    sc = make_scenario(2025, **SCENARIO)
    oracle = OracleEngine(4096, 1 << 15)
    replies = commit_all(sc, oracle)
    transfers, accounts = oracle.export_transfers(), oracle.export_accounts()
    ids = request_of(accounts, ABSENT)
    return dict(sc=sc, replies=replies, transfers=transfers, accounts=accounts, commit_timestamp=oracle.commit_timestamp,
                posted=oracle.export_posted(), checker=FlowMatrix(transfers, accounts), ids=ids, same=thinned(ids),
                everyone=[u128(a, "id") for a in accounts], sweep=sweep_pairs(sc.steps, transfers, oracle.commit_timestamp))


def requests_of(ledger):
    """(debit list, credit list): both the same, a rectangle that shares ids, two disjoint lists."""
    ids, same, everyone = ledger["ids"], ledger["same"], ledger["everyone"]
    assert len(same) ** 2 <= MAX and len(ids) ** 2 > MAX
    return [(same, same), (ids[:20], ids[15:]), (everyone[:30], everyone[30:])]


def test_single_engine_sweep(ledger, gpu_engine_factory):
    sc, checker, everyone = ledger["sc"], ledger["checker"], ledger["everyone"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    assert commit_all(sc, engine) == ledger["replies"]
    assert engine.commit_timestamp == ledger["commit_timestamp"]
    busy = 0
    for n, (t_open, t_close) in enumerate(ledger["sweep"]):
        for debit, credit in requests_of(ledger):
            got = check(engine, checker, debit, credit, t_open, t_close)
            busy += int((got["transfers"] > 0).sum())
        if n % 3 == 0:
            cells = check_statements(engine, everyone, t_open, t_close)
            assert sum(net_positions(cells).values()) == 0
    assert busy > 1000
    # out_cap_cells cuts the answer in cell order, inside a debit row too, and nothing past count cells is written.
    debit, credit = ledger["ids"][:9], ledger["ids"][5:40]
    t_open, t_close = max((p for p in ledger["sweep"] if p[0] and p[1]), key=lambda p: p[1] - p[0])
    whole = check(engine, checker, debit, credit, t_open, t_close)
    matched, width = len(whole), len(whole) // 9
    assert matched == 9 * width and width > 20 and whole["transfers"].sum() > 0
    for cap in (0, 1, width - 1, matched, matched + 3):
        check(engine, checker, debit, credit, t_open, t_close, cap=cap)
        status, (count, complete, m), raw = raw_call(engine, t_open, t_close, debit, len(debit), credit, len(credit), cap)
        assert status == _lib.STATUS_OK and (count, complete, m) == (min(cap, matched), 1, matched)
        assert raw[:CELL * count] == whole[:count].tobytes() and raw[CELL * count:] == b"\xAB" * (len(raw) - CELL * count)


def test_tile_wave_and_workgroup_edges(gpu_engine_factory):
    """tests/test_gpu_series.py's construction: two prepares of 4,200 events committed in place, so log
    position = event index and timestamp = first + position.  Records of the one pair A -> B sit around
    the scan's wave edge (63/64), tile edge (511/512) and workgroup edge (8191/8192); every lane of the
    wave at 1024-1087 holds A -> B and B -> A in turn, two chains interleaved in one wave; A -> X and
    X -> A, X not asked for, enter nothing; a pending transfer with its partial post, another with its
    void, two failing events that name the pair, and amounts whose sums carry across the 64-bit word.
    Periods open and close at, one below and one above every planted position, and inside the wave."""
    engine = gpu_engine_factory(transfers_max=1 << 14)
    oracle = OracleEngine(64, 1 << 14)
    n_acc, A, B, half = 8, account_id(0), account_id(1), 4200
    accounts = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(n_acc))
    assert engine.commit(128, 10**12, accounts) == oracle.commit(128, 10**12, accounts) == b""
    rng = random.Random(11)
    amounts = [(1 << 64) - 1, 1 << 64, 1 << 100, 1, (1 << 64) - 7]
    edges = [62, 63, 64, 65, 255, 256, 510, 511, 512, 513, 4199, 4200, 8190, 8191, 8192, 8193]
    wave = range(1024, 1088)
    batch = []
    for i in range(2 * half):
        dr = 2 + rng.randrange(n_acc - 2)
        cr = 2 + (dr - 2 + 1 + rng.randrange(n_acc - 3)) % (n_acc - 2)  # another account, never A or B
        ev = dict(id=1000 + i, debit_account_id=account_id(dr), credit_account_id=account_id(cr), amount=1 + i, ledger=1, code=1)
        if i in edges:
            ev.update(debit_account_id=A, credit_account_id=B, amount=amounts[i % len(amounts)], flags=PENDING if i % 7 == 3 else 0)
        elif i in wave:
            ev.update(amount=amounts[i % len(amounts)], flags=PENDING if i % 7 == 3 else 0)
            ev.update(debit_account_id=A, credit_account_id=B) if i % 2 == 0 else ev.update(debit_account_id=B, credit_account_id=A)
        elif i == 10:
            ev.update(debit_account_id=A, credit_account_id=B, amount=1 << 100, flags=PENDING)
        elif i == 514:
            ev.update(debit_account_id=0, credit_account_id=0, amount=(1 << 64) - 1, pending_id=1010, flags=POST)
        elif i == 61:
            ev.update(debit_account_id=B, credit_account_id=A, amount=1 << 64, flags=PENDING)
        elif i == 8189:
            ev.update(debit_account_id=0, credit_account_id=0, amount=0, pending_id=1061, flags=VOID)
        elif i == 66:
            ev.update(debit_account_id=A, credit_account_id=B, id=0)
        elif i == 8194:
            ev.update(debit_account_id=A, credit_account_id=B, id=1000 + 64)
        elif i % 50 == 7:
            ev.update(debit_account_id=A)  # A -> X
        elif i % 50 == 9:
            ev.update(credit_account_id=A)  # X -> A
        elif i % 50 == 11:
            ev.update(debit_account_id=B)  # B -> X
        batch.append(pack_transfer(**ev))
    bodies = [b"".join(batch[:half]), b"".join(batch[half:])]
    stamps = [10**12 + 10**6, 10**12 + 10**6 + half]
    expected = b"".join(oracle.commit(129, ts, body) for ts, body in zip(stamps, bodies))
    failed = np.frombuffer(expected, dtype=np.uint32)[0::2].tolist()
    assert failed == [66, 8194 - half]  # exactly the planted events failed
    exported = oracle.export_transfers()
    first = stamps[0] - half + 1
    at = lambda pos: first + pos
    assert len(exported) == 2 * half - 2 and int(exported["timestamp"].max()) == at(2 * half - 1)
    checker = FlowMatrix(exported, oracle.export_accounts())
    window = engine.log_window(2 * half)
    engine.to_device(window, np.frombuffer(bodies[0] + bodies[1], dtype=np.uint8))
    res, rb = engine.alloc(2 * half * 8), engine.alloc(8)
    engine.commit_device_async(129, stamps, [half, half], window, res, rb)
    # The query drains the pending call itself.
    pair = [A, B]
    whole = check(engine, checker, pair, pair, 0, 0)
    assert [pair_of(c) for c in whole] == [(A, A), (A, B), (B, A), (B, B)]
    assert int(whole[0]["transfers"]) == int(whole[3]["transfers"]) == 0
    assert int(whole[1]["transfers"]) == len(edges) + 32 + 2 and int(whole[2]["transfers"]) == 32 + 2  # + the pending and its post / void
    assert u128(whole[1], "posted") >> 64 and u128(whole[2], "posted") >> 64  # the sums carried
    marks = sorted({e + d for e in edges + [1024, 1087] for d in (-1, 0, 1)} | {9, 10, 61, 514, 8189, 8399})
    seen = set()
    for k, m in enumerate(marks):
        for t_open, t_close in ((at(m), 0), (0, at(m)), (at(m), at(marks[k + 1]) if k + 1 < len(marks) else at(m))):
            got = check(engine, checker, pair, pair, t_open, t_close)
            seen.add(got.tobytes())
    assert len(seen) > 40  # the cells move with the period: 21 planted positions, from either end
    everybody = [account_id(i) for i in range(n_acc)]
    check(engine, checker, everybody + [A], [B, account_id(5)] + everybody, at(63), at(8191))
    # Inside the full wave: the records of 1031..1050 and of 1036..1040, A -> B on the even positions.
    got = check(engine, checker, pair, pair, at(1030), at(1050))
    assert [int(c["transfers"]) for c in got] == [0, 10, 10, 0]
    got = check(engine, checker, pair, pair, at(1035), at(1040))
    assert [int(c["transfers"]) for c in got] == [0, 3, 2, 0]
    got = check(engine, checker, [B], [A], at(1023), at(1087))
    assert [int(c["transfers"]) for c in got] == [32]
    # The partial post and the void, alone in their periods.
    got = check(engine, checker, pair, pair, at(513), at(514))
    assert cell_sums(got[1]) == ((1 << 64) - 1, 0, 1 << 100, 1) and cell_sums(got[2]) == (0, 0, 0, 0)
    got = check(engine, checker, pair, pair, at(8188), at(8189))
    assert cell_sums(got[2]) == (0, 0, 1 << 64, 1) and cell_sums(got[1]) == (0, 0, 0, 0)
    assert engine.export_accounts().tobytes() == oracle.export_accounts().tobytes()
    assert engine.export_transfers().tobytes() == exported.tobytes()
    engine.free(res)
    engine.free(rb)


def test_more_keys_than_lds_bins(gpu_engine_factory):
    """63 debit and 65 credit accounts and one 4,095-transfer prepare with one record per pair: 4,095
    distinct keys inside one workgroup's 8,192 records, far more than its claimed LDS bins — bins are
    claimed, handed over at the workgroup's end and, once both of a key's slots are taken, bypassed for
    HBM."""
    n_debit, n_credit = 63, 65
    engine = gpu_engine_factory(transfers_max=1 << 13)
    body = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(n_debit + n_credit))
    assert engine.commit(128, 10**12, body) == b""
    order = list(range(MAX))
    random.Random(5).shuffle(order)
    body = b"".join(pack_transfer(id=10**6 + j, debit_account_id=account_id(j // n_credit),
                                  credit_account_id=account_id(n_debit + j % n_credit), amount=(1 << 63) + j, ledger=1, code=1,
                                  flags=PENDING if j % 3 == 0 else 0) for j in order)
    assert engine.commit(129, 2 * 10**12, body) == b""
    transfers = engine.export_transfers()
    assert len(transfers) == MAX
    checker = FlowMatrix(transfers, engine.export_accounts())
    debit = [account_id(i) for i in range(n_debit - 1, -1, -1)]
    credit = [account_id(n_debit + i) for i in range(n_credit)]
    got = check(engine, checker, debit, credit, 0, 0)
    assert len(got) == MAX and (got["transfers"] == 1).all()
    # The same with the first and the last 1,000 records outside the period, and the lists swapped: nothing.
    stamps = np.sort(transfers["timestamp"])
    got = check(engine, checker, debit, credit, int(stamps[999]), int(stamps[-1001]))
    assert int(got["transfers"].sum()) == MAX - 2000
    assert int(check(engine, checker, credit, debit, 0, 0)["transfers"].sum()) == 0


@pytest.fixture(scope="module")
def wide():
    """4,200 accounts and two 4,000-transfer prepares in which 600 accounts debit again and again
    (tests/test_gpu_statements.py's shape): the transfers as packed, shared by the tests below."""
    n_acc, hot = 4200, 600
    accounts = b"".join(pack_account(id=account_id(i), ledger=1, code=1) for i in range(n_acc))
    bodies = [b"".join(pack_transfer(id=10**6 + 4000 * k + j, debit_account_id=account_id((7 * j) % hot),
                                     credit_account_id=account_id(hot + (j * 13 + k) % (n_acc - hot)), amount=(1 << 63) + j, ledger=1,
                                     code=1, flags=PENDING if (j // hot) % 3 == 0 else 0) for j in range(4000)) for k in range(2)]
    return dict(n_acc=n_acc, hot=hot, accounts=accounts, bodies=bodies)


def test_capacity_shapes_and_invalid_sizes(wide, gpu_engine_factory):
    """1 x 4,095 and 4,095 x 1: the longest lists, 4,096 positions in the set and the maps.  4,096
    cells, a product that overflows 32 bits and NULL lists are invalid and write nothing."""
    n_acc, hot = wide["n_acc"], wide["hot"]
    engine = gpu_engine_factory(accounts_max=1 << 13, transfers_max=1 << 14)
    assert engine.commit(128, 10**12, wide["accounts"]) == b""
    for k, body in enumerate(wide["bodies"]):
        assert engine.commit(129, 2 * 10**12 + k * 10**6, body) == b""
    transfers = engine.export_transfers()
    assert len(transfers) == 8000
    checker = FlowMatrix(transfers, engine.export_accounts())
    stamps = [int(t) for t in np.sort(transfers["timestamp"])]
    long_list = [account_id(i) for i in range(n_acc - 1, n_acc - 1 - MAX, -1)]  # every cold account and most hot ones
    got = check(engine, checker, [account_id(7)], long_list, 0, 0)
    assert len(got) == MAX and int(got["transfers"].sum()) == 2 * len(range(1, 4000, hot)) and (got["posted_hi"] == 0).all()
    got = check(engine, checker, long_list, [account_id(hot + 13 * 50)], stamps[10], stamps[-100])  # j = 50 pays it, from account 350
    assert len(got) == MAX and int(got["transfers"].sum()) > 0
    check(engine, checker, long_list, [account_id(7)], 0, stamps[4000])  # a hot account asked as credit: nothing
    rng = random.Random(9)
    mixed = [account_id(rng.randrange(n_acc)) for _ in range(60)] + [account_id(n_acc + 1 + i) for i in range(3)]
    rng.shuffle(mixed)
    got = check(engine, checker, mixed, [account_id(hot + i) for i in range(65)], stamps[10], 0)
    assert 0 < len(got) < MAX  # ids past the table are skipped
    # One cell too many, a product past 32 bits, NULL lists.
    ids64 = long_list[:64]
    status, result, raw = raw_call(engine, 0, 0, ids64, 64, ids64, 64, 4096)
    assert status == _lib.STATUS_INVALID and result == (77, 77, 77) and raw == b"\xAB" * len(raw)
    status, result, raw = raw_call(engine, 0, 0, ids64[:1], 1, ids64, 4096, 4096)
    assert status == _lib.STATUS_INVALID and result == (77, 77, 77) and raw == b"\xAB" * len(raw)
    status, result, raw = raw_call(engine, 0, 0, ids64, 1 << 16, ids64, 1 << 16, 4096)  # 2^32: zero in 32 bits
    assert status == _lib.STATUS_INVALID and result == (77, 77, 77) and raw == b"\xAB" * len(raw)
    status, result, raw = raw_call(engine, 0, 0, ids64, 0x80000001, ids64, 2, 4096)  # 2 in 32 bits
    assert status == _lib.STATUS_INVALID and result == (77, 77, 77) and raw == b"\xAB" * len(raw)


def test_eviction_and_orphaned_posts(ledger, gpu_engine_factory):
    """After tbgpu_evict_transfers of an old prefix `complete` is 0 and the cells are the checker's over
    the resident export.  And posts whose pending transfers were never loaded, with nothing evicted:
    `complete` drops exactly when such a post lies in an asked cell inside the period."""
    transfers, accounts, everyone = ledger["transfers"], ledger["accounts"], ledger["everyone"]
    evicted = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(ledger["sc"], evicted)
    evicted.checkpoint_delta()
    assert evicted.evict_transfers(700) > 0
    resident = evicted.export_transfers()
    checker = FlowMatrix(resident, evicted.export_accounts())
    stamps = [int(t) for t in np.sort(resident["timestamp"])]
    third, half = stamps[len(stamps) // 3], stamps[len(stamps) // 2]
    assert checker.of(everyone, everyone, stamps[0] - 1, 0)[2] and len(stamps) > 100  # an orphan post is resident
    for t_open, t_close in ((0, third), (stamps[0] - 1, 0), (half, stamps[-5]), (1, stamps[0] - 1)):
        for debit, credit in requests_of(ledger):
            check(evicted, checker, debit, credit, t_open, t_close, evicted=True)
    # Loaded without some pending transfers: nothing was evicted, the orphans alone drop `complete`.
    states = posted_states(transfers, ledger["posted"])
    pending = {u128(t, "id"): t for t in transfers if int(t["flags"]) & PENDING}
    posts = [t for t in transfers if int(t["flags"]) & POST and not int(t["flags"]) & PENDING
             and u128(t, "amount") < u128(pending[u128(t, "pending_id")], "amount")
             and u128(t, "debit_account_id") != u128(t, "credit_account_id")]
    assert len(posts) > 3
    orphans = posts[len(posts) // 2:]
    lost = {u128(p, "pending_id") for p in orphans}
    keep = np.array([u128(t, "id") not in lost for t in transfers])
    engine = gpu_engine_factory(transfers_max=1 << 14)
    engine.load_accounts(accounts)
    engine.load_transfers(transfers[keep], states[keep])
    engine.set_commit_timestamp(ledger["commit_timestamp"])
    checker = FlowMatrix(engine.export_transfers(), engine.export_accounts())
    o = min(orphans, key=lambda p: int(p["timestamp"]))  # the oldest orphan post
    d, c, ts = u128(o, "debit_account_id"), u128(o, "credit_account_id"), int(o["timestamp"])
    other = [i for i in everyone if i not in (d, c)]
    requests = [([d], [c], ts - 1, ts), (other[:3] + [d], [c] + other[3:9], ts - 1, ts), ([c], [d], ts - 1, ts),
                ([d], other, ts - 1, ts), (other, [c], ts - 1, ts), ([d], [c], 0, ts - 1), ([d, c], [d, c], ts, ts),
                (everyone, everyone, 0, 0), (everyone, everyone, 0, ts - 1), ([d], [c], 0, 0)]
    verdicts = []
    for debit, credit, t_open, t_close in requests:
        check(engine, checker, debit, credit, t_open, t_close)
        verdicts.append(checker.of(debit, credit, t_open, t_close)[2])
    assert verdicts == [True, True, False, False, False, False, False, True, False, True]
    cell = engine.get_account_flow_matrix([d], [c], ts - 1, ts)[0][0]
    assert cell_sums(cell) == (u128(o, "amount"), 0, u128(o, "amount"), 1)  # P = its own amount
    # Under the cap or not.
    check(engine, checker, other[:3] + [d], [c] + other[3:9], ts - 1, ts, cap=2)
    assert engine.get_account_flow_matrix(other[:3] + [d], [c], ts - 1, ts, 0)[2] is False
    # The statements call sums every record that names d, this call only the cells asked for.
    assert engine.get_account_statements([d], ts - 1, ts)[2] is False
    assert engine.get_account_flow_matrix([d], other, ts - 1, ts)[2] is True
    assert engine.get_account_statements([d], 0, ts - 1)[2] is False  # (its tail holds the orphan too)
    assert engine.get_account_flow_matrix([d], [c], 0, ts - 1)[2] is True


def test_restart_and_unordered_log(gpu_engine_factory):
    """The accounts loaded, the newer half committed, then the older half loaded shuffled: older
    timestamps sit behind newer ones in the log, records inside and outside every period share tiles,
    and the answers still equal the checker."""
    kw = dict(n_accounts=8, n_transfer_batches=20, batch_len=(100, 300), p_pending=0.3, p_dup=0.05, p_linked=0.05,
              p_limit=0.0, p_balancing=0.0, p_invalid=0.05, id_space=1 << 40)
    sa = make_scenario(31, p_post_void=0.25, **kw)
    last = sa.steps[-1][2]
    sb = make_scenario(32, p_post_void=0.25, start_ts=last + 10**9, **kw)
    acct_steps = [s for s in sa.steps if s[1] == 128]
    a_steps = [s for s in sa.steps if s[1] == 129]
    b_steps = [s for s in sb.steps if s[1] == 129]
    oracle = OracleEngine(64, 1 << 15)
    engine1 = gpu_engine_factory(transfers_max=1 << 15)
    engine2 = gpu_engine_factory(transfers_max=1 << 15)
    commit_all(sa, oracle, engine1, steps=acct_steps + a_steps)
    half_a = engine1.export_transfers()
    states = posted_states(half_a, engine1.export_posted())
    engine2.load_accounts(engine1.export_accounts())
    engine2.set_commit_timestamp(last)
    ids = request_of(oracle.export_accounts(), ABSENT)
    # Restarted from the balances alone, an empty log: every cell is there and zero.
    loaded = FlowMatrix(engine2.export_transfers(), engine2.export_accounts())
    cells = check(engine2, loaded, ids, ids, 0, last)
    assert len(cells) == (len(ids) - 4) ** 2 and int(cells["transfers"].sum()) == 0
    commit_all(sb, oracle, engine2, steps=b_steps)
    order = np.random.default_rng(5).permutation(len(half_a))
    engine2.load_transfers(half_a[order], states[order])
    transfers = oracle.export_transfers()
    assert engine2.export_transfers().tobytes() == transfers.tobytes()
    assert len(half_a) > 500 and len(transfers) - len(half_a) > 500
    checker = FlowMatrix(engine2.export_transfers(), engine2.export_accounts())
    stamps = [int(t) for t in np.sort(transfers["timestamp"])]
    created = sorted(int(a["timestamp"]) for a in oracle.export_accounts())
    marks = [0, created[0] - 1, created[0], created[-1], stamps[0], stamps[len(half_a) // 2], int(half_a["timestamp"].max()), last,
             last + 1, stamps[len(half_a) + 50], stamps[-1], 0]
    everyone = [u128(a, "id") for a in oracle.export_accounts()]
    for t_open, t_close in list(zip(marks[:-1], marks[1:])) + [(marks[1], marks[-2]), (marks[4], 0), (0, marks[7])]:
        check(engine2, checker, ids, ids, t_open, t_close)
        check(engine2, checker, ids[:5], ids[3:], t_open, t_close)
        if t_open <= t_close or t_close == 0:
            check_statements(engine2, everyone, t_open, t_close)
    oldest = check(engine2, checker, ids, ids, 0, created[0])  # only the oldest account, as often as it is named
    assert 0 < len(oldest) <= 9 and len({pair_of(c) for c in oldest}) == 1


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)], ids=["node2", "node3"])
def test_node(devices, ledger, gpu_engine_factory):
    sc, checker, transfers = ledger["sc"], ledger["checker"], ledger["transfers"]
    world = len(devices)
    posts = transfers[(transfers["flags"] & POST) != 0]
    home = homes_of(np.stack([posts["id_lo"], posts["id_hi"]], axis=1), world)
    pending_home = homes_of(np.stack([posts["pending_id_lo"], posts["pending_id_hi"]], axis=1), world)
    assert np.any(home != pending_home)  # a post reads its pending transfer on another shard
    single = gpu_engine_factory(transfers_max=1 << 14)
    engine = gpu_engine_factory(accounts_max=4096, transfers_max=1 << 14, pass_events_max=2048, pass_batches_max=16,
                                devices=devices)
    assert commit_all(sc, engine, single) == ledger["replies"]
    for t_open, t_close in ledger["sweep"]:
        for debit, credit in requests_of(ledger):
            got = check(engine, checker, debit, credit, t_open, t_close)
            assert got.tobytes() == single.get_account_flow_matrix(debit, credit, t_open, t_close)[0].tobytes()
    debit, credit = ledger["ids"][:9], ledger["ids"][5:40]
    t_open, t_close = max((p for p in ledger["sweep"] if p[0] and p[1]), key=lambda p: p[1] - p[0])
    whole = check(engine, checker, debit, credit, t_open, t_close)
    width = len(whole) // 9
    for cap in (0, 1, width - 1, len(whole), len(whole) + 3):
        check(engine, checker, debit, credit, t_open, t_close, cap=cap)
    status, result, raw = raw_call(engine, t_open, t_close, debit, len(debit), credit, len(credit), width + 5)
    assert status == _lib.STATUS_OK and result == (width + 5, 1, len(whole))
    assert raw[:(width + 5) * CELL] == whole[:width + 5].tobytes() and raw[(width + 5) * CELL:] == b"\xAB" * (len(raw) - (width + 5) * CELL)
    check_statements(engine, ledger["everyone"], t_open, t_close)


def test_read_only_and_allocation_free(ledger, gpu_engine_factory):
    """50 calls around which the allocation count, commit_timestamp, the exports and the commit-path
    counters of tbgpu_get_stats stand still; one more inside an asynchronous write-back; then the
    next commit answers as the oracle did."""
    sc, transfers, ids = ledger["sc"], ledger["transfers"], ledger["ids"]
    engine = gpu_engine_factory(transfers_max=1 << 14)
    twin = gpu_engine_factory(transfers_max=1 << 14)
    commit_all(sc, engine, twin, steps=sc.steps[:-1])
    resident = engine.export_transfers()
    checker = FlowMatrix(resident, engine.export_accounts())
    before = (engine.commit_timestamp, engine.export_accounts().tobytes(), resident.tobytes(), engine.export_posted().tobytes())
    rng = random.Random(3)
    allocations = engine.lib.tbgpu_debug_allocations()
    stats = engine.stats()
    stamps = [int(t) for t in np.sort(resident["timestamp"])]
    marks = [0, 1, stamps[len(stamps) // 3], stamps[-5], stamps[-1] + 7]
    for _ in range(50):
        t_open = rng.choice(marks)
        t_close = rng.choice([0] + [m for m in marks if m >= t_open])
        engine.get_account_flow_matrix(rng.sample(ids, rng.choice((1, 5, 50))), rng.sample(ids, rng.choice((1, 7, 60))), t_open, t_close)
    assert engine.lib.tbgpu_debug_allocations() == allocations
    after = engine.stats()
    assert all(after[k] == stats[k] for k in ("passes", "events", "transfers", "accounts", "log_used"))
    assert before == (engine.commit_timestamp, engine.export_accounts().tobytes(), engine.export_transfers().tobytes(),
                      engine.export_posted().tobytes())
    # One between an asynchronous write-back's start and its wait leaves the delta alone.
    caps = (1 << 14, 1 << 14, 1 << 14)
    engine.checkpoint_delta_async(caps)
    allocations = engine.lib.tbgpu_debug_allocations()
    check(engine, checker, ledger["same"], ledger["same"], stamps[len(stamps) // 3], stamps[-5])
    assert engine.lib.tbgpu_debug_allocations() == allocations
    delta = engine.checkpoint_delta_wait()
    sync = twin.checkpoint_delta(caps)
    assert len(delta.transfers) == len(resident)
    assert delta.transfers.tobytes() == sync.transfers.tobytes() and delta.posted.tobytes() == sync.posted.tobytes()
    assert by_id(delta.accounts) == by_id(sync.accounts) and delta.created_after == sync.created_after
    # ... and the next commit still answers as the oracle did.
    _, op, ts, batch = sc.steps[-1]
    assert engine.commit(op, ts, b"".join(batch)) == ledger["replies"][-1]
    assert engine.commit_timestamp == ledger["commit_timestamp"]
    assert engine.export_transfers().tobytes() == transfers.tobytes()
    assert engine.export_accounts().tobytes() == ledger["accounts"].tobytes()


def test_on_an_engine_a_device_panic_stopped(gpu_engine_factory):
    """tests/test_gpu_alloc.py's way to a device panic (a post whose checked `-=` traps after the setup
    action zeroed the pending balance).  The stopped engine still answers."""
    engine = gpu_engine_factory()
    accounts = b"".join(pack_account(id=i, ledger=1, code=1) for i in (1, 2))
    assert engine.commit(128, 10, accounts) == b""
    assert engine.commit(129, 20, pack_transfer(id=10, debit_account_id=1, credit_account_id=2, amount=100, ledger=1, code=1,
                                                flags=PENDING)) == b""
    assert engine.commit(129, 25, pack_transfer(id=12, debit_account_id=2, credit_account_id=1, amount=7, ledger=1, code=1)) == b""
    healthy, matched, complete = engine.get_account_flow_matrix([1, 2], [1, 2], 10, 25)
    assert matched == 4 and complete
    assert [cell_sums(c) for c in healthy] == [(0, 0, 0, 0), (0, 100, 0, 1), (7, 0, 0, 1), (0, 0, 0, 0)]
    assert net_positions(healthy) == {1: 7, 2: -7}
    engine.set_balances(1, 0, 0, 0, 0)
    with pytest.raises(EnginePanic):
        engine.commit(129, 30, pack_transfer(id=11, pending_id=10, flags=POST))
    with pytest.raises(EnginePanic, match="stopped"):
        engine.commit(129, 40, pack_transfer(id=13, debit_account_id=1, credit_account_id=2, amount=1, ledger=1, code=1))
    checker = FlowMatrix(engine.export_transfers(), engine.export_accounts())
    allocations = engine.lib.tbgpu_debug_allocations()
    for t_open, t_close in ((0, 0), (10, 20), (19, 24), (20, 0), (24, 25)):
        want, matched, _ = checker.of([2, 1, 2], [1, 2], t_open, t_close)
        got, got_matched, _ = engine.get_account_flow_matrix([2, 1, 2], [1, 2], t_open, t_close)
        assert got.tobytes() == want.tobytes() and got_matched == matched == 6
    assert engine.lib.tbgpu_debug_allocations() == allocations


def test_invalid_input(ledger, gpu_engine_factory):
    sc, ids = ledger["sc"], ledger["same"]
    engine = gpu_engine_factory(transfers_max=1 << 12)
    empty = engine.get_account_flow_matrix(ids, ids, 0, 9)
    assert len(empty[0]) == 0 and empty[0].dtype == FLOW_CELL_DTYPE and empty[1:] == (0, True)  # an empty engine
    commit_all(sc, engine, steps=sc.steps[:4])
    t0, t1, t2 = sc.steps[1][2], sc.steps[2][2], sc.steps[3][2]
    valid, matched, complete = engine.get_account_flow_matrix(ids, ids, t0, t2)
    assert matched == len(valid) == (len(ids) - 4) ** 2 and complete
    assert valid["transfers"].sum() > 0
    n = len(ids)
    # Invalid periods are answered OK with zeros and write nothing.
    for t_open, t_close in ((U64_MAX, 0), (0, U64_MAX), (U64_MAX, U64_MAX), (t1, t0), (t2, 1)):
        got, m, complete = engine.get_account_flow_matrix(ids, ids, t_open, t_close)
        assert len(got) == 0 and m == 0 and complete
        status, result, raw = raw_call(engine, t_open, t_close, ids, n, ids, n, n * n)
        assert status == _lib.STATUS_OK and result == (0, 1, 0) and raw == b"\xAB" * len(raw)
    for debit, credit in (([], ids), (ids, []), ([], [])):
        got, m, complete = engine.get_account_flow_matrix(debit, credit, t0, t2)
        assert len(got) == 0 and m == 0 and complete
    fn = engine.lib.tbgpu_get_account_flow_matrix
    src = ctypes.create_string_buffer(ids_body(ids), 16 * n)
    sentinel = b"\xAB" * (CELL * n * n)
    out = ctypes.create_string_buffer(sentinel, len(sentinel))
    res = _lib.tbgpu_query_result(count=77, complete=77, matched=77)
    untouched = lambda: out.raw == sentinel and (res.count, res.complete, res.matched) == (77, 77, 77)
    r = ctypes.byref(res)
    assert fn(engine.h, t0, t2, src, 0, src, n, out, n * n, r) == _lib.STATUS_OK and untouched()
    assert fn(engine.h, t0, t2, src, n, src, 0, out, n * n, r) == _lib.STATUS_OK and untouched()
    assert fn(engine.h, t0, t2, None, 0, None, n, None, 0, None) == _lib.STATUS_OK
    assert fn(engine.h, t0, t2, None, n, None, 0, None, 0, None) == _lib.STATUS_OK
    assert fn(engine.h, t0, t2, None, n, src, n, out, n * n, r) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, t0, t2, src, n, None, n, out, n * n, r) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, t0, t2, src, n, src, n, None, n * n, r) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, t0, t2, src, n, src, n, out, n * n, None) == _lib.STATUS_INVALID and out.raw == sentinel
    assert fn(engine.h, t0, t2, None, n, None, n, None, n * n, None) == _lib.STATUS_INVALID
    assert fn(engine.h, U64_MAX, 0, src, n, None, n, out, n * n, r) == _lib.STATUS_INVALID and untouched()  # NULL before the period
    assert fn(engine.h, t0, t2, src, 64, src, 64, out, n * n, r) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, t0, t2, src, 0xFFFFFFFF, src, 0xFFFFFFFF, out, n * n, r) == _lib.STATUS_INVALID and untouched()
    assert fn(engine.h, t0, t2, src, n, src, n, out, n * n, r) == _lib.STATUS_OK
    assert res.count == len(valid) and out.raw[:CELL * len(valid)] == valid.tobytes()
    assert out.raw[CELL * len(valid):] == sentinel[CELL * len(valid):]
