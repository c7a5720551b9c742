"""tb::StateMachine::get_account_balance_extremes (tigerbeetle_amd/host/): the C++ mirror's answer to
one request, byte for byte the Python mirror's, through `tb_table_runner --query-extremes`."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.harness.balances import u128
from tests.harness.extremes import ids_body
from tests.harness.workload import account_id, make_scenario
from tigerbeetle_amd.types import MEASURE_CREDIT_AVAILABLE, extreme_value, pack_balance_measure


@pytest.mark.gpu
def test_cpp_mirror_extremes_equal_python(tmp_path, gpu_engine_factory):
    from tigerbeetle_amd import build
    build.build(verbose=False)
    sc = make_scenario(2027, n_accounts=8, n_transfer_batches=3, batch_len=(100, 200), p_pending=0.3, p_post_void=0.25)
    engine = gpu_engine_factory(transfers_max=1 << 14)
    for _, op, ts, events in sc.steps:
        engine.commit(op, ts, b"".join(events))
    transfers = engine.export_transfers()
    accounts = [u128(a, "id") for a in engine.export_accounts()]
    ids = accounts[::-1] + [account_id(5000), 0] + accounts[:3]
    stamps = np.sort(transfers["timestamp"])
    t_open, t_close = int(stamps[len(transfers) // 4]), int(stamps[3 * len(transfers) // 4])
    measure = MEASURE_CREDIT_AVAILABLE
    want, matched, complete = engine.get_account_balance_extremes(ids, t_open, t_close, measure)
    assert len(want) == matched == len(ids) - 2 and complete
    assert want.tobytes() != engine.get_account_balance_extremes(ids, 0, 0, measure)[0].tobytes()
    assert (want["t_open"] == t_open).all() and (want["t_end"] == t_close).all() and (want["records"] > 0).all()
    assert all(extreme_value(r, "low") < extreme_value(r, "high") for r in want) and any(extreme_value(r, "low") < 0 for r in want)
    assert ((want["t_low"] > t_open) & (want["t_low"] < t_close)).any()

    src, dst = str(tmp_path / "prepares.bin"), str(tmp_path / "answer.bin")
    with open(src, "wb") as out:
        for _, op, ts, events in sc.steps:
            body = b"".join(events)
            out.write(struct.pack("<QII", ts, op, len(body)) + body)
        out.write(struct.pack("<QII", 0, 0, 24 + 16 * len(ids)) + struct.pack("<QQ", t_open, t_close) + pack_balance_measure(measure)
                  + ids_body(ids))
    r = subprocess.run([build.RUNNER, "--query-extremes", src, dst, "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    answer = open(dst, "rb").read()
    count, cpp_complete, cpp_matched = struct.unpack("<IIQ", answer[:16])
    assert (count, cpp_matched, bool(cpp_complete)) == (len(want), matched, complete)
    assert answer[16:] == want.tobytes()
    assert os.path.getsize(dst) == 16 + 192 * count
