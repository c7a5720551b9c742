"""tb::StateMachine::get_account_flow_matrix (tigerbeetle_amd/host/): the C++ mirror's answer to one
request, byte for byte the Python mirror's, through `tb_table_runner --query-flow-matrix`."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.harness.balances import u128
from tests.harness.statements import ids_body
from tests.harness.workload import account_id, make_scenario


@pytest.mark.gpu
def test_cpp_mirror_flow_matrix_equal_python(tmp_path, gpu_engine_factory):
    from tigerbeetle_amd import build
    build.build(verbose=False)
    sc = make_scenario(2027, n_accounts=8, n_transfer_batches=3, batch_len=(100, 200), p_pending=0.3, p_post_void=0.25)
    engine = gpu_engine_factory(transfers_max=1 << 14)
    for _, op, ts, events in sc.steps:
        engine.commit(op, ts, b"".join(events))
    transfers = engine.export_transfers()
    accounts = [u128(a, "id") for a in engine.export_accounts()]
    debit = accounts[::-1] + [account_id(5000), 0] + accounts[:3]
    credit = accounts[2:] + [account_id(5001)] + accounts[1:2]
    stamps = np.sort(transfers["timestamp"])
    t_open, t_close = int(stamps[len(transfers) // 8]), int(stamps[len(transfers) * 7 // 8])
    want, matched, complete = engine.get_account_flow_matrix(debit, credit, t_open, t_close)
    assert len(want) == matched == (len(debit) - 2) * (len(credit) - 1) and complete
    assert want["posted_lo"].max() > 0 and want["pending_in_lo"].max() > 0 and want["pending_out_lo"].max() > 0
    assert want["transfers"].max() > 1 and (want["transfers"] == 0).any()

    src, dst = str(tmp_path / "prepares.bin"), str(tmp_path / "answer.bin")
    with open(src, "wb") as out:
        for _, op, ts, events in sc.steps:
            body = b"".join(events)
            out.write(struct.pack("<QII", ts, op, len(body)) + body)
        request = struct.pack("<QQII", t_open, t_close, len(debit), len(credit)) + ids_body(debit) + ids_body(credit)
        out.write(struct.pack("<QII", 0, 0, len(request)) + request)
    r = subprocess.run([build.RUNNER, "--query-flow-matrix", src, dst, "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    answer = open(dst, "rb").read()
    count, cpp_complete, cpp_matched = struct.unpack("<IIQ", answer[:16])
    assert (count, cpp_matched, bool(cpp_complete)) == (len(want), matched, complete)
    assert answer[16:] == want.tobytes()
    assert os.path.getsize(dst) == 16 + 96 * count
