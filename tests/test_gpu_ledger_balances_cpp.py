"""tb::StateMachine::get_ledger_balances (tigerbeetle_amd/host/): the C++ mirror's answer to one request,
byte for byte the Python mirror's, through `tb_table_runner --query-ledgers`."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.harness.ledgers import ledgers_body
from tests.harness.workload import make_scenario


@pytest.mark.gpu
def test_cpp_mirror_ledger_balances_equal_python(tmp_path, gpu_engine_factory):
    from tigerbeetle_amd import build
    build.build(verbose=False)
    sc = make_scenario(2027, n_accounts=8, n_transfer_batches=3, batch_len=(100, 200), p_pending=0.3, p_post_void=0.25,
                       ledgers=(1, 7, 2**32 - 1))
    engine = gpu_engine_factory(transfers_max=1 << 14)
    for _, op, ts, events in sc.steps:
        engine.commit(op, ts, b"".join(events))
    transfers = engine.export_transfers()
    request = [2**32 - 1, 0, 7, 5, 1, 7]
    T = int(np.sort(transfers["timestamp"])[len(transfers) // 4])
    want, matched, complete = engine.get_ledger_balances(request, T)
    assert len(want) == matched == len(request) and complete
    assert want.tobytes() != engine.get_ledger_balances(request, 0)[0].tobytes()
    assert want["debits_posted_lo"].max() > 0 and want["ledger"].tolist() == request

    src, dst = str(tmp_path / "prepares.bin"), str(tmp_path / "answer.bin")
    with open(src, "wb") as out:
        for _, op, ts, events in sc.steps:
            body = b"".join(events)
            out.write(struct.pack("<QII", ts, op, len(body)) + body)
        out.write(struct.pack("<QII", 0, 0, 8 + 4 * len(request)) + struct.pack("<Q", T) + ledgers_body(request))
    r = subprocess.run([build.RUNNER, "--query-ledgers", src, dst, "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    answer = open(dst, "rb").read()
    count, cpp_complete, cpp_matched = struct.unpack("<IIQ", answer[:16])
    assert (count, cpp_matched, bool(cpp_complete)) == (len(want), matched, complete)
    assert answer[16:] == want.tobytes()
    assert os.path.getsize(dst) == 16 + 128 * count
