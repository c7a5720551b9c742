"""tb::StateMachine::get_account_balances (tigerbeetle_amd/host/): the C++ mirror's answer to one
account filter, byte for byte the Python mirror's, through `tb_table_runner --query-balances`."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.harness.workload import make_scenario
from tests.test_gpu_query import brute, ids_of
from tigerbeetle_amd.state_machine import Engine


@pytest.mark.gpu
def test_cpp_mirror_balances_equal_python(tmp_path, gpu_engine_factory):
    from tigerbeetle_amd import build
    build.build(verbose=False)
    sc = make_scenario(2027, n_accounts=8, n_transfer_batches=3, batch_len=(100, 200), p_pending=0.3, p_post_void=0.25)
    engine = gpu_engine_factory(transfers_max=1 << 14)
    for _, op, ts, events in sc.steps:
        engine.commit(op, ts, b"".join(events))
    transfers = engine.export_transfers()
    account = max(ids_of(transfers), key=lambda a: brute(transfers, a)[1])
    f = Engine.account_filter(account, reversed=True, limit=10,
                              timestamp_min=int(np.sort(transfers["timestamp"])[len(transfers) // 4]))
    want, matched, complete = engine.get_account_balances_raw(f)
    assert len(want) == 10 and matched > 10 and complete
    assert want["timestamp"].tolist() == engine.get_account_transfers_raw(f)[0]["timestamp"].tolist()

    src, dst = str(tmp_path / "prepares.bin"), str(tmp_path / "answer.bin")
    with open(src, "wb") as out:
        for _, op, ts, events in sc.steps:
            body = b"".join(events)
            out.write(struct.pack("<QII", ts, op, len(body)) + body)
        out.write(struct.pack("<QII", 0, 0, 64) + f)
    r = subprocess.run([build.RUNNER, "--query-balances", src, dst, "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    answer = open(dst, "rb").read()
    count, cpp_complete, cpp_matched = struct.unpack("<IIQ", answer[:16])
    assert (count, cpp_matched, bool(cpp_complete)) == (len(want), matched, complete)
    assert answer[16:] == want.tobytes()
    assert os.path.getsize(dst) == 16 + 128 * count
