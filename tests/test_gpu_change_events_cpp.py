"""tb::StateMachine::get_change_events (tigerbeetle_amd/host/): the C++ mirror's answer to one
change-events filter, byte for byte the Python mirror's, through `tb_table_runner --query-change-events`."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.harness.workload import make_scenario
from tigerbeetle_amd.types import pack_change_events_filter


@pytest.mark.gpu
def test_cpp_mirror_change_events_equal_python(tmp_path, gpu_engine_factory):
    from tigerbeetle_amd import build
    build.build(verbose=False)
    sc = make_scenario(2027, n_accounts=8, n_transfer_batches=3, batch_len=(100, 200), p_pending=0.3, p_post_void=0.25)
    engine = gpu_engine_factory(transfers_max=1 << 14)
    for _, op, ts, events in sc.steps:
        engine.commit(op, ts, b"".join(events))
    transfers = engine.export_transfers()
    f = pack_change_events_filter(timestamp_min=int(np.sort(transfers["timestamp"])[len(transfers) // 4]), limit=10)
    want, matched, complete = engine.get_change_events_raw(f)
    assert len(want) == 10 and matched > 10 and complete
    assert want["transfer"].tobytes() == engine.query_transfers(
        timestamp_min=int(want["transfer"]["timestamp"][0]), limit=10)[0].tobytes()
    assert want["debit_account"]["debits_posted_lo"].max() > 0

    src, dst = str(tmp_path / "prepares.bin"), str(tmp_path / "answer.bin")
    with open(src, "wb") as out:
        for _, op, ts, events in sc.steps:
            body = b"".join(events)
            out.write(struct.pack("<QII", ts, op, len(body)) + body)
        out.write(struct.pack("<QII", 0, 0, 64) + f)
    r = subprocess.run([build.RUNNER, "--query-change-events", src, dst, "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    answer = open(dst, "rb").read()
    count, cpp_complete, cpp_matched = struct.unpack("<IIQ", answer[:16])
    assert (count, cpp_matched, bool(cpp_complete)) == (len(want), matched, complete)
    assert answer[16:] == want.tobytes()
    assert os.path.getsize(dst) == 16 + 384 * count
