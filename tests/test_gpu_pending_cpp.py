"""tb::StateMachine::get_pending_transfers (tigerbeetle_amd/host/): the C++ mirror's answer to one
filter, byte for byte the Python mirror's, through `tb_table_runner --query-pending`."""
import os
import struct
import subprocess

import pytest

from tests.harness.pending import NS
from tests.harness.workload import make_scenario
from tigerbeetle_amd.types import PENDING_EXPIRED, PENDING_OPEN, PENDING_POSTED, PENDING_VOIDED


@pytest.mark.gpu
def test_cpp_mirror_pending_transfers_equal_python(tmp_path, gpu_engine_factory):
    from tigerbeetle_amd import build
    build.build(verbose=False)
    sc = make_scenario(2027, n_accounts=8, n_transfer_batches=3, batch_len=(100, 200), p_pending=0.3, p_post_void=0.25)
    engine = gpu_engine_factory(transfers_max=1 << 14)
    for _, op, ts, events in sc.steps:
        engine.commit(op, ts, b"".join(events))
    now = engine.commit_timestamp + 3 * NS
    f = engine.pending_filter(now=now, reversed=True, limit=100)
    want, states, matched, complete = engine.get_pending_transfers_raw(f)
    assert 0 < len(want) <= matched and complete
    assert set(states.tolist()) == {PENDING_OPEN, PENDING_EXPIRED, PENDING_POSTED, PENDING_VOIDED}
    assert want["resolution"]["timestamp"].any()

    src, dst = str(tmp_path / "prepares.bin"), str(tmp_path / "answer.bin")
    with open(src, "wb") as out:
        for _, op, ts, events in sc.steps:
            body = b"".join(events)
            out.write(struct.pack("<QII", ts, op, len(body)) + body)
        out.write(struct.pack("<QII", 0, 0, len(f)) + f)
    r = subprocess.run([build.RUNNER, "--query-pending", src, dst, "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    answer = open(dst, "rb").read()
    count, cpp_complete, cpp_matched = struct.unpack("<IIQ", answer[:16])
    assert (count, cpp_matched, bool(cpp_complete)) == (len(want), matched, complete)
    assert answer[16:16 + 256 * count] == want.tobytes() and answer[16 + 256 * count:] == states.tobytes()
    assert os.path.getsize(dst) == 16 + 257 * count
