"""tb::StateMachine::query_transfers / query_accounts (tigerbeetle_amd/host/): the C++ mirror's answer to
one field filter each, byte for byte the Python mirror's, through `tb_table_runner --query-fields`."""
import os
import struct
import subprocess

import pytest

from tests.test_gpu_query_filter import U128_VALUES, make_workload, run
from tigerbeetle_amd.state_machine import Engine


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["transfers", "accounts"])
def test_cpp_mirror_query_equals_python(which, tmp_path, gpu_engine_factory):
    from tigerbeetle_amd import build
    build.build(verbose=False)
    steps = make_workload(79, {1: 300, 2: 100}, 250, 4, 200, 12)
    engine = gpu_engine_factory(transfers_max=1 << 14)
    run(steps, engine)
    if which == "transfers":
        f = Engine.query_filter(ledger=1, code=2, reversed=True, limit=10,
                                timestamp_min=int(engine.export_transfers()["timestamp"][100]))
        want, matched, complete = engine.query_transfers_raw(f)
    else:
        f = Engine.query_filter(user_data_128=U128_VALUES[2], ledger=1, reversed=True, limit=10)
        want, matched, complete = engine.query_accounts_raw(f)
    assert len(want) == 10 and matched > 10 and complete

    src, dst = str(tmp_path / "prepares.bin"), str(tmp_path / "answer.bin")
    with open(src, "wb") as out:
        for op, ts, body in steps:
            out.write(struct.pack("<QII", ts, op, len(body)) + body)
        out.write(struct.pack("<QII", 0, 0, 64) + f)
    r = subprocess.run([build.RUNNER, "--query-fields", which, src, dst, "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    answer = open(dst, "rb").read()
    count, cpp_complete, cpp_matched = struct.unpack("<IIQ", answer[:16])
    assert (count, cpp_matched, bool(cpp_complete)) == (len(want), matched, complete)
    assert answer[16:] == want.tobytes()
    assert os.path.getsize(dst) == 16 + 128 * count
