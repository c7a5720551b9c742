"""tb::StateMachine::get_active_accounts (tigerbeetle_amd/host/): the C++ mirror's answer to one request
in the by-id and the by-volume order, byte for byte the Python mirror's, through `tb_table_runner
--query-active`."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.harness.workload import make_scenario
from tigerbeetle_amd.types import ACTIVE_BY_VOLUME, pack_activity_filter


@pytest.mark.gpu
def test_cpp_mirror_active_accounts_equal_python(tmp_path, gpu_engine_factory):
    from tigerbeetle_amd import build
    build.build(verbose=False)
    sc = make_scenario(2027, n_accounts=8, n_transfer_batches=3, batch_len=(100, 200), p_pending=0.3, p_post_void=0.25)
    engine = gpu_engine_factory(transfers_max=1 << 14)
    for _, op, ts, events in sc.steps:
        engine.commit(op, ts, b"".join(events))
    transfers = engine.export_transfers()
    stamps = np.sort(transfers["timestamp"])
    t_open, t_close = int(stamps[len(transfers) // 8]), int(stamps[len(transfers) * 7 // 8])
    for flags, limit in ((3, 8191), (3 | ACTIVE_BY_VOLUME, 2)):
        request = pack_activity_filter(t_open, t_close, 0, 0, 0, limit, flags)
        want, matched, complete = engine.get_active_accounts_raw(request)
        assert len(want) == min(limit, matched) and matched > 2 and complete
        assert want["debits_posted_lo"].max() > 0 and want["credits_transfers"].max() > 1

        src, dst = str(tmp_path / "prepares.bin"), str(tmp_path / "answer.bin")
        with open(src, "wb") as out:
            for _, op, ts, events in sc.steps:
                body = b"".join(events)
                out.write(struct.pack("<QII", ts, op, len(body)) + body)
            out.write(struct.pack("<QII", 0, 0, len(request)) + request)
        r = subprocess.run([build.RUNNER, "--query-active", src, dst, "0"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        answer = open(dst, "rb").read()
        count, cpp_complete, cpp_matched = struct.unpack("<IIQ", answer[:16])
        assert (count, cpp_matched, bool(cpp_complete)) == (len(want), matched, complete)
        assert answer[16:] == want.tobytes()
        assert os.path.getsize(dst) == 16 + 128 * count
