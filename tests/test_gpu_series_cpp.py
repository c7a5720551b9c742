"""tb::StateMachine::get_account_statement_series (tigerbeetle_amd/host/): the C++ mirror's answer to
one request, byte for byte the Python mirror's, through `tb_table_runner --query-series`."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.harness.balances import u128
from tests.harness.statements import ids_body
from tests.harness.workload import account_id, make_scenario


@pytest.mark.gpu
def test_cpp_mirror_series_equal_python(tmp_path, gpu_engine_factory):
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
    bounds = [int(stamps[len(transfers) * q // 8]) for q in range(1, 8)]
    n_buckets = len(bounds) - 1
    want, matched, complete = engine.get_account_statement_series(ids, bounds)
    assert len(want) == matched == (len(ids) - 2) * n_buckets and complete
    assert want["debits_posted_in_lo"].max() > 0 and want["credits_pending_out_lo"].max() > 0 and want["debit_transfers"].max() > 0
    assert len({row.tobytes() for row in want[:n_buckets]}) == n_buckets

    src, dst = str(tmp_path / "prepares.bin"), str(tmp_path / "answer.bin")
    with open(src, "wb") as out:
        for _, op, ts, events in sc.steps:
            body = b"".join(events)
            out.write(struct.pack("<QII", ts, op, len(body)) + body)
        request = struct.pack("<II", n_buckets, len(ids)) + struct.pack("<%dQ" % len(bounds), *bounds) + ids_body(ids)
        out.write(struct.pack("<QII", 0, 0, len(request)) + request)
    r = subprocess.run([build.RUNNER, "--query-series", src, dst, "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    answer = open(dst, "rb").read()
    count, cpp_complete, cpp_matched = struct.unpack("<IIQ", answer[:16])
    assert (count, cpp_matched, bool(cpp_complete)) == (len(want), matched, complete)
    assert answer[16:] == want.tobytes()
    assert os.path.getsize(dst) == 16 + 256 * count
