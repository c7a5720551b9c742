"""tb::StateMachine::get_account_transfers_many (tigerbeetle_amd/host/): the C++ mirror's answers to a
batch of five account filters — mixed directions, one invalid, one duplicate — byte for byte the
Python mirror's, through `tb_table_runner --query-many`."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.harness.workload import make_scenario
from tests.test_gpu_query import brute, ids_of
from tigerbeetle_amd.state_machine import Engine


@pytest.mark.gpu
def test_cpp_mirror_query_many_equals_python(tmp_path, gpu_engine_factory):
    from tigerbeetle_amd import build
    build.build(verbose=False)
    sc = make_scenario(2027, n_accounts=8, n_transfer_batches=3, batch_len=(100, 200), p_pending=0.3, p_post_void=0.25)
    engine = gpu_engine_factory(transfers_max=1 << 14)
    for _, op, ts, events in sc.steps:
        engine.commit(op, ts, b"".join(events))
    transfers = engine.export_transfers()
    accounts = sorted(ids_of(transfers), key=lambda a: -brute(transfers, a)[1])
    quarter = int(np.sort(transfers["timestamp"])[len(transfers) // 4])
    filters = [Engine.account_filter(accounts[0], reversed=True, limit=10, timestamp_min=quarter),
               Engine.account_filter(accounts[1], credits=False, limit=8190),
               Engine.account_filter(accounts[2], limit=0),                      # invalid
               Engine.account_filter(accounts[0], reversed=True, limit=10, timestamp_min=quarter),  # a duplicate
               Engine.account_filter(accounts[3], debits=False, limit=3)]
    want = engine.get_account_transfers_many(filters)
    assert [len(g) for g, _, _ in want][0::2] == [10, 0, 3] and want[0][1] > 10 and want[1][1] == len(want[1][0]) > 0
    assert want[3][0].tobytes() == want[0][0].tobytes() and all(c for _, _, c in want)

    src, dst = str(tmp_path / "prepares.bin"), str(tmp_path / "answer.bin")
    with open(src, "wb") as out:
        for _, op, ts, events in sc.steps:
            body = b"".join(events)
            out.write(struct.pack("<QII", ts, op, len(body)) + body)
        out.write(struct.pack("<QII", 0, 0, 64 * len(filters)) + b"".join(filters))
    r = subprocess.run([build.RUNNER, "--query-many", src, dst, "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    answer = open(dst, "rb").read()
    at = 0
    for records, matched, complete in want:
        count, cpp_complete, cpp_matched = struct.unpack("<IIQ", answer[at:at + 16])
        assert (count, cpp_matched, bool(cpp_complete)) == (len(records), matched, complete)
        assert answer[at + 16:at + 16 + 128 * count] == records.tobytes()
        at += 16 + 128 * count
    assert os.path.getsize(dst) == at
