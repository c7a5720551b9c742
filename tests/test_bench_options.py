"""bench.py's run modes: a plain run keeps only the timed steps (every other leg's size option is
ignored without --full), --full keeps the legs' defaults, and --dump-outputs writes what the last
timed step computed."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _parse(monkeypatch, *argv):
    spec = importlib.util.spec_from_file_location("bench_options_under_test", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench, bench.parse()


def test_plain_run_switches_every_other_leg_off(monkeypatch):
    bench, args = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2", "--host-steps", "3")
    assert args.steps == 7 and args.warmup == 2 and not args.full and args.dump_outputs is None
    assert all(getattr(args, leg) == 0 for leg in bench.FULL_LEGS)


def test_full_keeps_the_legs(monkeypatch):
    bench, args = _parse(monkeypatch, "--full", "--secondary", "0")
    assert args.full and args.secondary == 0
    assert all(getattr(args, leg) > 0 for leg in bench.FULL_LEGS if leg != "secondary")


def test_dump_outputs_is_single_gpu(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--gpus", "2", "--dump-outputs", "somewhere")


@pytest.mark.gpu
def test_dump_outputs_of_a_small_run(tmp_path):
    """C4 (failing events, two-phase transfers) at a small size: the dumped arrays are float64, agree
    with the result line and with each other, and stay far below the size limit."""
    out = tmp_path / "dump"
    n_acct, n_xfer, batch = 10_000, 200_000, 8190
    cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", "c4", "--accounts", str(n_acct),
           "--transfers", str(n_xfer), "--pass-batches", "8", "--dump-outputs", str(out)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    line = json.loads([x for x in run.stdout.splitlines() if x.startswith("{")][-1])
    assert line["steps"] == 2 and len(line["step_ms"]) == 2 and line["ms_per_step"] > 0
    assert line["host_path"] is None and line["cpu_baseline"] is None and line["secondary"] is None

    arrays = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(arrays) == ["accounts", "reply_bytes", "results", "transfers"]
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) < 64 << 20
    rb, res, accts, xfers = (arrays[k] for k in ("reply_bytes", "results", "accounts", "transfers"))
    n_prep = -(-n_xfer // batch)
    assert rb.shape == (n_prep,) and int(rb.sum()) // 8 == line["failed_events"] > 0
    assert accts.shape == (n_acct, 32) and xfers.shape == (256 * 256, 33) and res.shape == (256 * 256, 3)
    # the sample: runs of 256 consecutive events, each named by its prepare and its index there
    assert (res[:, 0] < n_prep).all() and (res[:, 1] < batch).all()
    pos = (res[:, 0] * batch + res[:, 1]).reshape(256, 256)
    assert (np.diff(pos, axis=1) == 1).all() and (np.diff(pos[:, 0]) > 0).all() and pos.max() < n_xfer
    # no more failures in a prepare's sampled events than its reply holds records
    failed = res[:, 2] > 0
    assert failed.any() and (np.bincount(res[failed, 0].astype(np.int64), minlength=n_prep) * 8 <= rb).all()
    # an event without a record in its reply is stored and carries its timestamp (words 30, 31)
    stored = xfers[:, 32] > 0
    assert stored[~failed].all() and 0 < stored.sum() < len(xfers)
    assert ((xfers[stored, 30] + xfers[stored, 31]) > 0).all() and (xfers[~stored, :32] == 0).all()


class _FakeEngine:
    """Device memory as one byte array; addresses are offsets into it."""

    def __init__(self, memory, accounts):
        self.memory, self.accounts = memory, accounts

    def to_host(self, ptr, nbytes):
        return self.memory[ptr:ptr + nbytes].copy()

    def export_accounts(self):
        return self.accounts

    def fetch_transfers(self, ids):
        from tigerbeetle_amd.types import TRANSFER_DTYPE
        out = np.zeros(len(ids), dtype=TRANSFER_DTYPE)
        out["id_lo"], out["timestamp"] = ids[:, 0], ids[:, 0] + 5
        return out, np.ones(len(ids), dtype=np.uint8)


def test_dump_outputs_decodes_sparse_replies(tmp_path, monkeypatch):
    """dump_outputs over a made-up step: three prepares of 300, 300 and 100 events, replies with
    records for events 7 and 299 of the first and 0 of the last."""
    from tigerbeetle_amd.types import ACCOUNT_DTYPE, TRANSFER_DTYPE
    bench, args = _parse(monkeypatch, "--seed", "3")
    lens, n = [300, 300, 100], 700
    events = np.zeros(n, dtype=TRANSFER_DTYPE)
    events["id_lo"] = np.arange(n) + 1000
    results = np.full((n, 2), 0xDEAD, dtype=np.uint32)  # stale beyond each reply's bytes
    results[0], results[1], results[600] = (7, 21), (299, 46), (0, 33)
    reply_bytes = np.array([16, 0, 8], dtype=np.uint32)
    src, res_dev, rb_dev = 0, events.nbytes, events.nbytes + results.nbytes
    memory = np.concatenate([events.view(np.uint8), results.view(np.uint8).reshape(-1), reply_bytes.view(np.uint8)])
    accounts = np.zeros(50, dtype=ACCOUNT_DTYPE)
    accounts["id_lo"] = np.arange(50) + 1
    bench.dump_outputs(str(tmp_path), _FakeEngine(memory, accounts), args, lens, src, res_dev, rb_dev)

    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(a.dtype == np.float64 and a.size > 0 for a in got.values())
    assert got["reply_bytes"].tolist() == [16, 0, 8]
    assert got["accounts"].shape == (50, 32) and got["accounts"][:, 0].tolist() == list(range(1, 51))
    res, xfers = got["results"], got["transfers"]
    assert res.shape == (512, 3) and xfers.shape == (512, 33)  # both runs of 256 events (700 // 256 = 2)
    pos = np.concatenate([[0], np.cumsum(lens)])[res[:, 0].astype(int)] + res[:, 1]
    assert pos.tolist() == list(range(512)) and (xfers[:, 0] == pos + 1000).all() and (xfers[:, 30] == pos + 1005).all()
    expect = np.zeros(512)
    expect[7], expect[299] = 21, 46  # event 600 lies outside the sampled runs
    assert (res[:, 2] == expect).all()
