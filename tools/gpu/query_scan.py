"""The account-filter scan (tbgpu_get_account_transfers, csrc/k_query.h) over a 16M-transfer log (2 GB)
against a device-to-device copy of the same log range, in one process.

usage: python tools/gpu/query_scan.py [transfers] [runs]

The log is built by the device generator, committed in place (the way tools/gpu/device_pass.py builds
a pass): once with uniform C2 ids, where the queried account is a cold one (a few dozen matches), and
once with the Zipf draw, where it is the hottest account.  Each query (limit 8190, ascending and
newest first) is timed with the engine's markers, three warm-ups then the median of `runs`; so is the
copy.  Both load shapes of tb_query_count are measured (TBGPU_QUERY_COOP, read at tbgpu_init).
Prints one JSON line; the bar is query <= copy.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np  # noqa: E402

from tests.harness.configs import KINDS, batches, timestamps  # noqa: E402
from tigerbeetle_amd.state_machine import Engine, Options  # noqa: E402
from tigerbeetle_amd.types import TRANSFER_DTYPE  # noqa: E402

n_xfer = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 24
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 21
n_acct, batch, pb = 1_000_000, 8190, 512
WARMUPS = 3


def timed(e, fn):
    out = []
    for i in range(WARMUPS + runs):
        e.marker(0)
        fn()
        e.marker(1)
        e.sync()
        if i >= WARMUPS:
            out.append(e.marker_elapsed_ms(0, 1))
    return statistics.median(out), min(out), max(out)


def rates(ms):
    return dict(ms=round(ms, 4), log_gbs=round(n_xfer * 128 / ms / 1e6, 1), needed_gbs=round(n_xfer * 40 / ms / 1e6, 1))


def measure(coop):
    os.environ["TBGPU_QUERY_COOP"] = "1" if coop else "0"
    e = Engine(Options(accounts_max=n_acct, transfers_max=n_xfer, pass_events_max=pb * batch, pass_batches_max=pb))
    a_lens = batches(n_acct, batch)
    a_ts, t = timestamps(a_lens, 1_000_000_000)
    acct = e.alloc(n_acct * 128)
    e.generate_accounts(acct, 0, n_acct, seed=42)
    res = e.alloc(max(n_acct, n_xfer) * 8)
    rb = e.alloc((n_xfer // batch + 2) * 4)
    e.commit_device_async(128, a_ts, a_lens, acct, res, rb)
    e.sync()
    spare = e.alloc(n_xfer * 128)
    out = {}
    for name, kind in (("uniform_cold", "c2"), ("zipf_hot", "c3")):
        if name != "uniform_cold":
            e.reset_transfers()
        log = e.log_window(n_xfer)
        e.generate_transfers(log, 0, n_xfer, n_acct, seed=42, kind=KINDS[kind])
        e.sync()
        x_lens = batches(n_xfer, batch)
        x_ts, t = timestamps(x_lens, t + 10)
        e.commit_device_async(129, x_ts, x_lens, log, res, rb)
        e.sync()
        # The queried account: the debit account of the log's middle record (cold), or the most
        # frequent debit account of a sample (hot).
        sample = e.to_host(log + (n_xfer // 2) * 128, min(n_xfer // 2, 1 << 16) * 128).view(TRANSFER_DTYPE)
        if name == "uniform_cold":
            lo, hi = int(sample["debit_account_id_lo"][0]), int(sample["debit_account_id_hi"][0])
        else:
            ids, counts = np.unique(sample[["debit_account_id_lo", "debit_account_id_hi"]], return_counts=True)
            lo, hi = (int(v) for v in ids[np.argmax(counts)])
        account = lo | (hi << 64)
        for rev in (False, True):
            recs, matched, complete = e.get_account_transfers(account, reversed=rev, limit=8190)
            ts = recs["timestamp"].astype(np.int64)
            assert complete and len(recs) == min(matched, 8190) and np.all(np.diff(ts) < 0 if rev else np.diff(ts) > 0)
            med, lo_ms, hi_ms = timed(e, lambda: e.get_account_transfers(account, reversed=rev, limit=8190))
            out["%s_%s" % (name, "reversed" if rev else "ascending")] = dict(rates(med), min_ms=round(lo_ms, 4),
                                                                             max_ms=round(hi_ms, 4), matched=matched,
                                                                             count=len(recs))
        if name == "uniform_cold":
            med, lo_ms, hi_ms = timed(e, lambda: e.copy_device_async(spare, log, n_xfer * 128))
            out["copy_d2d"] = dict(rates(med), min_ms=round(lo_ms, 4), max_ms=round(hi_ms, 4))
    e.close()
    return out


result = dict(transfers=n_xfer, log_bytes=n_xfer * 128, runs=runs, warmups=WARMUPS,
              lane_per_record=measure(False), cooperative=measure(True))
for shape in ("lane_per_record", "cooperative"):
    r = result[shape]
    r["bar_query_le_copy"] = all(v["ms"] <= r["copy_d2d"]["ms"] for k, v in r.items() if k != "copy_d2d")
print(json.dumps(result))
