"""What the order of the transfer ids costs kernel 1 (tb_transfers_validate): C2 passes committed in
place as tools/gpu/device_pass.py does, with the generated events' `id` field rewritten in HBM (a
torch op) to one of three families, and validate's device-clock span per pass printed
(stats()["span_ms"][0]).  The index clusters consecutive ids (csrc/tb_device.h tb_xi_home), so
`reversed` and `sequential` claim a few 64-byte segments per wave and `random` one per id.

usage: [TBGPU_AB_LIB=.../libtbgpu_base.so] python tools/gpu/index_locality.py <family> [passes] [pass_prepares]
  family: reversed (as generated: maxInt - (k + 1)), sequential (k + 1), random (a 64-bit bijective mix of k)
Prints one JSON line.  Run a base build and the current one alternately (TBGPU_AB_LIB) to compare.
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests.harness.configs import KINDS, batches, timestamps  # noqa: E402
from tigerbeetle_amd.state_machine import Engine, Options  # noqa: E402

family = sys.argv[1] if len(sys.argv) > 1 else "reversed"
passes = int(sys.argv[2]) if len(sys.argv) > 2 else 10
pb = int(sys.argv[3]) if len(sys.argv) > 3 else 512
assert family in ("reversed", "sequential", "random")
n_acct, batch = 1_000_000, 8190
n_xfer = passes * pb * batch


def mix64(x):
    """tb_mix64 on int64 tensors (logical shifts; products wrap)."""
    def shr(v, s):
        return (v >> s) & ((1 << (64 - s)) - 1)
    x = x ^ shr(x, 31)
    x = x * torch.tensor(0x7fb5d329728ea185, dtype=torch.int64, device=x.device)
    x = x ^ shr(x, 27)
    x = x * torch.tensor(0x81dadef4bc2dd44d - (1 << 64), dtype=torch.int64, device=x.device)
    return x ^ shr(x, 33)


# Tables sized as the headline engine (100M transfers: a 2-GB index), whatever this run commits.
e = Engine(Options(accounts_max=n_acct, transfers_max=max(n_xfer, 100_000_000), pass_events_max=pb * batch,
                   pass_batches_max=pb, profile=True))
a_lens = batches(n_acct, batch)
a_ts, t = timestamps(a_lens, 1_000_000_000)
acct = e.alloc(n_acct * 128)
e.generate_accounts(acct, 0, n_acct, seed=42)
res = e.alloc(max(n_acct, n_xfer) * 8)
rb = e.alloc((n_xfer // batch + 2) * 4)
e.commit_device_async(128, a_ts, a_lens, acct, res, rb)
e.sync()

dev = torch.device("cuda", 0)
ev = torch.empty((n_xfer, 16), dtype=torch.int64, device=dev)  # 128-B events as 16 words: id = words 0, 1
e.generate_transfers(ev.data_ptr(), 0, n_xfer, n_acct, seed=42, kind=KINDS["c2"])
e.sync()
if family != "reversed":
    k1 = torch.arange(1, n_xfer + 1, dtype=torch.int64, device=dev)
    ev[:, 0] = k1 if family == "sequential" else mix64(k1)  # a bijection of k + 1 >= 1: never 0
    ev[:, 1] = 0
    del k1
torch.cuda.synchronize()
window = e.log_window(n_xfer)
e.copy_device_async(window, ev.data_ptr(), n_xfer * 128)
e.sync()
del ev

x_lens = batches(n_xfer, batch)
x_ts, _ = timestamps(x_lens, t + 10)
e.profile_mask(e.PROF_SPANS)
e.reset_stats()
e.commit_device_async(129, x_ts, x_lens, window, res, rb)
e.sync()
st = e.stats()
replies = e.to_host(rb, len(x_lens) * 4).view(np.uint32)
launches = st["span_launches"][0]
print(json.dumps({"family": family, "lib": os.path.basename(os.environ.get("TBGPU_AB_LIB", "libtbgpu.so")),
                  "transfers": n_xfer, "pass_prepares": pb, "validate_launches": launches,
                  "validate_ms_per_pass": round(st["span_ms"][0] / max(launches, 1), 4),
                  "reply_bytes": int(replies.sum()), "stored": st["transfers"]}))
e.close()
