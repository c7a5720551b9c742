"""Table of an A/B session (tools/gpu/ab.sh): per variant every run's rate, step times and validate's
device-clock span per pass, and the keep rule of DESIGN.md §4 for each variant against the first.

usage: python tools/gpu/ab_table.py <dir with ab_<variant>_<round>.log> [first variant, default base]
"""
import glob
import json
import os
import re
import sys

d = sys.argv[1]
first = sys.argv[2] if len(sys.argv) > 2 else "base"
runs = {}
for path in sorted(glob.glob(os.path.join(d, "ab_*_*.log"))):
    m = re.match(r"ab_(.+)_(\d+)\.log$", os.path.basename(path))
    line = json.loads(open(path).read().strip().splitlines()[-1])
    roof = line.get("roofline") or {}
    runs.setdefault(m.group(1), []).append((int(m.group(2)), line["value"] / 1e9, line["step_ms"],
                                             roof.get("avg_launch_ms"), roof.get("frac")))


def steps(v):
    return [s for _, _, st, _, _ in runs[v] for s in st]


for v in sorted(runs, key=lambda v: (v != first, v)):
    rs = sorted(runs[v])
    st = steps(v)
    spans = [r[3] for r in rs if r[3] is not None]
    print("%s runs %d G/s mean %.3f ms/step mean %.3f min %.3f max %.3f validate span mean %.4f [%.4f..%.4f]" % (
        v, len(rs), sum(r[1] for r in rs) / len(rs), sum(st) / len(st), min(st), max(st),
        sum(spans) / max(1, len(spans)), min(spans, default=0), max(spans, default=0)))
    for r in rs:
        print("   #%d %.3f G/s steps %s validate %s frac %s" % (r[0], r[1], r[2], r[3], r[4]))
if first in runs:
    b = steps(first)
    for v in sorted(runs):
        if v == first:
            continue
        s = steps(v)
        gain = sum(b) / len(b) - sum(s) / len(s)
        print("keep rule %s vs %s: every step below every step of %s: %s (max %.3f, %s min %.3f); mean gain %.3f ms, "
              "%s's spread %.3f ms: %s" % (v, first, first, max(s) < min(b), max(s), first, min(b), gain, first,
                                           max(b) - min(b), "KEEP" if max(s) < min(b) and gain > max(b) - min(b) else "DROP"))
