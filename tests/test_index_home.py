"""The transfer index's layout (csrc/tb_device.h tb_xi_home / tb_xi_next / tb_xi_steps), checked on
the host through tools/index_home.cpp, which includes the engine's own header:

* the G ids of a group (id >> log2 G) land in one 64-byte segment on G distinct slots;
* a probe path is a cycle of xidx_cap / G entries that never leaves its slot class;
* id families whose low bits are skewed still fill the G classes, and the segments, evenly.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "index_home.cpp")
BIN = os.path.join(ROOT, "tools", "bin", "index_home")
CAPS = [2048, 32768]
FAMILIES = ["sequential", "reversed", "shl3", "shl16", "hi", "scramble"]
U64 = (1 << 64) - 1


def build_index_home():
    """tools/bin/index_home, compiled host-only from tools/index_home.cpp (no GPU code, no GPU)."""
    from tigerbeetle_amd import build
    deps = [SRC, os.path.join(build.CSRC, "tb_device.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        subprocess.run([build.HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-o", BIN + ".tmp", SRC],
                       check=True)
        os.replace(BIN + ".tmp", BIN)
    return BIN


def run_index_home(args, stdin=""):
    r = subprocess.run([build_index_home()] + [str(a) for a in args], input=stdin, capture_output=True, text=True,
                       check=True, timeout=120)
    return [int(x) for x in r.stdout.split()]


def group_size():
    return run_index_home(["group"])[0]


def homes(ids, cap):
    """Home entry of every id (Python ints, 128-bit) in an index of `cap` entries."""
    text = "".join("%x %x\n" % (i >> 64, i & U64) for i in ids)
    out = run_index_home(["homes", cap], text)
    assert len(out) == len(ids)
    return out


@pytest.fixture(scope="module")
def G():
    g = group_size()
    assert g in (8, 16)
    return g


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("start", [0, 8, 1024, (1 << 64) - 16, (1 << 128) - 32],
                         ids=["zero", "eight", "1024", "across_2_64", "near_max"])
def test_consecutive_ids_share_a_segment(cap, start, G):
    n = 4 * G  # four aligned groups; across_2_64: the high word changes between the second and third
    assert start % G == 0
    ids = [start + k for k in range(n) if start + k < (1 << 128)]
    h = homes(ids, cap)
    assert all(0 <= x < cap for x in h)
    for g0 in range(0, len(ids), G):
        group = h[g0:g0 + G]
        assert len({x // G for x in group}) == 1, "a group spans segments"
        assert sorted(x % G for x in group) == list(range(len(group))), "slots of a group are not distinct"


@pytest.mark.parametrize("cap", CAPS)
def test_probe_path_is_a_full_cycle_of_one_class(cap, G):
    for start in (0, 5, G - 1, cap // 2 + 3, cap - 1):
        out = run_index_home(["cycle", cap, start])
        steps, path = out[0], out[1:]
        assert steps == cap // G
        assert len(path) == steps + 1 and path[0] == start and path[steps] == start
        assert all(p % G == start % G for p in path), "a probe left its slot class"
        assert sorted(path[:steps]) == list(range(start % G, cap, G)), "a class entry was skipped or repeated"


@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("family", FAMILIES)
def test_skewed_families_fill_classes_and_segments_evenly(family, cap, G):
    n = 1_000_000
    out = run_index_home(["family", family, n, cap])
    classes, empty = out[:G], out[G]
    assert sum(classes) == n
    mean = n / G
    # binomial sd at n / G per class is ~0.26 % of the mean: 2 % is far outside chance and far inside
    # a collapse onto 1 / G of the table
    assert max(abs(c - mean) for c in classes) <= 0.02 * mean, classes
    assert empty <= 16, "%d of %d segments never used" % (empty, cap // G)
