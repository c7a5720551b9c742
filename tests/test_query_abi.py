"""The account-filter query's boundary (include/tbgpu.h tbgpu_get_account_transfers): the filter and
result layouts in the ctypes and numpy mirrors, and the header's declaration.  No GPU."""
import ctypes
import os
import re

from tests.conftest import ROOT
from tigerbeetle_amd import _lib, types


def test_filter_and_result_sizes():
    assert ctypes.sizeof(_lib.tbgpu_account_filter) == 64
    assert ctypes.sizeof(_lib.tbgpu_query_result) == 16


def test_filter_field_offsets():
    F = _lib.tbgpu_account_filter
    offsets = [getattr(F, n).offset for n in ("account_id_lo", "timestamp_min", "timestamp_max", "limit", "flags",
                                              "reserved")]
    assert offsets == [0, 16, 24, 32, 36, 40]
    assert F.account_id_hi.offset == 8
    R = _lib.tbgpu_query_result
    assert (R.count.offset, R.complete.offset, R.matched.offset) == (0, 4, 8)


def test_numpy_filter_matches_ctypes():
    D = types.ACCOUNT_FILTER_DTYPE
    assert D.itemsize == 64
    for name, _ in _lib.tbgpu_account_filter._fields_:
        assert D.fields[name][1] == getattr(_lib.tbgpu_account_filter, name).offset, name
    assert (types.FILTER_DEBITS, types.FILTER_CREDITS, types.FILTER_REVERSED) == (1, 2, 4)


def test_header_declares_the_query():
    text = open(os.path.join(ROOT, "include", "tbgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+tbgpu_get_account_transfers\s*\(\s*tbgpu_t\s*\*", code)
    for name, bit in (("DEBITS", 0), ("CREDITS", 1), ("REVERSED", 2)):
        assert re.search(r"#define\s+TBGPU_FILTER_%s\s+\(1u << %d\)" % (name, bit), code)
    assert "tbgpu_get_account_transfers" in {n for n, _, _ in _lib.SIGNATURES}
    bench = open(os.path.join(ROOT, "include", "tbgpu_bench.h")).read()
    assert "tbgpu_bench_query_keys_max" in re.sub(r"/\*.*?\*/", "", bench, flags=re.S)
