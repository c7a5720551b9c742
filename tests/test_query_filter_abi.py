"""The field-filter queries' boundary (include/tbgpu.h tbgpu_query_transfers / tbgpu_query_accounts): the
filter's layout in the ctypes and numpy mirrors, and the header's declarations.  No GPU."""
import ctypes
import os
import re

from tests.conftest import ROOT
from tigerbeetle_amd import _lib, types

NAMES = ("user_data_128_lo", "user_data_128_hi", "user_data_64", "user_data_32", "ledger", "code", "reserved",
         "timestamp_min", "timestamp_max", "limit", "flags")


def test_filter_size_and_offsets():
    F = _lib.tbgpu_query_filter
    assert ctypes.sizeof(F) == 64
    assert tuple(n for n, _ in F._fields_) == NAMES
    assert [getattr(F, n).offset for n in NAMES] == [0, 8, 16, 24, 28, 32, 34, 40, 48, 56, 60]
    assert F.reserved.size == 6


def test_numpy_filter_matches_ctypes():
    D = types.QUERY_FILTER_DTYPE
    assert D.itemsize == 64 and D.names == NAMES
    for name in NAMES:
        assert D.fields[name][1] == getattr(_lib.tbgpu_query_filter, name).offset, name
        assert D.fields[name][0].itemsize == getattr(_lib.tbgpu_query_filter, name).size, name
    assert types.QUERY_REVERSED == 1


def test_header_declares_the_queries():
    text = open(os.path.join(ROOT, "include", "tbgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for fn in ("tbgpu_query_transfers", "tbgpu_query_accounts"):
        assert re.search(r"\bint\s+%s\s*\(\s*tbgpu_t\s*\*\s*\w*\s*,\s*const\s+tbgpu_query_filter\s*\*" % fn, code), fn
        assert fn in {n for n, _, _ in _lib.SIGNATURES}
    assert re.search(r"#define\s+TBGPU_QUERY_REVERSED\s+\(1u << 0\)", code)
    assert re.search(r"typedef\s+struct\s+tbgpu_query_filter\s*\{", code)
