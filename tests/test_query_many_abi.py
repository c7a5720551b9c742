"""The batched account-filter query's boundary (include/tbgpu.h tbgpu_get_account_transfers_many): the
header's declaration and constant, the ctypes mirror, the bench hook, and the Python wrapper's own
argument checks.  No GPU."""
import os
import re

import pytest

from tests.conftest import ROOT
from tigerbeetle_amd import _lib
from tigerbeetle_amd.state_machine import Engine, StateMachine


def code_of(path):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", path)).read(), flags=re.S)


def test_header_declares_the_batched_query():
    code = code_of("tbgpu.h")
    assert re.search(r"#define\s+TBGPU_QUERY_FILTERS_MAX\s+64u\b", code)
    assert re.search(r"\bint\s+tbgpu_get_account_transfers_many\s*\(\s*tbgpu_t\s*\*\s*\w+\s*,\s*const\s+tbgpu_account_filter\s*\*"
                     r"\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*void\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*tbgpu_query_result\s*\*", code)
    assert re.search(r"\bint\s+tbgpu_bench_query_many_tiles\s*\(\s*tbgpu_t\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*\)", code_of("tbgpu_bench.h"))


def test_signatures_list_the_batched_query():
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    ret, args = sigs["tbgpu_get_account_transfers_many"]
    assert ret is _lib.ctypes.c_int and len(args) == 6
    assert args[2] is _lib.ctypes.c_uint32 and args[4] is _lib.ctypes.c_uint32
    assert "tbgpu_bench_query_many_tiles" in sigs
    assert Engine.FILTERS_MAX == 64


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library (%s)" % name)


def test_wrapper_checks_its_arguments_before_the_library():
    engine = Engine.__new__(Engine)
    engine.lib, engine.h = NoLibrary(), None
    good = Engine.account_filter(1)
    assert len(good) == 64
    with pytest.raises(ValueError):
        engine.get_account_transfers_many([good, good[:63]])
    with pytest.raises(ValueError):
        engine.get_account_transfers_many([good + b"\0"])
    with pytest.raises(ValueError):
        engine.get_account_transfers_many([good] * 65)
    assert engine.get_account_transfers_many([]) == []
    assert callable(StateMachine.get_account_transfers_many)
