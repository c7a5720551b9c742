"""lookup_accounts_at's boundary (include/tbgpu.h tbgpu_lookup_accounts_at): the header's declaration
and constant, the ctypes mirror, and the Python wrapper's own argument checks.  No GPU."""
import os
import re

import pytest

from tests.conftest import ROOT
from tigerbeetle_amd import _lib
from tigerbeetle_amd.state_machine import Engine, StateMachine


def test_header_declares_the_call():
    text = open(os.path.join(ROOT, "include", "tbgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+TBGPU_LOOKUP_AT_MAX\s+8191u\b", code)
    assert re.search(r"\bint\s+tbgpu_lookup_accounts_at\s*\(\s*tbgpu_t\s*\*\s*engine\s*,\s*uint64_t\s+timestamp\s*,\s*const\s+void\s*\*"
                     r"\s*ids\s*,\s*uint32_t\s+n\s*,\s*void\s*\*\s*out\s*,\s*uint32_t\s+out_cap_records\s*,\s*tbgpu_query_result\s*\*"
                     r"\s*result\s*\)\s*;", code)


def test_signatures_list_the_call():
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    ret, args = sigs["tbgpu_lookup_accounts_at"]
    c = _lib.ctypes
    assert ret is c.c_int
    assert args[:6] == [c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint32, c.c_void_p, c.c_uint32]
    assert args[6] == c.POINTER(_lib.tbgpu_query_result) and len(args) == 7
    assert Engine.LOOKUP_AT_MAX == 8191


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library (%s)" % name)


def test_wrapper_checks_its_arguments_before_the_library():
    engine = Engine.__new__(Engine)
    engine.lib, engine.h = NoLibrary(), None
    with pytest.raises(ValueError):
        engine.lookup_accounts_at(range(1, 8193), 5)
    with pytest.raises(ValueError):
        engine.lookup_accounts_at_raw(bytes(16 * 8192), 5)
    with pytest.raises(ValueError):
        engine.lookup_accounts_at_raw(bytes(17), 5)
    with pytest.raises(ValueError):
        engine.lookup_accounts_at_raw(bytes(15), 0)
    empty = engine.lookup_accounts_at([], 5)  # answered without the library, complete like every empty answer
    assert len(empty[0]) == 0 and empty[1:] == (0, True)
    with pytest.raises(AssertionError):  # a well-formed request reaches the library
        engine.lookup_accounts_at([1, 2], 5)
    assert callable(StateMachine.lookup_accounts_at)
