"""get_account_statement_series' boundary (include/tbgpu.h tbgpu_get_account_statement_series): the
header's constant and declaration, the ctypes signature, and the Python wrapper's own argument checks.
No GPU."""
import os
import re

import pytest

from tests.conftest import ROOT
from tigerbeetle_amd import _lib, types
from tigerbeetle_amd.state_machine import Engine, StateMachine
from tigerbeetle_amd.types import STATEMENT_DTYPE


def test_header_declares_the_constant_and_the_call():
    text = open(os.path.join(ROOT, "include", "tbgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+TBGPU_SERIES_ROWS_MAX\s+4095u\b", code)
    assert re.search(r"\bint\s+tbgpu_get_account_statement_series\s*\(\s*tbgpu_t\s*\*\s*engine\s*,\s*const\s+uint64_t\s*\*\s*bounds\s*,"
                     r"\s*uint32_t\s+n_buckets\s*,\s*const\s+void\s*\*\s*ids\s*,\s*uint32_t\s+n\s*,\s*void\s*\*\s*out\s*,"
                     r"\s*uint32_t\s+out_cap_rows\s*,\s*tbgpu_query_result\s*\*\s*result\s*\)\s*;", code)
    # The rows are the statements call's struct: no second one.
    assert len(re.findall(r"typedef\s+struct\s+tbgpu_account_statement\b", code)) == 1


def test_constants_agree():
    assert _lib.SERIES_ROWS_MAX == types.SERIES_ROWS_MAX == Engine.SERIES_ROWS_MAX == 4095


def test_signatures_list_the_call():
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    ret, args = sigs["tbgpu_get_account_statement_series"]
    c = _lib.ctypes
    assert ret is c.c_int
    assert args[:7] == [c.c_void_p, c.c_void_p, c.c_uint32, c.c_void_p, c.c_uint32, c.c_void_p, c.c_uint32]
    assert args[7] == c.POINTER(_lib.tbgpu_query_result) and len(args) == 8


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library (%s)" % name)


def test_wrapper_checks_its_arguments_before_the_library():
    engine = Engine.__new__(Engine)
    engine.lib, engine.h = NoLibrary(), None
    with pytest.raises(ValueError):  # 4,096 rows
        engine.get_account_statement_series(range(1, 65), range(1, 66))
    with pytest.raises(ValueError):
        engine.get_account_statement_series(range(1, 4097), [0, 0])
    with pytest.raises(ValueError):
        engine.get_account_statement_series([1], range(1, 4098))
    with pytest.raises(ValueError):
        engine.get_account_statement_series_raw(bytes(16 * 2048), [1, 2, 3])
    with pytest.raises(ValueError):  # no bucket
        engine.get_account_statement_series([1, 2], [])
    with pytest.raises(ValueError):
        engine.get_account_statement_series([1, 2], [5])
    with pytest.raises(ValueError):
        engine.get_account_statement_series_raw(bytes(32), [5])
    with pytest.raises(ValueError):  # an id is 16 bytes
        engine.get_account_statement_series_raw(bytes(17), [0, 5])
    with pytest.raises(ValueError):
        engine.get_account_statement_series_raw(bytes(15), [5, 0])
    with pytest.raises(ValueError):  # a bound is 64 bits
        engine.get_account_statement_series([1], [0, 1 << 64])
    empty = engine.get_account_statement_series([], [3, 5, 9])  # answered without the library
    assert len(empty[0]) == 0 and empty[0].dtype == STATEMENT_DTYPE and empty[1:] == (0, True)
    for ids, bounds in (([1, 2], [3, 5]), (range(1, 4096), [0, 0]), ([7], range(1, 4097)), (range(1, 64), range(1, 67)),
                        (range(1, 586), range(1, 9))):
        with pytest.raises(AssertionError):  # a well-formed request reaches the library
            engine.get_account_statement_series(ids, bounds)
    assert callable(StateMachine.get_account_statement_series)
