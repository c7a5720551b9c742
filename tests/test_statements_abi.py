"""get_account_statements' boundary (include/tbgpu.h tbgpu_get_account_statements): the header's
declaration, constant and struct, the ctypes and numpy mirrors, and the Python wrapper's own argument
checks.  No GPU."""
import ctypes
import os
import re

import pytest

from tests.conftest import ROOT
from tigerbeetle_amd import _lib
from tigerbeetle_amd.state_machine import Engine, StateMachine
from tigerbeetle_amd.types import STATEMENT_DTYPE, STATEMENTS_MAX


def test_header_declares_the_constant_the_struct_and_the_call():
    text = open(os.path.join(ROOT, "include", "tbgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+TBGPU_STATEMENTS_MAX\s+4095u\b", code)
    struct = re.search(r"typedef\s+struct\s+tbgpu_account_statement\s*\{(.*?)\}\s*tbgpu_account_statement\s*;", code, flags=re.S)
    assert struct
    fields = re.findall(r"(\w+)(?:\[(\d+)\])?\s*[,;]", struct.group(1))
    assert fields == [("id_lo", ""), ("id_hi", ""), ("opening", "8"), ("closing", "8"), ("debits_pending_in", "2"),
                      ("debits_pending_out", "2"), ("debits_posted_in", "2"), ("credits_pending_in", "2"),
                      ("credits_pending_out", "2"), ("credits_posted_in", "2"), ("debit_transfers", ""), ("credit_transfers", "")]
    assert re.search(r"\bint\s+tbgpu_get_account_statements\s*\(\s*tbgpu_t\s*\*\s*engine\s*,\s*uint64_t\s+t_open\s*,\s*uint64_t\s+t_close\s*,"
                     r"\s*const\s+void\s*\*\s*ids\s*,\s*uint32_t\s+n\s*,\s*void\s*\*\s*out\s*,\s*uint32_t\s+out_cap_rows\s*,"
                     r"\s*tbgpu_query_result\s*\*\s*result\s*\)\s*;", code)


def test_the_struct_is_256_bytes_in_every_mirror():
    assert ctypes.sizeof(_lib.tbgpu_account_statement) == 256 == STATEMENT_DTYPE.itemsize
    # The numpy fields sit where the C fields do.
    for name, _ in _lib.tbgpu_account_statement._fields_:
        at = getattr(_lib.tbgpu_account_statement, name).offset
        first = {"opening": "opening_debits_pending_lo", "closing": "closing_debits_pending_lo", "id_lo": "id_lo", "id_hi": "id_hi",
                 "debit_transfers": "debit_transfers", "credit_transfers": "credit_transfers"}.get(name, name + "_lo")
        assert STATEMENT_DTYPE.fields[first][1] == at, name
    assert STATEMENT_DTYPE.fields["closing_credits_posted_hi"][1] == 16 + 64 + 56
    assert _lib.STATEMENTS_MAX == STATEMENTS_MAX == Engine.STATEMENTS_MAX == 4095


def test_signatures_list_the_call():
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    ret, args = sigs["tbgpu_get_account_statements"]
    c = _lib.ctypes
    assert ret is c.c_int
    assert args[:7] == [c.c_void_p, c.c_uint64, c.c_uint64, c.c_void_p, c.c_uint32, c.c_void_p, c.c_uint32]
    assert args[7] == c.POINTER(_lib.tbgpu_query_result) and len(args) == 8


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library (%s)" % name)


def test_wrapper_checks_its_arguments_before_the_library():
    engine = Engine.__new__(Engine)
    engine.lib, engine.h = NoLibrary(), None
    with pytest.raises(ValueError):
        engine.get_account_statements(range(1, 4097), 0, 0)
    with pytest.raises(ValueError):
        engine.get_account_statements_raw(bytes(16 * 4096), 0, 0)
    with pytest.raises(ValueError):
        engine.get_account_statements_raw(bytes(17), 0, 5)
    with pytest.raises(ValueError):
        engine.get_account_statements_raw(bytes(15), 5, 0)
    empty = engine.get_account_statements([], 3, 5)  # answered without the library, complete like every empty answer
    assert len(empty[0]) == 0 and empty[0].dtype == STATEMENT_DTYPE and empty[1:] == (0, True)
    with pytest.raises(AssertionError):  # a well-formed request reaches the library
        engine.get_account_statements([1, 2], 3, 5)
    with pytest.raises(AssertionError):
        engine.get_account_statements(range(1, 4096), 0, 0)
    assert callable(StateMachine.get_account_statements)
