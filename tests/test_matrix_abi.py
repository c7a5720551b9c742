"""get_account_flow_matrix's boundary (include/tbgpu.h tbgpu_get_account_flow_matrix): the header's
declaration, constant and struct, the ctypes and numpy mirrors, and the Python wrapper's own argument
checks.  No GPU."""
import ctypes
import os
import re

import pytest

from tests.conftest import ROOT
from tigerbeetle_amd import _lib
from tigerbeetle_amd.state_machine import Engine, StateMachine, net_positions
from tigerbeetle_amd.types import FLOW_CELL_DTYPE, FLOW_MATRIX_CELLS_MAX


def test_header_declares_the_constant_the_struct_and_the_call():
    text = open(os.path.join(ROOT, "include", "tbgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+TBGPU_FLOW_MATRIX_CELLS_MAX\s+4095u\b", code)
    struct = re.search(r"typedef\s+struct\s+tbgpu_flow_cell\s*\{(.*?)\}\s*tbgpu_flow_cell\s*;", code, flags=re.S)
    assert struct
    fields = re.findall(r"(\w+)(?:\[(\d+)\])?\s*[,;]", struct.group(1))
    assert fields == [("debit_id_lo", ""), ("debit_id_hi", ""), ("credit_id_lo", ""), ("credit_id_hi", ""), ("posted", "2"),
                      ("pending_in", "2"), ("pending_out", "2"), ("transfers", ""), ("reserved", "")]
    assert re.search(r"\bint\s+tbgpu_get_account_flow_matrix\s*\(\s*tbgpu_t\s*\*\s*engine\s*,\s*uint64_t\s+t_open\s*,"
                     r"\s*uint64_t\s+t_close\s*,\s*const\s+void\s*\*\s*debit_ids\s*,\s*uint32_t\s+n_debit\s*,"
                     r"\s*const\s+void\s*\*\s*credit_ids\s*,\s*uint32_t\s+n_credit\s*,\s*void\s*\*\s*out\s*,"
                     r"\s*uint32_t\s+out_cap_cells\s*,\s*tbgpu_query_result\s*\*\s*result\s*\)\s*;", code)
    # The specification is restated in the header's comment.
    comment = re.search(r"/\* get_account_flow_matrix:.*?\*/", text, flags=re.S).group(0)
    for phrase in ("r * found_credit + q", "modulo 2^128", "TBGPU_STATUS_INVALID", "tbgpu_lookup_accounts_at",
                   "tbgpu_get_account_statements", "computed in 64 bits", "whether or not that cell lies under the cap"):
        assert phrase in comment


def test_the_struct_is_96_bytes_in_every_mirror():
    c = _lib.tbgpu_flow_cell
    assert ctypes.sizeof(c) == 96 == FLOW_CELL_DTYPE.itemsize
    assert [(name, getattr(c, name).offset) for name, _ in c._fields_] == [
        ("debit_id_lo", 0), ("debit_id_hi", 8), ("credit_id_lo", 16), ("credit_id_hi", 24), ("posted", 32), ("pending_in", 48),
        ("pending_out", 64), ("transfers", 80), ("reserved", 88)]
    # The numpy fields sit where the C fields do.
    first = {"posted": "posted_lo", "pending_in": "pending_in_lo", "pending_out": "pending_out_lo"}
    for name, _ in c._fields_:
        assert FLOW_CELL_DTYPE.fields[first.get(name, name)][1] == getattr(c, name).offset, name
    for name in first:
        assert FLOW_CELL_DTYPE.fields[name + "_hi"][1] == getattr(c, name).offset + 8
    assert _lib.FLOW_MATRIX_CELLS_MAX == FLOW_MATRIX_CELLS_MAX == Engine.FLOW_MATRIX_CELLS_MAX == 4095


def test_signatures_list_the_call():
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    ret, args = sigs["tbgpu_get_account_flow_matrix"]
    c = _lib.ctypes
    assert ret is c.c_int
    assert args[:9] == [c.c_void_p, c.c_uint64, c.c_uint64, c.c_void_p, c.c_uint32, c.c_void_p, c.c_uint32, c.c_void_p, c.c_uint32]
    assert args[9] == c.POINTER(_lib.tbgpu_query_result) and len(args) == 10


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library (%s)" % name)


def test_wrapper_checks_its_arguments_before_the_library():
    engine = Engine.__new__(Engine)
    engine.lib, engine.h = NoLibrary(), None
    with pytest.raises(ValueError):
        engine.get_account_flow_matrix(range(1, 65), range(1, 65), 0, 0)  # 64 x 64
    with pytest.raises(ValueError):
        engine.get_account_flow_matrix([1], range(1, 4097), 0, 0)  # 1 x 4,096
    with pytest.raises(ValueError):
        engine.get_account_flow_matrix_raw(bytes(16 * 64), bytes(16 * 64), 0, 0)
    with pytest.raises(ValueError):
        engine.get_account_flow_matrix_raw(bytes(17), bytes(16), 0, 5)
    with pytest.raises(ValueError):
        engine.get_account_flow_matrix_raw(bytes(16), bytes(15), 5, 0)
    with pytest.raises(ValueError):
        engine.get_account_flow_matrix([1], [2], 0, 5, out_cap_cells=1 << 32)
    with pytest.raises(ValueError):
        engine.get_account_flow_matrix([1], [2], 1 << 64, 0)
    with pytest.raises(ValueError):
        engine.get_account_flow_matrix([1], [2], 0, -1)
    for debit, credit in (([], [1, 2]), ([1, 2], []), ([], [])):  # answered without the library, complete like every empty answer
        empty = engine.get_account_flow_matrix(debit, credit, 3, 5)
        assert len(empty[0]) == 0 and empty[0].dtype == FLOW_CELL_DTYPE and empty[1:] == (0, True)
    with pytest.raises(AssertionError):  # a well-formed request reaches the library
        engine.get_account_flow_matrix(range(1, 64), range(1, 66), 3, 5)  # 63 x 65
    with pytest.raises(AssertionError):
        engine.get_account_flow_matrix(range(1, 4096), [7], 0, 0)  # 4,095 x 1
    with pytest.raises(AssertionError):
        engine.get_account_flow_matrix_raw(bytes(16), bytes(16 * 4095), 0, 0)
    assert callable(StateMachine.get_account_flow_matrix) and callable(StateMachine.get_account_flow_matrix_raw)
    assert callable(net_positions)
