"""get_account_balance_integrals' boundary (include/tbgpu.h tbgpu_get_account_balance_integrals): the
header's declaration, constant and struct, the ctypes and numpy mirrors, and the Python wrapper's own
argument checks.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT
from tigerbeetle_amd import _lib
from tigerbeetle_amd.state_machine import Engine, StateMachine, average_balances
from tigerbeetle_amd.types import INTEGRAL_DTYPE, INTEGRALS_MAX

COLUMNS = ("debits_pending", "debits_posted", "credits_pending", "credits_posted")


def test_header_declares_the_constant_the_struct_and_the_call():
    text = open(os.path.join(ROOT, "include", "tbgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+TBGPU_INTEGRALS_MAX\s+4095u\b", code)
    struct = re.search(r"typedef\s+struct\s+tbgpu_account_balance_integral\s*\{(.*?)\}\s*tbgpu_account_balance_integral\s*;", code,
                       flags=re.S)
    assert struct
    fields = re.findall(r"(\w+)(?:\[(\d+)\])?\s*[,;]", struct.group(1))
    assert fields == [("id_lo", ""), ("id_hi", ""), ("opening", "8"), ("closing", "8"), ("integral", "12"), ("t_open", ""), ("t_end", "")]
    assert re.search(r"\bint\s+tbgpu_get_account_balance_integrals\s*\(\s*tbgpu_t\s*\*\s*engine\s*,\s*uint64_t\s+t_open\s*,"
                     r"\s*uint64_t\s+t_close\s*,\s*const\s+void\s*\*\s*ids\s*,\s*uint32_t\s+n\s*,\s*void\s*\*\s*out\s*,"
                     r"\s*uint32_t\s+out_cap_rows\s*,\s*tbgpu_query_result\s*\*\s*result\s*\)\s*;", code)
    # The specification is restated in the header's comment.
    comment = re.search(r"/\* get_account_balance_integrals:.*?\*/", text, flags=re.S).group(0)
    for phrase in ("modulo 2^192", "commit_timestamp", "TBGPU_STATUS_INVALID", "tbgpu_lookup_accounts_at"):
        assert phrase in comment


def test_the_struct_is_256_bytes_in_every_mirror():
    c = _lib.tbgpu_account_balance_integral
    assert ctypes.sizeof(c) == 256 == INTEGRAL_DTYPE.itemsize
    assert [(name, getattr(c, name).offset) for name, _ in c._fields_] == [
        ("id_lo", 0), ("id_hi", 8), ("opening", 16), ("closing", 80), ("integral", 144), ("t_open", 240), ("t_end", 248)]
    # The numpy fields sit where the C fields do.
    first = {"opening": "opening_debits_pending_lo", "closing": "closing_debits_pending_lo", "integral": "integral_debits_pending_w0"}
    for name, _ in c._fields_:
        assert INTEGRAL_DTYPE.fields[first.get(name, name)][1] == getattr(c, name).offset, name
    assert INTEGRAL_DTYPE.fields["closing_credits_posted_hi"][1] == 16 + 64 + 56
    for k, column in enumerate(COLUMNS):
        for w in range(3):
            assert INTEGRAL_DTYPE.fields["integral_%s_w%d" % (column, w)][1] == 144 + 24 * k + 8 * w
    assert _lib.INTEGRALS_MAX == INTEGRALS_MAX == Engine.INTEGRALS_MAX == 4095


def test_signatures_list_the_call():
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    ret, args = sigs["tbgpu_get_account_balance_integrals"]
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
        engine.get_account_balance_integrals(range(1, 4097), 0, 0)
    with pytest.raises(ValueError):
        engine.get_account_balance_integrals_raw(bytes(16 * 4096), 0, 0)
    with pytest.raises(ValueError):
        engine.get_account_balance_integrals_raw(bytes(17), 0, 5)
    with pytest.raises(ValueError):
        engine.get_account_balance_integrals_raw(bytes(15), 5, 0)
    with pytest.raises(ValueError):
        engine.get_account_balance_integrals([1], 0, 5, out_cap_rows=1 << 32)
    empty = engine.get_account_balance_integrals([], 3, 5)  # answered without the library, complete like every empty answer
    assert len(empty[0]) == 0 and empty[0].dtype == INTEGRAL_DTYPE and empty[1:] == (0, True)
    with pytest.raises(AssertionError):  # a well-formed request reaches the library
        engine.get_account_balance_integrals([1, 2], 3, 5)
    with pytest.raises(AssertionError):
        engine.get_account_balance_integrals(range(1, 4096), 0, 0)
    assert callable(StateMachine.get_account_balance_integrals)


def test_average_balances_divides_the_three_word_integral_by_the_period():
    row = np.zeros(1, dtype=INTEGRAL_DTYPE)[0]
    row["t_open"], row["t_end"] = 1000, 1000
    assert average_balances(row) is None
    row["t_end"] = 1007
    values = ((1 << 191) + 12345, 6, 7 * ((1 << 128) - 1), (1 << 64) * 7 + 3)
    for column, v in zip(COLUMNS, values):
        for w in range(3):
            row["integral_%s_w%d" % (column, w)] = (v >> (64 * w)) & ((1 << 64) - 1)
    got = average_balances(row)
    assert got == tuple(v // 7 for v in values) and all(type(v) is int for v in got)
    assert got[2] == (1 << 128) - 1 and got[1] == 0
