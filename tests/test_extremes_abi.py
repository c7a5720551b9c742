"""get_account_balance_extremes' boundary (include/tbgpu.h tbgpu_get_account_balance_extremes): the
header's declaration, constants, measure macros and structs, the ctypes and numpy mirrors, and the
Python wrapper's own argument checks; what makes the library itself answer TBGPU_STATUS_INVALID is
listed from the header here and exercised on the device in tests/test_gpu_extremes.py.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT
from tigerbeetle_amd import _lib
from tigerbeetle_amd import types as T
from tigerbeetle_amd.state_machine import Engine, StateMachine
from tigerbeetle_amd.types import EXTREME_DTYPE, EXTREMES_MAX, extreme_value, pack_balance_measure


def header():
    text = open(os.path.join(ROOT, "include", "tbgpu.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_constant_the_structs_and_the_call():
    text, code = header()
    assert re.search(r"#define\s+TBGPU_EXTREMES_MAX\s+4095u\b", code)
    measure = re.search(r"typedef\s+struct\s+tbgpu_balance_measure\s*\{(.*?)\}\s*tbgpu_balance_measure\s*;", code, flags=re.S)
    assert measure and re.findall(r"(\w+)(?:\[(\d+)\])?\s*[,;]", measure.group(1)) == [
        ("debits_pending", ""), ("debits_posted", ""), ("credits_pending", ""), ("credits_posted", ""), ("reserved", "4")]
    assert re.search(r"int8_t\s+debits_pending", measure.group(1)) and re.search(r"uint8_t\s+reserved\[4\]", measure.group(1))
    struct = re.search(r"typedef\s+struct\s+tbgpu_account_balance_extreme\s*\{(.*?)\}\s*tbgpu_account_balance_extreme\s*;", code, flags=re.S)
    assert struct
    fields = re.findall(r"(\w+)(?:\[(\d+)\])?\s*[,;]", struct.group(1))
    assert fields == [("id_lo", ""), ("id_hi", ""), ("opening", "3"), ("closing", "3"), ("low", "3"), ("high", "3"), ("t_low", ""),
                      ("t_high", ""), ("records", ""), ("t_open", ""), ("t_end", ""), ("measure", ""), ("reserved", "4")]
    assert re.search(r"\bint\s+tbgpu_get_account_balance_extremes\s*\(\s*tbgpu_t\s*\*\s*engine\s*,\s*uint64_t\s+t_open\s*,"
                     r"\s*uint64_t\s+t_close\s*,\s*const\s+tbgpu_balance_measure\s*\*\s*measure\s*,\s*const\s+void\s*\*\s*ids\s*,"
                     r"\s*uint32_t\s+n\s*,\s*void\s*\*\s*out\s*,\s*uint32_t\s+out_cap_rows\s*,\s*tbgpu_query_result\s*\*\s*result\s*\)\s*;",
                     code)
    # The specification is restated in the header's comment, every INVALID rule and the cost of the exact path with it.
    comment = re.search(r"/\* get_account_balance_extremes:.*?\*/", text, flags=re.S).group(0)
    for phrase in ("tbgpu_lookup_accounts_at", "commit_timestamp", "first i that reaches it", "A post is one step", "below 2^130",
                   "A coefficient outside {-1, 0, +1}", "a measure that is all zero", "a non-zero reserved byte", "NULL\n *     measure, ids, out or result",
                   "n > TBGPU_EXTREMES_MAX is TBGPU_STATUS_INVALID", "writes nothing", "A node\n *     engine", "slowly"):
        assert phrase in comment, phrase


def test_measure_macros_match_the_python_tuples():
    _, code = header()
    macros = dict(re.findall(r"#define\s+TBGPU_MEASURE_(\w+)\s+\{\s*([-+\d\s,]+?),\s*\{0, 0, 0, 0\}\}", code))
    assert len(macros) == 8
    for name, body in macros.items():
        assert tuple(int(v) for v in body.split(",")) == getattr(T, "MEASURE_" + name), name
    assert T.MEASURE_CREDIT_NET_POSTED == (0, -1, 0, 1) and T.MEASURE_CREDIT_AVAILABLE == (-1, -1, 0, 1)
    singles = [T.MEASURE_DEBITS_PENDING, T.MEASURE_DEBITS_POSTED, T.MEASURE_CREDITS_PENDING, T.MEASURE_CREDITS_POSTED]
    assert singles == [tuple(int(i == k) for i in range(4)) for k in range(4)]


def test_the_row_is_192_bytes_and_the_measure_8_in_every_mirror():
    c = _lib.tbgpu_account_balance_extreme
    assert ctypes.sizeof(c) == 192 == EXTREME_DTYPE.itemsize
    assert [(name, getattr(c, name).offset) for name, _ in c._fields_] == [
        ("id_lo", 0), ("id_hi", 8), ("opening", 16), ("closing", 40), ("low", 64), ("high", 88), ("t_low", 112), ("t_high", 120),
        ("records", 128), ("t_open", 136), ("t_end", 144), ("measure", 152), ("reserved", 160)]
    first = {v: v + "_w0" for v in ("opening", "closing", "low", "high")}
    for name, _ in c._fields_:
        assert EXTREME_DTYPE.fields[first.get(name, name)][1] == getattr(c, name).offset, name
    assert EXTREME_DTYPE.fields["high_w2"][1] == 88 + 16
    m = _lib.tbgpu_balance_measure
    assert ctypes.sizeof(m) == 8 == len(pack_balance_measure(T.MEASURE_CREDIT_AVAILABLE))
    assert [(name, getattr(m, name).offset) for name, _ in m._fields_] == [
        ("debits_pending", 0), ("debits_posted", 1), ("credits_pending", 2), ("credits_posted", 3), ("reserved", 4)]
    assert pack_balance_measure((-1, -1, 0, 1)) == b"\xff\xff\x00\x01\x00\x00\x00\x00"
    assert bytes(m(-1, -1, 0, 1)) == pack_balance_measure((-1, -1, 0, 1))
    assert _lib.EXTREMES_MAX == EXTREMES_MAX == Engine.EXTREMES_MAX == 4095


def test_signatures_list_the_call():
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    ret, args = sigs["tbgpu_get_account_balance_extremes"]
    c = _lib.ctypes
    assert ret is c.c_int
    assert args[:8] == [c.c_void_p, c.c_uint64, c.c_uint64, c.c_void_p, c.c_void_p, c.c_uint32, c.c_void_p, c.c_uint32]
    assert args[8] == c.POINTER(_lib.tbgpu_query_result) and len(args) == 9


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library (%s)" % name)


def test_wrapper_checks_its_arguments_before_the_library():
    engine = Engine.__new__(Engine)
    engine.lib, engine.h = NoLibrary(), None
    net = T.MEASURE_CREDIT_NET_POSTED
    with pytest.raises(ValueError):
        engine.get_account_balance_extremes(range(1, 4097), 0, 0, net)
    with pytest.raises(ValueError):
        engine.get_account_balance_extremes_raw(bytes(16 * 4096), 0, 0, pack_balance_measure(net))
    with pytest.raises(ValueError):
        engine.get_account_balance_extremes_raw(bytes(17), 0, 5, pack_balance_measure(net))
    with pytest.raises(ValueError):
        engine.get_account_balance_extremes_raw(bytes(16), 0, 5, bytes(7))  # a measure is 8 bytes
    with pytest.raises(ValueError):
        engine.get_account_balance_extremes([1], 0, 5, (0, 1, 0))  # ... of four coefficients
    with pytest.raises(ValueError):
        engine.get_account_balance_extremes([1], 0, 5, (0, 200, 0, 0))  # ... each a signed byte
    with pytest.raises(ValueError):
        engine.get_account_balance_extremes([1], 0, 5, net, out_cap_rows=1 << 32)
    empty = engine.get_account_balance_extremes([], 3, 5, net)  # answered without the library, complete like every empty answer
    assert len(empty[0]) == 0 and empty[0].dtype == EXTREME_DTYPE and empty[1:] == (0, True)
    # What only the library judges reaches it: a coefficient of 2, a measure of no column, a reserved byte.
    for measure_bytes in (pack_balance_measure((2, 0, 0, 0)), pack_balance_measure((0, 0, 0, 0)), pack_balance_measure(net, b"\0\0\1\0")):
        with pytest.raises(AssertionError):
            engine.get_account_balance_extremes_raw(bytes(16), 3, 5, measure_bytes)
    with pytest.raises(AssertionError):
        engine.get_account_balance_extremes(range(1, 4096), 0, 0, net)
    assert callable(StateMachine.get_account_balance_extremes)


def test_extreme_value_reads_a_signed_192_bit_field():
    row = np.zeros(1, dtype=EXTREME_DTYPE)[0]
    for name, v in (("opening", -1), ("closing", (1 << 191) - 1), ("low", -(1 << 191)), ("high", (1 << 128) + 5)):
        for w in range(3):
            row["%s_w%d" % (name, w)] = ((v % (1 << 192)) >> (64 * w)) & ((1 << 64) - 1)
        assert extreme_value(row, name) == v and type(extreme_value(row, name)) is int
