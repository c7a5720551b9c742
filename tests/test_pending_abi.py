"""get_pending_transfers' boundary (include/tbgpu.h tbgpu_get_pending_transfers): the header's
declaration and constants, the ctypes and numpy mirrors, and the Python wrapper's own argument checks.
No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT
from tigerbeetle_amd import _lib, types
from tigerbeetle_amd.state_machine import Engine, StateMachine


def test_header_declares_the_call():
    text = open(os.path.join(ROOT, "include", "tbgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, bit in (("OPEN", 4), ("EXPIRED", 5), ("POSTED", 6), ("VOIDED", 7)):
        assert re.search(r"#define\s+TBGPU_PENDING_%s\s+\(1u\s*<<\s*%d\)" % (name, bit), code)
    assert re.search(r"#define\s+TBGPU_PENDING_ROWS_MAX\s+4095u\b", code)
    assert re.search(r"\bint\s+tbgpu_get_pending_transfers\s*\(\s*tbgpu_t\s*\*\s*engine\s*,\s*const\s+tbgpu_pending_filter\s*\*\s*filter\s*,"
                     r"\s*void\s*\*\s*out_rows\s*,\s*uint8_t\s*\*\s*out_states\s*,\s*uint32_t\s+out_cap_rows\s*,\s*tbgpu_query_result\s*\*"
                     r"\s*result\s*\)\s*;", code)
    assert re.search(r"typedef\s+struct\s+tbgpu_pending_filter\s*\{\s*uint64_t\s+account_id_lo\s*,\s*account_id_hi\s*;\s*uint64_t\s+"
                     r"timestamp_min\s*,\s*timestamp_max\s*;\s*uint64_t\s+now\s*;\s*uint32_t\s+limit\s*;\s*uint32_t\s+flags\s*;\s*uint8_t\s+"
                     r"reserved\s*\[\s*16\s*\]\s*;\s*\}\s*tbgpu_pending_filter\s*;", code)
    assert re.search(r"typedef\s+struct\s+tbgpu_pending_row\s*\{\s*uint8_t\s+pending\s*\[\s*128\s*\]\s*;\s*uint8_t\s+resolution\s*\[\s*128\s*\]"
                     r"\s*;\s*\}\s*tbgpu_pending_row\s*;", code)
    # The side and direction bits are the account filter's.
    assert (types.FILTER_DEBITS, types.FILTER_CREDITS, types.FILTER_REVERSED) == (1, 2, 4)


def test_the_filter_is_64_bytes_and_a_row_256():
    assert ctypes.sizeof(_lib.tbgpu_pending_filter) == 64 and ctypes.sizeof(_lib.tbgpu_pending_row) == 256
    assert types.PENDING_FILTER_DTYPE.itemsize == 64 and types.PENDING_ROW_DTYPE.itemsize == 256
    offsets = dict(account_id_lo=0, account_id_hi=8, timestamp_min=16, timestamp_max=24, now=32, limit=40, flags=44, reserved=48)
    for name, _ in _lib.tbgpu_pending_filter._fields_:
        assert getattr(_lib.tbgpu_pending_filter, name).offset == types.PENDING_FILTER_DTYPE.fields[name][1] == offsets[name]
    assert _lib.tbgpu_pending_row.pending.offset == types.PENDING_ROW_DTYPE.fields["pending"][1] == 0
    assert _lib.tbgpu_pending_row.resolution.offset == types.PENDING_ROW_DTYPE.fields["resolution"][1] == 128
    assert types.PENDING_ROW_DTYPE.fields["pending"][0] == types.TRANSFER_DTYPE == types.PENDING_ROW_DTYPE.fields["resolution"][0]
    assert (types.PENDING_OPEN, types.PENDING_EXPIRED, types.PENDING_POSTED, types.PENDING_VOIDED) == (16, 32, 64, 128)
    assert types.PENDING_STATES == 0xF0


def test_signatures_list_the_call():
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    ret, args = sigs["tbgpu_get_pending_transfers"]
    c = _lib.ctypes
    assert ret is c.c_int
    assert args[:5] == [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint32]
    assert args[5] == c.POINTER(_lib.tbgpu_query_result) and len(args) == 6
    assert Engine.PENDING_ROWS_MAX == types.PENDING_ROWS_MAX == _lib.PENDING_ROWS_MAX == 4095
    assert 4095 * 256 <= 8191 * 128  # the rows of one reply fit one message body


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library (%s)" % name)


def test_wrapper_checks_its_arguments_before_the_library():
    engine = Engine.__new__(Engine)
    engine.lib, engine.h = NoLibrary(), None
    with pytest.raises(ValueError):
        engine.get_pending_transfers(1 << 128)
    with pytest.raises(ValueError):
        engine.get_pending_transfers(-1)
    with pytest.raises(ValueError):
        engine.get_pending_transfers(states=types.PENDING_OPEN | 1)
    with pytest.raises(ValueError):
        engine.get_pending_transfers(states=1 << 8)
    with pytest.raises(ValueError):
        engine.get_pending_transfers(now=1 << 64)
    with pytest.raises(ValueError):
        engine.get_pending_transfers(timestamp_min=-1)
    with pytest.raises(ValueError):
        engine.get_pending_transfers(limit=1 << 32)
    with pytest.raises(ValueError):
        engine.get_pending_transfers_raw(bytes(63))
    with pytest.raises(ValueError):
        engine.get_pending_transfers_raw(bytes(128))
    with pytest.raises(ValueError):
        engine.get_pending_transfers_raw(Engine.pending_filter(), -1)
    f = np.frombuffer(Engine.pending_filter(5, types.PENDING_OPEN, debits=False, reversed=True, timestamp_min=7, timestamp_max=9,
                                            now=11, limit=13), dtype=types.PENDING_FILTER_DTYPE)[0]
    assert (int(f["account_id_lo"]), int(f["timestamp_min"]), int(f["timestamp_max"]), int(f["now"]), int(f["limit"])) == (5, 7, 9, 11, 13)
    assert int(f["flags"]) == types.PENDING_OPEN | types.FILTER_CREDITS | types.FILTER_REVERSED and not f["reserved"].any()
    with pytest.raises(AssertionError):  # a well-formed request reaches the library
        engine.get_pending_transfers()
    with pytest.raises(AssertionError):
        engine.get_pending_transfers((1 << 128) - 1, states=0, limit=0)  # invalid filters are the library's to answer
    assert callable(StateMachine.get_pending_transfers)
