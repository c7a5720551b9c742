"""get_active_accounts' boundary (include/tbgpu.h tbgpu_get_active_accounts): the header's declaration,
constants and structs, the ctypes and numpy mirrors, the symbol the built library exports, and the
Python wrapper's own argument checks.  No GPU."""
import ctypes
import os
import re

import pytest

from tests.conftest import ROOT
from tigerbeetle_amd import _lib
from tigerbeetle_amd import types as T
from tigerbeetle_amd.state_machine import Engine, StateMachine


def test_header_declares_the_constants_the_structs_and_the_call():
    text = open(os.path.join(ROOT, "include", "tbgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+TBGPU_ACTIVE_BY_VOLUME\s+\(1u\s*<<\s*8\)", code)
    assert re.search(r"#define\s+TBGPU_ACTIVE_BY_TRANSFERS\s+\(1u\s*<<\s*9\)", code)
    assert re.search(r"#define\s+TBGPU_ACTIVE_ROWS_MAX\s+8191u\b", code)
    fields_of = lambda name: re.findall(
        r"(\w+)(?:\[(\d+)\])?\s*[,;]",
        re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), code, flags=re.S).group(1))
    assert fields_of("tbgpu_activity_filter") == [
        ("t_open", ""), ("t_close", ""), ("id_min_lo", ""), ("id_min_hi", ""), ("ledger", ""), ("code", ""), ("reserved0", "2"),
        ("limit", ""), ("flags", ""), ("reserved", "16")]
    assert fields_of("tbgpu_account_activity") == [("id_lo", ""), ("id_hi", ""), ("debits", ""), ("credits", "")]
    assert re.search(r"\bint\s+tbgpu_get_active_accounts\s*\(\s*tbgpu_t\s*\*\s*engine\s*,"
                     r"\s*const\s+tbgpu_activity_filter\s*\*\s*filter\s*,\s*void\s*\*\s*out\s*,"
                     r"\s*uint32_t\s+out_cap_rows\s*,\s*tbgpu_query_result\s*\*\s*result\s*\)\s*;", code)
    # The specification is restated in the header's comment.
    comment = re.search(r"/\* get_active_accounts:.*?\*/", text, flags=re.S).group(0)
    for phrase in ("modulo 2^128", "TBGPU_STATUS_INVALID", "tbgpu_get_account_statements", "tbgpu_get_account_counterparties",
                   "id_min = the last", "equal volumes by x ascending", "equal counts by x ascending", "No account table is read",
                   "never a partial answer", "whether or not its groups are returned", "added before any order is applied",
                   "Statement identity", "Counterparty identity", "Double entry", "Ledger identity", "both BY_* bits",
                   "r.ledger == ledger when", "r.code == code when", "feeds both halves of one row"):
        assert phrase in comment, phrase


def test_the_structs_are_64_and_128_bytes_in_every_mirror():
    f, flow, row = _lib.tbgpu_activity_filter, _lib.tbgpu_counterparty_flow, _lib.tbgpu_account_activity
    assert ctypes.sizeof(f) == 64 == T.ACTIVITY_FILTER_DTYPE.itemsize
    assert ctypes.sizeof(row) == 128 == T.ACCOUNT_ACTIVITY_DTYPE.itemsize
    assert [(name, getattr(f, name).offset) for name, _ in f._fields_] == [
        ("t_open", 0), ("t_close", 8), ("id_min_lo", 16), ("id_min_hi", 24), ("ledger", 32), ("code", 36), ("reserved0", 38),
        ("limit", 40), ("flags", 44), ("reserved", 48)]
    assert [(name, getattr(row, name).offset) for name, _ in row._fields_] == [("id_lo", 0), ("id_hi", 8), ("debits", 16), ("credits", 72)]
    # The numpy fields sit where the C fields do.
    for name, _ in f._fields_:
        assert T.ACTIVITY_FILTER_DTYPE.fields[name][1] == getattr(f, name).offset, name
    for half, base in (("debits", 16), ("credits", 72)):
        for name, _ in flow._fields_:
            first = name if name == "transfers" else name + "_lo"
            assert T.ACCOUNT_ACTIVITY_DTYPE.fields[half + "_" + first][1] == base + getattr(flow, name).offset
            if name != "transfers":
                assert T.ACCOUNT_ACTIVITY_DTYPE.fields[half + "_" + name + "_hi"][1] == base + getattr(flow, name).offset + 8
    assert T.ACCOUNT_ACTIVITY_DTYPE.fields["id_lo"][1] == 0 and T.ACCOUNT_ACTIVITY_DTYPE.fields["id_hi"][1] == 8
    assert _lib.ACTIVE_ROWS_MAX == T.ACTIVE_ROWS_MAX == Engine.ACTIVE_ROWS_MAX == 8191
    assert _lib.ACTIVE_BY_VOLUME == T.ACTIVE_BY_VOLUME == 1 << 8 and _lib.ACTIVE_BY_TRANSFERS == T.ACTIVE_BY_TRANSFERS == 1 << 9
    assert (T.FILTER_DEBITS, T.FILTER_CREDITS) == (1, 2)


def test_the_packer_fills_the_filter():
    b = T.pack_activity_filter(11, 13, (17 << 64) | 19, 7, 12, 23, T.FILTER_CREDITS | T.ACTIVE_BY_TRANSFERS)
    f = _lib.tbgpu_activity_filter.from_buffer_copy(b)
    assert (f.t_open, f.t_close, f.id_min_lo, f.id_min_hi, f.ledger, f.code, f.limit, f.flags) == (11, 13, 19, 17, 7, 12, 23, 2 | 512)
    assert bytes(f.reserved0) == bytes(2) and bytes(f.reserved) == bytes(16)
    d = _lib.tbgpu_activity_filter.from_buffer_copy(T.pack_activity_filter())
    assert (d.limit, d.flags, d.t_open, d.t_close, d.id_min_lo, d.id_min_hi, d.ledger, d.code) == (8191, 3, 0, 0, 0, 0, 0, 0)


def test_signatures_list_the_call_and_the_library_exports_it():
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    ret, args = sigs["tbgpu_get_active_accounts"]
    c = _lib.ctypes
    assert ret is c.c_int
    assert args == [c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint32, c.POINTER(_lib.tbgpu_query_result)]
    lib = ctypes.CDLL(_lib.LIB_PATH)  # the built library itself
    assert hasattr(lib, "tbgpu_get_active_accounts")


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library (%s)" % name)


def test_wrapper_checks_its_arguments_before_the_library():
    engine = Engine.__new__(Engine)
    engine.lib, engine.h = NoLibrary(), None
    with pytest.raises(ValueError):
        engine.get_active_accounts_raw(bytes(63))
    with pytest.raises(ValueError):
        engine.get_active_accounts(out_cap_rows=1 << 32)
    with pytest.raises(ValueError):
        engine.get_active_accounts(by="amount")
    with pytest.raises(AssertionError):  # a well-formed request reaches the library
        engine.get_active_accounts(3, 5, ledger=7, code=12, by="transfers", limit=10)
    with pytest.raises(AssertionError):
        engine.top_accounts(3, 5, 10)
    assert callable(StateMachine.get_active_accounts) and callable(StateMachine.top_accounts)
