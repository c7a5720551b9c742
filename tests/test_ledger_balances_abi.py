"""get_ledger_balances' boundary (include/tbgpu.h tbgpu_get_ledger_balances): the header's declaration
and constant, the ctypes mirror, and the Python wrapper's own argument checks.  No GPU."""
import ctypes
import os
import re

import pytest

from tests.conftest import ROOT
from tigerbeetle_amd import _lib, types
from tigerbeetle_amd.state_machine import Engine, StateMachine


def test_header_declares_the_call():
    text = open(os.path.join(ROOT, "include", "tbgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+TBGPU_LEDGERS_MAX\s+1024u\b", code)
    assert re.search(r"\bint\s+tbgpu_get_ledger_balances\s*\(\s*tbgpu_t\s*\*\s*engine\s*,\s*uint64_t\s+timestamp\s*,\s*const\s+uint32_t\s*\*"
                     r"\s*ledgers\s*,\s*uint32_t\s+n\s*,\s*void\s*\*\s*out\s*,\s*uint32_t\s+out_cap_rows\s*,\s*tbgpu_query_result\s*\*"
                     r"\s*result\s*\)\s*;", code)
    assert re.search(r"typedef\s+struct\s+tbgpu_ledger_balance\s*\{[^}]*uint64_t\s+accounts\s*;\s*uint32_t\s+ledger\s*;\s*uint8_t\s+"
                     r"reserved\s*\[\s*52\s*\]\s*;\s*\}\s*tbgpu_ledger_balance\s*;", code)


def test_the_row_is_128_bytes():
    assert ctypes.sizeof(_lib.tbgpu_ledger_balance) == 128
    assert _lib.tbgpu_ledger_balance.ledger.offset == 72 and _lib.tbgpu_ledger_balance.accounts.offset == 64
    assert types.LEDGER_BALANCE_DTYPE.itemsize == 128
    assert types.LEDGER_BALANCE_DTYPE.fields["ledger"][1] == 72 and types.LEDGER_BALANCE_DTYPE.fields["accounts"][1] == 64
    for name, _ in _lib.tbgpu_ledger_balance._fields_:
        assert getattr(_lib.tbgpu_ledger_balance, name).offset == types.LEDGER_BALANCE_DTYPE.fields[name][1]


def test_signatures_list_the_call():
    sigs = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    ret, args = sigs["tbgpu_get_ledger_balances"]
    c = _lib.ctypes
    assert ret is c.c_int
    assert args[:6] == [c.c_void_p, c.c_uint64, c.c_void_p, c.c_uint32, c.c_void_p, c.c_uint32]
    assert args[6] == c.POINTER(_lib.tbgpu_query_result) and len(args) == 7
    assert Engine.LEDGERS_MAX == types.LEDGERS_MAX == _lib.LEDGERS_MAX == 1024


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the wrapper called the library (%s)" % name)


def test_wrapper_checks_its_arguments_before_the_library():
    engine = Engine.__new__(Engine)
    engine.lib, engine.h = NoLibrary(), None
    with pytest.raises(ValueError):
        engine.get_ledger_balances(range(1, 1026), 5)
    with pytest.raises(ValueError):
        engine.get_ledger_balances_raw(bytes(4 * 1025), 5)
    with pytest.raises(ValueError):
        engine.get_ledger_balances([1, 1 << 32], 5)
    with pytest.raises(ValueError):
        engine.get_ledger_balances([-1])
    with pytest.raises(ValueError):
        engine.get_ledger_balances_raw(bytes(6), 5)
    with pytest.raises(ValueError):
        engine.get_ledger_balances_raw(bytes(3))
    empty = engine.get_ledger_balances([], 5)  # answered without the library, complete like every empty answer
    assert len(empty[0]) == 0 and empty[0].dtype == types.LEDGER_BALANCE_DTYPE and empty[1:] == (0, True)
    with pytest.raises(AssertionError):  # a well-formed request reaches the library
        engine.get_ledger_balances([1, 0, (1 << 32) - 1], 5)
    with pytest.raises(AssertionError):
        engine.get_ledger_balances(range(1, 1025))
    assert callable(StateMachine.get_ledger_balances)
