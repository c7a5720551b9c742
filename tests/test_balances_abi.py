"""The balance-history query's boundary (include/tbgpu.h tbgpu_get_account_balances): the row layout
in the ctypes and numpy mirrors, and the header's declarations.  No GPU."""
import ctypes
import os
import re

from tests.conftest import ROOT
from tigerbeetle_amd import _lib, types

WORDS = ("debits_pending_lo", "debits_pending_hi", "debits_posted_lo", "debits_posted_hi", "credits_pending_lo",
         "credits_pending_hi", "credits_posted_lo", "credits_posted_hi", "timestamp")


def test_row_size_and_offsets():
    B = _lib.tbgpu_account_balance
    assert ctypes.sizeof(B) == 128
    assert [getattr(B, n).offset for n in WORDS] == [8 * i for i in range(9)]
    assert B.reserved.offset == 72 and B.reserved.size == 56


def test_numpy_row_matches_ctypes():
    D = types.ACCOUNT_BALANCE_DTYPE
    assert D.itemsize == 128
    assert [n for n, _ in _lib.tbgpu_account_balance._fields_] == list(D.names)
    for name, _ in _lib.tbgpu_account_balance._fields_:
        assert D.fields[name][1] == getattr(_lib.tbgpu_account_balance, name).offset, name
        assert D.fields[name][0].itemsize == getattr(_lib.tbgpu_account_balance, name).size, name


def test_header_declares_the_query():
    text = open(os.path.join(ROOT, "include", "tbgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+tbgpu_get_account_balances\s*\(\s*tbgpu_t\s*\*\s*engine\s*,\s*const\s+tbgpu_account_filter\s*\*", code)
    struct = re.search(r"typedef\s+struct\s+tbgpu_account_balance\s*\{(.*?)\}\s*tbgpu_account_balance\s*;", code, flags=re.S)
    assert struct
    declared = re.findall(r"\b(\w+)\s*(?:\[\s*56\s*\])?\s*[,;]", struct.group(1))
    assert declared == list(WORDS) + ["reserved"]
    signature = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert signature["tbgpu_get_account_balances"] == signature["tbgpu_get_account_transfers"]
