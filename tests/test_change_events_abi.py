"""The change stream's boundary (include/tbgpu.h tbgpu_get_change_events): the filter and event
layouts in the ctypes and numpy mirrors, and the header's declarations.  No GPU."""
import ctypes
import os
import re

from tests.conftest import ROOT
from tigerbeetle_amd import _lib, types


def test_struct_sizes_and_offsets():
    F, E = _lib.tbgpu_change_events_filter, _lib.tbgpu_change_event
    assert ctypes.sizeof(F) == 64 and ctypes.sizeof(E) == 384
    assert (F.timestamp_min.offset, F.timestamp_max.offset, F.limit.offset) == (0, 8, 16)
    assert F.reserved.offset == 20 and F.reserved.size == 44
    assert [(getattr(E, n).offset, getattr(E, n).size) for n in ("transfer", "debit_account", "credit_account")] == [
        (0, 128), (128, 128), (256, 128)]


def test_numpy_matches_ctypes():
    for D, S in ((types.CHANGE_EVENTS_FILTER_DTYPE, _lib.tbgpu_change_events_filter),
                 (types.CHANGE_EVENT_DTYPE, _lib.tbgpu_change_event)):
        assert D.itemsize == ctypes.sizeof(S)
        assert [n for n, _ in S._fields_] == list(D.names)
        for name, _ in S._fields_:
            assert D.fields[name][1] == getattr(S, name).offset, name
            assert D.fields[name][0].itemsize == getattr(S, name).size, name
    E = types.CHANGE_EVENT_DTYPE
    assert E.fields["transfer"][0] == types.TRANSFER_DTYPE
    assert E.fields["debit_account"][0] == types.ACCOUNT_DTYPE and E.fields["credit_account"][0] == types.ACCOUNT_DTYPE
    packed = types.pack_change_events_filter(timestamp_min=5, timestamp_max=9, limit=7)
    f = _lib.tbgpu_change_events_filter.from_buffer_copy(packed)
    assert (f.timestamp_min, f.timestamp_max, f.limit, bytes(f.reserved)) == (5, 9, 7, bytes(44))
    assert types.CHANGE_EVENTS_MAX == _lib.CHANGE_EVENTS_MAX == 2730


def test_header_declares_the_call():
    text = open(os.path.join(ROOT, "include", "tbgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+TBGPU_CHANGE_EVENTS_MAX\s+2730u\b", code)
    assert 2730 * 384 <= 8191 * 128 < 2731 * 384
    assert re.search(r"\bint\s+tbgpu_get_change_events\s*\(\s*tbgpu_t\s*\*\s*engine\s*,\s*const\s+tbgpu_change_events_filter\s*\*"
                     r"\s*filter\s*,\s*void\s*\*\s*out\s*,\s*uint32_t\s+out_cap_events\s*,\s*tbgpu_query_result\s*\*\s*result\s*\)", code)
    flt = re.search(r"typedef\s+struct\s+tbgpu_change_events_filter\s*\{(.*?)\}\s*tbgpu_change_events_filter\s*;", code, flags=re.S)
    ev = re.search(r"typedef\s+struct\s+tbgpu_change_event\s*\{(.*?)\}\s*tbgpu_change_event\s*;", code, flags=re.S)
    assert flt and ev
    assert re.findall(r"\b(\w+)\s*(?:\[\s*\d+\s*\])?\s*;", flt.group(1)) == ["timestamp_min", "timestamp_max", "limit", "reserved"]
    assert re.findall(r"\b(\w+)\s*\[\s*128\s*\]\s*;", ev.group(1)) == ["transfer", "debit_account", "credit_account"]
    signature = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    assert signature["tbgpu_get_change_events"] == signature["tbgpu_query_transfers"]
