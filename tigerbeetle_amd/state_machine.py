"""Host-side mirror of the reference's StateMachine plugin interface, backed by the MI355X engine.

The reference's replica drives a comptime duck-typed `StateMachineType`
(src/state_machine.zig:28-1150; the contract is listed in SURVEY.md §8b):

    init(allocator, grid, options) / deinit / reset
    prepare(operation, input)                    -> prepare_timestamp += len(events)   (:336-343)
    prefetch(callback, op, operation, input)     -> async staging of objects          (:345-506)
    commit(client, op, timestamp, operation, input, output) -> reply bytes             (:508-540)
    compact(callback, op) / checkpoint(callback)                                        (:542-582)
    fields prepare_timestamp, commit_timestamp

`StateMachine` below keeps that shape; `commit` crosses into HIP through the C ABI
(include/tbgpu.h).  Objects live in HBM, so `prefetch` completes immediately (its callback fires
synchronously, which the reference allows: src/lsm/groove.zig:723-742).  `checkpoint` hands the
objects changed since the previous checkpoint (tbgpu_checkpoint_delta) to an optional write-back
sink — what a durable replica inserts / upserts into its forest; `compact` has nothing to do.
"""
import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from .types import (ACCOUNT_BALANCE_DTYPE, ACCOUNT_DTYPE, ACCOUNT_FILTER_DTYPE, BATCH_MAX, CHANGE_EVENT_DTYPE, CHANGE_EVENTS_FILTER_DTYPE,
                    CHANGE_EVENTS_MAX, LEDGER_BALANCE_DTYPE, LEDGERS_MAX, PENDING_FILTER_DTYPE, PENDING_ROW_DTYPE, PENDING_ROWS_MAX, PENDING_STATES, STATEMENT_DTYPE, INTEGRAL_DTYPE, EXTREME_DTYPE, pack_balance_measure, FLOW_CELL_DTYPE, COUNTERPARTY_DTYPE, COUNTERPARTIES_BY_VOLUME, COUNTERPARTIES_ROWS_MAX, pack_counterparty_filter, ACCOUNT_ACTIVITY_DTYPE, ACTIVE_BY_TRANSFERS, ACTIVE_BY_VOLUME, ACTIVE_ROWS_MAX, pack_activity_filter, FILTER_CREDITS, FILTER_DEBITS, FILTER_REVERSED, pack_change_events_filter, QUERY_FILTER_DTYPE, QUERY_REVERSED, TRANSFER_DTYPE, U64_MAX, Operation)


def average_balances(row):
    """The four time-weighted average balances of one get_account_balance_integrals row — (debits_pending,
    debits_posted, credits_pending, credits_posted), each `integral // L` with L = t_end - t_open, as
    Python ints; None for an empty period (L == 0)."""
    length = int(row["t_end"]) - int(row["t_open"])
    if length == 0:
        return None
    return tuple(sum(int(row["integral_%s_w%d" % (c, k)]) << (64 * k) for k in range(3)) // length
                 for c in ("debits_pending", "debits_posted", "credits_pending", "credits_posted"))


def net_positions(cells):
    """The multilateral net of get_account_flow_matrix cells: {account id: the posted amount it received
    minus the posted amount it paid}, as Python ints, over every account the cells name on either side.
    A cell (d, c) adds its `posted` to c's position and takes it from d's; a cell (d, d) changes nothing.
    With both lists the same the positions sum to zero."""
    net = {}
    for cell in cells:
        d = int(cell["debit_id_lo"]) | int(cell["debit_id_hi"]) << 64
        c = int(cell["credit_id_lo"]) | int(cell["credit_id_hi"]) << 64
        posted = int(cell["posted_lo"]) | int(cell["posted_hi"]) << 64
        net[d] = net.get(d, 0) - posted
        net[c] = net.get(c, 0) + posted
    return net


@dataclass
class Options:
    """StateMachine.Options (state_machine.zig:216-221) plus the HBM sizing the engine needs."""
    accounts_max: int = 1 << 16
    transfers_max: int = 1 << 20
    pass_events_max: int = 8190 * 64
    pass_batches_max: int = 512
    device: int = 0
    # Two or more HIP device ordinals: a node engine, one shard per entry (include/tbgpu.h
    # tbgpu_config.devices; an ordinal may repeat: logical shards sharing one GPU).
    devices: tuple = ()
    profile: bool = False
    sequential_fallback: bool = False  # ordered fallback on one lane (tb_replay) instead of tb_flow
    # Limit checks: "auto" (scan rounds while they decide enough, then the in-order sweep), "early"
    # (sweep after the first round) or "off" (rounds only, else the ordered run); the sweep is one
    # walker per limit account, or with "window" / "window-early" one wave walking the checks in
    # event order (round 2's form).  Identical results.
    bounds_sweep: str = "auto"
    # Reference cache options are accepted for interface parity; the HBM tables hold every object.
    lsm_forest_node_count: int = 0
    cache_entries_accounts: int = 0
    cache_entries_transfers: int = 0
    cache_entries_posted: int = 0


class Engine:
    """Thin ctypes handle over one tbgpu engine: one GPU, or a node of shards (Options.devices)."""

    def __init__(self, options=None, **kw):
        options = options or Options(**kw)
        self.options = options
        self.lib = _lib.load()
        cfg = _lib.tbgpu_config(options.accounts_max, options.transfers_max, options.pass_events_max,
                                options.pass_batches_max, options.device,
                                (_lib.CONFIG_PROFILE if options.profile else 0)
                                | (_lib.CONFIG_SEQUENTIAL_FALLBACK if options.sequential_fallback else 0)
                                | {"auto": 0, "early": _lib.CONFIG_SWEEP_EARLY,
                                   "off": _lib.CONFIG_SWEEP_OFF, "window": _lib.CONFIG_SWEEP_WINDOW,
                                   "window-early": _lib.CONFIG_SWEEP_WINDOW | _lib.CONFIG_SWEEP_EARLY,
                                   }[options.bounds_sweep])
        devices = list(options.devices or ())
        if len(devices) > len(cfg.devices):
            raise ValueError("at most %d devices" % len(cfg.devices))
        cfg.device_count = len(devices)
        for i, d in enumerate(devices):
            cfg.devices[i] = int(d)
        h = ctypes.c_void_p()
        _lib.check(self.lib.tbgpu_init(ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            for _caps, bufs in (getattr(self, "_delta_bufs", None) or {}).values():
                for arr in bufs:
                    self.lib.tbgpu_unregister_host(self.h, arr.ctypes.data)
            self._delta_bufs = None
            self.lib.tbgpu_deinit(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        _lib.check(self.lib.tbgpu_reset(self.h))

    # -- commit ------------------------------------------------------------------------------
    def commit(self, operation, timestamp, body):
        """StateMachine.commit: returns the reply body bytes."""
        body = bytes(body)
        op = int(operation)
        if op in (Operation.lookup_accounts, Operation.lookup_transfers):
            cap = max(len(body) // 16 * 128, 128)
        else:
            cap = max(len(body) // 128 * 8, 8)
        out = ctypes.create_string_buffer(cap)
        n = ctypes.c_uint32(0)
        src = ctypes.create_string_buffer(body, len(body)) if body else None
        _lib.check(self.lib.tbgpu_commit(self.h, op, timestamp, src, len(body), out, cap, ctypes.byref(n)))
        return out.raw[:n.value]

    def commit_many(self, operation, timestamps, bodies):
        """N prepares in one device pass; returns the N reply bodies."""
        n = len(bodies)
        if n == 0:
            return []
        bufs = [ctypes.create_string_buffer(bytes(b), len(b)) if len(b) else None for b in bodies]
        outs = [ctypes.create_string_buffer(max(len(b) // 128 * 8, 8)) for b in bodies]
        ts = (ctypes.c_uint64 * n)(*timestamps)
        ins = (ctypes.c_void_p * n)(*[ctypes.cast(b, ctypes.c_void_p) if b is not None else None for b in bufs])
        lens = (ctypes.c_uint32 * n)(*[len(b) for b in bodies])
        outp = (ctypes.c_void_p * n)(*[ctypes.cast(o, ctypes.c_void_p) for o in outs])
        out_lens = (ctypes.c_uint32 * n)()
        _lib.check(self.lib.tbgpu_commit_many(self.h, int(operation), n, ts, ins, lens, outp, out_lens))
        return [outs[k].raw[:out_lens[k]] for k in range(n)]

    def commit_pipelined(self, operation, timestamps, lens, events, chunk_batches=0, latency=False, replies=None):
        """tbgpu_commit_pipelined over prepares stored back to back in the host array `events`
        (uint8; register it with register_host for DMA at full PCIe rate).  Returns (reply_bytes
        uint32[n], replies uint8 buffer with prepare k's reply at 8 * its first event, latency_ms
        float64[n] or None)."""
        n = len(lens)
        lens = np.asarray(lens, dtype=np.uint64)
        first = np.zeros(n, dtype=np.uint64)
        if n > 1:
            first[1:] = np.cumsum(lens[:-1])
        total = int(lens.sum())
        assert events.dtype == np.uint8 and events.flags["C_CONTIGUOUS"] and events.nbytes >= total * 128
        if replies is None or replies.nbytes < total * 8:
            replies = np.empty(max(total, 1) * 8, dtype=np.uint8)
        ts = np.ascontiguousarray(timestamps, dtype=np.uint64)
        ins = (first * 128 + np.uint64(events.ctypes.data)).astype(np.uint64)
        outs = (first * 8 + np.uint64(replies.ctypes.data)).astype(np.uint64)
        in_lens = (lens * 128).astype(np.uint32)
        out_lens = np.zeros(n, dtype=np.uint32)
        lat = np.zeros(n, dtype=np.float64) if latency else None
        P = ctypes.c_void_p
        _lib.check(self.lib.tbgpu_commit_pipelined(
            self.h, int(operation), n, ts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            ins.ctypes.data_as(ctypes.POINTER(P)), in_lens.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
            outs.ctypes.data_as(ctypes.POINTER(P)), out_lens.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
            int(chunk_batches), lat.ctypes.data if lat is not None else None))
        return out_lens, replies, lat

    def commit_pipelined_ptrs(self, operation, timestamps, lens, in_ptrs, replies, chunk_batches=0, latency=False):
        """tbgpu_commit_pipelined over prepares at explicit host addresses (in_ptrs[k]: prepare k's
        body, lens[k] events); replies: a uint8 host buffer, prepare k's reply at 8 * its first event
        (prepares in order).  Returns (reply_bytes uint32[n], latency_ms float64[n] or None)."""
        n = len(lens)
        lens = np.asarray(lens, dtype=np.uint64)
        first = np.zeros(n, dtype=np.uint64)
        if n > 1:
            first[1:] = np.cumsum(lens[:-1])
        assert replies.dtype == np.uint8 and replies.nbytes >= int(lens.sum()) * 8
        ts = np.ascontiguousarray(timestamps, dtype=np.uint64)
        ins = np.ascontiguousarray(in_ptrs, dtype=np.uint64)
        outs = (first * 8 + np.uint64(replies.ctypes.data)).astype(np.uint64)
        in_lens = (lens * 128).astype(np.uint32)
        out_lens = np.zeros(n, dtype=np.uint32)
        lat = np.zeros(n, dtype=np.float64) if latency else None
        P = ctypes.c_void_p
        _lib.check(self.lib.tbgpu_commit_pipelined(
            self.h, int(operation), n, ts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            ins.ctypes.data_as(ctypes.POINTER(P)), in_lens.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
            outs.ctypes.data_as(ctypes.POINTER(P)), out_lens.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
            int(chunk_batches), lat.ctypes.data if lat is not None else None))
        return out_lens, lat

    def register_host(self, array):
        """Pin a host array for DMA (the replica's message pool; tbgpu_register_host)."""
        _lib.check(self.lib.tbgpu_register_host(self.h, array.ctypes.data, array.nbytes))

    def unregister_host(self, array):
        _lib.check(self.lib.tbgpu_unregister_host(self.h, array.ctypes.data))

    def commit_device_async(self, operation, timestamps, lens, events_dev, results_dev, reply_bytes_dev):
        n = len(lens)
        # numpy's conversion, not a per-element ctypes array: 12K prepares took ~1.2 ms of host time
        # before the call reached the engine (a headline step is ~18 ms)
        ts = np.ascontiguousarray(timestamps, dtype=np.uint64)
        ls = np.ascontiguousarray(lens, dtype=np.uint32)
        assert len(ts) == n
        _lib.check(self.lib.tbgpu_commit_device_async(self.h, int(operation), n,
                                                      ts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                                      ls.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                      events_dev, results_dev, reply_bytes_dev))

    def sync(self):
        _lib.check(self.lib.tbgpu_sync(self.h))

    def log_window(self, events):
        """Device address where the next `events` transfer records go (tbgpu_log_window): prepares
        placed there and committed with commit_device_async(129, ..., events_dev=window) are committed
        in place."""
        w = ctypes.c_void_p(0)
        _lib.check(self.lib.tbgpu_log_window(self.h, int(events), ctypes.byref(w)))
        return int(w.value)

    @property
    def commit_timestamp(self):
        return self.lib.tbgpu_commit_timestamp(self.h)

    def set_balances(self, account_id, dp, dpost, cp, cpost):
        arr = (ctypes.c_uint64 * 8)()
        for i, v in enumerate((dp, dpost, cp, cpost)):
            arr[2 * i] = v & U64_MAX
            arr[2 * i + 1] = v >> 64
        _lib.check(self.lib.tbgpu_test_set_balances(self.h, account_id & U64_MAX, account_id >> 64, arr))

    # -- parity read-back --------------------------------------------------------------------
    def _export(self, fn, dtype, cap):
        out = np.zeros(max(cap, 1), dtype=dtype)
        n = ctypes.c_uint64(0)
        _lib.check(fn(self.h, out.ctypes.data, cap, ctypes.byref(n)))
        return out[:n.value]

    def export_accounts(self, cap=None):
        return self._export(self.lib.tbgpu_export_accounts, ACCOUNT_DTYPE, cap or self.options.accounts_max)

    def export_transfers(self, cap=None):
        return self._export(self.lib.tbgpu_export_transfers, TRANSFER_DTYPE, cap or self.options.transfers_max)

    def export_posted(self, cap=None):
        cap = cap or self.options.transfers_max
        out = np.zeros((max(cap, 1), 2), dtype=np.uint64)
        n = ctypes.c_uint64(0)
        _lib.check(self.lib.tbgpu_export_posted(self.h, out.ctypes.data, cap, ctypes.byref(n)))
        return out[:n.value]

    # -- queries -----------------------------------------------------------------------------
    def get_account_transfers(self, account_id, *, debits=True, credits=True, reversed=False, timestamp_min=0,
                              timestamp_max=0, limit=8190, out_cap_records=None):
        """The resident transfers that touched `account_id` (tbgpu_get_account_transfers): by
        timestamp ascending, newest first under `reversed`, at most `limit` (and one message body).
        Returns (records ndarray of TRANSFER_DTYPE, matched, complete): `matched` counts every match
        before the limit; `complete` is False once the engine has evicted transfers (the caller
        merges with its forest).  An invalid filter matches nothing."""
        f = self.account_filter(account_id, debits, credits, reversed, timestamp_min, timestamp_max, limit)
        return self.get_account_transfers_raw(f, out_cap_records)

    @staticmethod
    def account_filter(account_id, debits=True, credits=True, reversed=False, timestamp_min=0, timestamp_max=0,
                       limit=8190):
        """The 64 bytes of a tbgpu_account_filter (ACCOUNT_FILTER_DTYPE)."""
        f = np.zeros(1, dtype=ACCOUNT_FILTER_DTYPE)
        f["account_id_lo"], f["account_id_hi"] = account_id & U64_MAX, account_id >> 64
        f["timestamp_min"], f["timestamp_max"], f["limit"] = timestamp_min, timestamp_max, limit
        f["flags"] = ((FILTER_DEBITS if debits else 0) | (FILTER_CREDITS if credits else 0)
                      | (FILTER_REVERSED if reversed else 0))
        return f.tobytes()

    def get_account_transfers_raw(self, filter_bytes, out_cap_records=None):
        """The same query from the 64 bytes of a tbgpu_account_filter (ACCOUNT_FILTER_DTYPE)."""
        return self._account_filter_raw(self.lib.tbgpu_get_account_transfers, TRANSFER_DTYPE, filter_bytes, out_cap_records)

    def _account_filter_raw(self, fn, dtype, filter_bytes, out_cap_records):
        filter_bytes = bytes(filter_bytes)
        if len(filter_bytes) != ACCOUNT_FILTER_DTYPE.itemsize:
            raise ValueError("an account filter is %d bytes" % ACCOUNT_FILTER_DTYPE.itemsize)
        limit = int(np.frombuffer(filter_bytes, dtype=ACCOUNT_FILTER_DTYPE)["limit"][0])
        cap = min(limit, BATCH_MAX) if out_cap_records is None else int(out_cap_records)
        out = np.zeros(max(cap, 1), dtype=dtype)
        res = _lib.tbgpu_query_result()
        src = ctypes.create_string_buffer(filter_bytes, len(filter_bytes))
        _lib.check(fn(self.h, src, out.ctypes.data, cap, ctypes.byref(res)))
        return out[:res.count], int(res.matched), bool(res.complete)

    FILTERS_MAX = 64  # TBGPU_QUERY_FILTERS_MAX

    def get_account_transfers_many(self, filters, out_cap_records=None):
        """Up to 64 account filters over one read of the log (tbgpu_get_account_transfers_many).
        filters: a list of 64-byte tbgpu_account_filter records (account_filter(...) builds one).
        Returns a list of (records, matched, complete), entry i exactly what
        get_account_transfers_raw(filters[i], out_cap_records) returns; an invalid filter's entry is
        empty.  out_cap_records: room per filter (default: the largest limit, one message body at most)."""
        filters = [bytes(f) for f in filters]
        if len(filters) > self.FILTERS_MAX:
            raise ValueError("at most %d filters in one call" % self.FILTERS_MAX)
        for f in filters:
            if len(f) != ACCOUNT_FILTER_DTYPE.itemsize:
                raise ValueError("an account filter is %d bytes" % ACCOUNT_FILTER_DTYPE.itemsize)
        if not filters:
            return []
        src = np.frombuffer(b"".join(filters), dtype=ACCOUNT_FILTER_DTYPE).copy()
        cap = int(min(src["limit"].max(), BATCH_MAX)) if out_cap_records is None else int(out_cap_records)
        out = np.zeros((len(filters), max(cap, 1)), dtype=TRANSFER_DTYPE)
        res = (_lib.tbgpu_query_result * len(filters))()
        _lib.check(self.lib.tbgpu_get_account_transfers_many(self.h, src.ctypes.data, len(filters), out.ctypes.data, cap, res))
        return [(out[i, :r.count].copy(), int(r.matched), bool(r.complete)) for i, r in enumerate(res)]

    def query_many_tiles(self, tiles):
        """Tiles per chunk of get_account_transfers_many's scan (tbgpu_bench_query_many_tiles)."""
        _lib.check(self.lib.tbgpu_bench_query_many_tiles(self.h, int(tiles)))

    def get_account_balances(self, account_id, *, debits=True, credits=True, reversed=False, timestamp_min=0,
                             timestamp_max=0, limit=8190, out_cap_records=None):
        """The balances of `account_id` right after each transfer get_account_transfers returns for
        the same keywords (tbgpu_get_account_balances), in the same order: derived from the current
        balances and the resident log, whatever the account's flags.  Returns (rows ndarray of
        ACCOUNT_BALANCE_DTYPE, matched, complete); `complete` is False once the engine has evicted
        transfers or a post in a sum had lost its pending transfer (tbgpu.h says when the rows are
        exact all the same)."""
        f = self.account_filter(account_id, debits, credits, reversed, timestamp_min, timestamp_max, limit)
        return self.get_account_balances_raw(f, out_cap_records)

    def get_account_balances_raw(self, filter_bytes, out_cap_records=None):
        """get_account_balances from the 64 bytes of a tbgpu_account_filter."""
        return self._account_filter_raw(self.lib.tbgpu_get_account_balances, ACCOUNT_BALANCE_DTYPE, filter_bytes,
                                        out_cap_records)

    def get_change_events(self, timestamp_min=0, timestamp_max=0, limit=CHANGE_EVENTS_MAX, out_cap_events=None):
        """The change stream (tbgpu_get_change_events): every resident transfer of the window by
        timestamp ascending, at most `limit` (and one message body), each with its debit and its
        credit account as they stood right after it.  Returns (events ndarray of CHANGE_EVENT_DTYPE,
        matched, complete); `complete` is False once the engine has evicted transfers, a post in a sum
        had lost its pending transfer, or an event names an account the table lacks (its block is
        zero).  Page with timestamp_min = the last event's timestamp + 1."""
        return self.get_change_events_raw(pack_change_events_filter(timestamp_min, timestamp_max, limit), out_cap_events)

    def get_change_events_raw(self, filter_bytes, out_cap_events=None):
        """get_change_events from the 64 bytes of a tbgpu_change_events_filter."""
        filter_bytes = bytes(filter_bytes)
        if len(filter_bytes) != CHANGE_EVENTS_FILTER_DTYPE.itemsize:
            raise ValueError("a change-events filter is %d bytes" % CHANGE_EVENTS_FILTER_DTYPE.itemsize)
        limit = int(np.frombuffer(filter_bytes, dtype=CHANGE_EVENTS_FILTER_DTYPE)["limit"][0])
        cap = min(limit, CHANGE_EVENTS_MAX) if out_cap_events is None else int(out_cap_events)
        out = np.zeros(max(cap, 1), dtype=CHANGE_EVENT_DTYPE)
        res = _lib.tbgpu_query_result()
        src = ctypes.create_string_buffer(filter_bytes, len(filter_bytes))
        _lib.check(self.lib.tbgpu_get_change_events(self.h, src, out.ctypes.data, cap, ctypes.byref(res)))
        return out[:res.count], int(res.matched), bool(res.complete)

    LOOKUP_AT_MAX = 8191  # TBGPU_LOOKUP_AT_MAX

    def lookup_accounts_at(self, ids, timestamp, out_cap_records=None):
        """The accounts `ids` as they stood at `timestamp` (tbgpu_lookup_accounts_at): one record per id
        the table holds, in request order, a repeated id once per occurrence, with the balances less
        the effects of every resident transfer newer than `timestamp`; an account created after it is
        skipped.  timestamp 0 means now (lookup_accounts' bytes, no scan).  Returns (records ndarray
        of ACCOUNT_DTYPE, matched, complete); `complete` is False once the engine has evicted
        transfers or a post in a sum had lost its pending transfer."""
        ids = [int(i) for i in ids]
        if len(ids) > self.LOOKUP_AT_MAX:
            raise ValueError("at most %d ids in one call" % self.LOOKUP_AT_MAX)
        body = b"".join(i.to_bytes(16, "little") for i in ids)
        return self.lookup_accounts_at_raw(body, timestamp, out_cap_records)

    def lookup_accounts_at_raw(self, id_bytes, timestamp, out_cap_records=None):
        """lookup_accounts_at from the ids' bytes, 16 each ({lo, hi}, little-endian)."""
        id_bytes = bytes(id_bytes)
        if len(id_bytes) % 16 != 0:
            raise ValueError("an id is 16 bytes")
        n = len(id_bytes) // 16
        if n > self.LOOKUP_AT_MAX:
            raise ValueError("at most %d ids in one call" % self.LOOKUP_AT_MAX)
        if n == 0:  # the library returns at once and leaves its result alone
            return np.zeros(0, dtype=ACCOUNT_DTYPE), 0, True
        cap = n if out_cap_records is None else int(out_cap_records)
        out = np.zeros(max(cap, 1), dtype=ACCOUNT_DTYPE)
        res = _lib.tbgpu_query_result()
        src = ctypes.create_string_buffer(id_bytes, len(id_bytes))
        _lib.check(self.lib.tbgpu_lookup_accounts_at(self.h, int(timestamp), src, n, out.ctypes.data, cap, ctypes.byref(res)))
        return out[:res.count], int(res.matched), bool(res.complete)

    LEDGERS_MAX = LEDGERS_MAX  # TBGPU_LEDGERS_MAX

    def get_ledger_balances(self, ledgers, timestamp=0, out_cap_rows=None):
        """A trial balance per ledger as of `timestamp` (tbgpu_get_ledger_balances; 0 means now): one
        row per requested position, in request order — the four balances summed over the ledger's
        accounts, less the effects of every resident transfer of the ledger newer than `timestamp`,
        and the accounts that existed then.  Ledger 0 asks for every ledger together.  Returns (rows
        ndarray of LEDGER_BALANCE_DTYPE, matched, complete); `complete` is False once the engine has
        evicted transfers or a post in a sum had lost its pending transfer."""
        ledgers = [int(x) for x in ledgers]
        if len(ledgers) > self.LEDGERS_MAX:
            raise ValueError("at most %d ledgers in one call" % self.LEDGERS_MAX)
        if any(x < 0 or x >> 32 for x in ledgers):
            raise ValueError("a ledger is 32 bits")
        return self.get_ledger_balances_raw(np.array(ledgers, dtype="<u4").tobytes(), timestamp, out_cap_rows)

    def get_ledger_balances_raw(self, ledger_bytes, timestamp=0, out_cap_rows=None):
        """get_ledger_balances from the ledgers' bytes, 4 each (little-endian)."""
        ledger_bytes = bytes(ledger_bytes)
        if len(ledger_bytes) % 4 != 0:
            raise ValueError("a ledger is 4 bytes")
        n = len(ledger_bytes) // 4
        if n > self.LEDGERS_MAX:
            raise ValueError("at most %d ledgers in one call" % self.LEDGERS_MAX)
        if n == 0:  # the library returns at once and leaves its result alone
            return np.zeros(0, dtype=LEDGER_BALANCE_DTYPE), 0, True
        cap = n if out_cap_rows is None else int(out_cap_rows)
        out = np.zeros(max(cap, 1), dtype=LEDGER_BALANCE_DTYPE)
        res = _lib.tbgpu_query_result()
        src = ctypes.create_string_buffer(ledger_bytes, len(ledger_bytes))
        _lib.check(self.lib.tbgpu_get_ledger_balances(self.h, int(timestamp), src, n, out.ctypes.data, cap, ctypes.byref(res)))
        return out[:res.count], int(res.matched), bool(res.complete)

    PENDING_ROWS_MAX = PENDING_ROWS_MAX  # TBGPU_PENDING_ROWS_MAX

    @staticmethod
    def pending_filter(account_id=0, states=PENDING_STATES, debits=True, credits=True, reversed=False, timestamp_min=0,
                       timestamp_max=0, now=0, limit=PENDING_ROWS_MAX):
        """The 64 bytes of a tbgpu_pending_filter (PENDING_FILTER_DTYPE)."""
        account_id, states = int(account_id), int(states)
        if account_id < 0 or account_id >> 128:
            raise ValueError("an account id is 128 bits")
        if states & ~PENDING_STATES:
            raise ValueError("states is a mask of PENDING_OPEN, PENDING_EXPIRED, PENDING_POSTED and PENDING_VOIDED")
        for name, v in (("timestamp_min", timestamp_min), ("timestamp_max", timestamp_max), ("now", now)):
            if int(v) < 0 or int(v) >> 64:
                raise ValueError("%s is 64 bits" % name)
        if int(limit) < 0 or int(limit) >> 32:
            raise ValueError("limit is 32 bits")
        f = np.zeros(1, dtype=PENDING_FILTER_DTYPE)
        f["account_id_lo"], f["account_id_hi"] = account_id & U64_MAX, account_id >> 64
        f["timestamp_min"], f["timestamp_max"], f["now"], f["limit"] = timestamp_min, timestamp_max, now, limit
        f["flags"] = (states | (FILTER_DEBITS if debits else 0) | (FILTER_CREDITS if credits else 0)
                      | (FILTER_REVERSED if reversed else 0))
        return f.tobytes()

    def get_pending_transfers(self, account_id=0, *, states=PENDING_STATES, debits=True, credits=True, reversed=False,
                              timestamp_min=0, timestamp_max=0, now=0, limit=PENDING_ROWS_MAX, out_cap_rows=None):
        """The resident two-phase transfers with their state (tbgpu_get_pending_transfers): those of
        `account_id` on the wanted sides (0: any account) whose state at `now` (0: commit_timestamp) is
        in the mask `states`, by the pending record's timestamp, newest first under `reversed`.
        Returns (rows ndarray of PENDING_ROW_DTYPE, states ndarray of u8 — one PENDING_* bit a row,
        matched, complete); a row's `resolution` is the post or void record that resolved it, zero if
        none is resident; `complete` is False once transfers were evicted or a returned posted or
        voided row lacks its resolution.  An invalid filter matches nothing."""
        f = self.pending_filter(account_id, states, debits, credits, reversed, timestamp_min, timestamp_max, now, limit)
        return self.get_pending_transfers_raw(f, out_cap_rows)

    def get_pending_transfers_raw(self, filter_bytes, out_cap_rows=None):
        """The same query from the 64 bytes of a tbgpu_pending_filter (PENDING_FILTER_DTYPE)."""
        filter_bytes = bytes(filter_bytes)
        if len(filter_bytes) != PENDING_FILTER_DTYPE.itemsize:
            raise ValueError("a pending filter is %d bytes" % PENDING_FILTER_DTYPE.itemsize)
        limit = int(np.frombuffer(filter_bytes, dtype=PENDING_FILTER_DTYPE)["limit"][0])
        cap = min(limit, self.PENDING_ROWS_MAX) if out_cap_rows is None else int(out_cap_rows)
        if cap < 0 or cap >> 32:
            raise ValueError("out_cap_rows is 32 bits")
        rows = np.zeros(max(cap, 1), dtype=PENDING_ROW_DTYPE)
        states = np.zeros(max(cap, 1), dtype=np.uint8)
        res = _lib.tbgpu_query_result()
        src = ctypes.create_string_buffer(filter_bytes, len(filter_bytes))
        _lib.check(self.lib.tbgpu_get_pending_transfers(self.h, src, rows.ctypes.data, states.ctypes.data, cap, ctypes.byref(res)))
        return rows[:res.count], states[:res.count], int(res.matched), bool(res.complete)

    STATEMENTS_MAX = 4095  # TBGPU_STATEMENTS_MAX

    def get_account_statements(self, ids, t_open, t_close, out_cap_rows=None):
        """A statement header per account of `ids` over the period (t_open, t_close]
        (tbgpu_get_account_statements): the balances at its start and at its end, the gross flows in
        between and the transfer counts, one row per id the table holds and that existed at t_close,
        in request order, a repeated id once per occurrence.  t_open 0: from before every record;
        t_close 0: up to now.  Returns (rows ndarray of STATEMENT_DTYPE, matched, complete);
        `complete` is False once the engine has evicted transfers or a post in a sum had lost its
        pending transfer.  An invalid period (an end at 2^64-1, a non-zero t_close below t_open)
        matches nothing."""
        ids = [int(i) for i in ids]
        if len(ids) > self.STATEMENTS_MAX:
            raise ValueError("at most %d ids in one call" % self.STATEMENTS_MAX)
        body = b"".join(i.to_bytes(16, "little") for i in ids)
        return self.get_account_statements_raw(body, t_open, t_close, out_cap_rows)

    def get_account_statements_raw(self, id_bytes, t_open, t_close, out_cap_rows=None):
        """get_account_statements from the ids' bytes, 16 each ({lo, hi}, little-endian)."""
        id_bytes = bytes(id_bytes)
        if len(id_bytes) % 16 != 0:
            raise ValueError("an id is 16 bytes")
        n = len(id_bytes) // 16
        if n > self.STATEMENTS_MAX:
            raise ValueError("at most %d ids in one call" % self.STATEMENTS_MAX)
        if n == 0:  # the library returns at once and leaves its result alone
            return np.zeros(0, dtype=STATEMENT_DTYPE), 0, True
        cap = n if out_cap_rows is None else int(out_cap_rows)
        if cap < 0 or cap >> 32:
            raise ValueError("out_cap_rows is 32 bits")
        out = np.zeros(max(cap, 1), dtype=STATEMENT_DTYPE)
        res = _lib.tbgpu_query_result()
        src = ctypes.create_string_buffer(id_bytes, len(id_bytes))
        _lib.check(self.lib.tbgpu_get_account_statements(self.h, int(t_open), int(t_close), src, n, out.ctypes.data, cap,
                                                         ctypes.byref(res)))
        return out[:res.count], int(res.matched), bool(res.complete)

    INTEGRALS_MAX = 4095  # TBGPU_INTEGRALS_MAX

    def get_account_balance_integrals(self, ids, t_open, t_close, out_cap_rows=None):
        """The time-weighted balances of the accounts `ids` over the period (t_open, t_end]
        (tbgpu_get_account_balance_integrals): the balances at its start and at its end and, per
        column, the sum of the balance over every nanosecond of the period, modulo 2^192 (three words,
        low word first) — one row per id the table holds and that existed at t_end, in request order,
        a repeated id once per occurrence.  t_open 0 is read literally; t_close 0: t_end is
        commit_timestamp.  Returns (rows ndarray of INTEGRAL_DTYPE, matched, complete); `complete` is
        False once the engine has evicted transfers or a post in a sum had lost its pending transfer.
        An invalid period (an end at 2^64-1, t_end below t_open) matches nothing.
        average_balances(row) divides by the period's length."""
        ids = [int(i) for i in ids]
        if len(ids) > self.INTEGRALS_MAX:
            raise ValueError("at most %d ids in one call" % self.INTEGRALS_MAX)
        body = b"".join(i.to_bytes(16, "little") for i in ids)
        return self.get_account_balance_integrals_raw(body, t_open, t_close, out_cap_rows)

    def get_account_balance_integrals_raw(self, id_bytes, t_open, t_close, out_cap_rows=None):
        """get_account_balance_integrals from the ids' bytes, 16 each ({lo, hi}, little-endian)."""
        id_bytes = bytes(id_bytes)
        if len(id_bytes) % 16 != 0:
            raise ValueError("an id is 16 bytes")
        n = len(id_bytes) // 16
        if n > self.INTEGRALS_MAX:
            raise ValueError("at most %d ids in one call" % self.INTEGRALS_MAX)
        if n == 0:  # the library returns at once and leaves its result alone
            return np.zeros(0, dtype=INTEGRAL_DTYPE), 0, True
        cap = n if out_cap_rows is None else int(out_cap_rows)
        if cap < 0 or cap >> 32:
            raise ValueError("out_cap_rows is 32 bits")
        out = np.zeros(max(cap, 1), dtype=INTEGRAL_DTYPE)
        res = _lib.tbgpu_query_result()
        src = ctypes.create_string_buffer(id_bytes, len(id_bytes))
        _lib.check(self.lib.tbgpu_get_account_balance_integrals(self.h, int(t_open), int(t_close), src, n, out.ctypes.data, cap,
                                                                ctypes.byref(res)))
        return out[:res.count], int(res.matched), bool(res.complete)

    EXTREMES_MAX = 4095  # TBGPU_EXTREMES_MAX

    def get_account_balance_extremes(self, ids, t_open, t_close, measure, out_cap_rows=None):
        """The lowest and the highest value a balance of the accounts `ids` reached over the period
        [t_open, t_end], and when (tbgpu_get_account_balance_extremes).  `measure`: the coefficients of
        (debits_pending, debits_posted, credits_pending, credits_posted), each -1, 0 or +1 — the
        types.MEASURE_* tuples name the usual ones.  One EXTREME_DTYPE row per id the table holds and
        that existed at t_end, in request order, a repeated id once per occurrence: the measure at both
        ends, its low and high as signed 192-bit values (types.extreme_value reads one), the timestamps
        where each was first reached (t_open: the opening itself) and the period's records.  t_open 0
        is read literally; t_close 0: t_end is commit_timestamp.  Returns (rows, matched, complete).
        An invalid period matches nothing; an invalid measure raises.  One ordered walk of the log on a
        single engine; a node engine, and a log loaded out of timestamp order, are answered exactly
        but by a scan or two per account per page of its history."""
        ids = [int(i) for i in ids]
        if len(ids) > self.EXTREMES_MAX:
            raise ValueError("at most %d ids in one call" % self.EXTREMES_MAX)
        body = b"".join(i.to_bytes(16, "little") for i in ids)
        return self.get_account_balance_extremes_raw(body, t_open, t_close, pack_balance_measure(measure), out_cap_rows)

    def get_account_balance_extremes_raw(self, id_bytes, t_open, t_close, measure_bytes, out_cap_rows=None):
        """get_account_balance_extremes from the ids' bytes, 16 each ({lo, hi}, little-endian), and the
        measure's 8 bytes as they are (the library validates them)."""
        id_bytes, measure_bytes = bytes(id_bytes), bytes(measure_bytes)
        if len(id_bytes) % 16 != 0:
            raise ValueError("an id is 16 bytes")
        if len(measure_bytes) != 8:
            raise ValueError("a measure is 8 bytes")
        n = len(id_bytes) // 16
        if n > self.EXTREMES_MAX:
            raise ValueError("at most %d ids in one call" % self.EXTREMES_MAX)
        if n == 0:  # the library returns at once and leaves its result alone
            return np.zeros(0, dtype=EXTREME_DTYPE), 0, True
        cap = n if out_cap_rows is None else int(out_cap_rows)
        if cap < 0 or cap >> 32:
            raise ValueError("out_cap_rows is 32 bits")
        out = np.zeros(max(cap, 1), dtype=EXTREME_DTYPE)
        res = _lib.tbgpu_query_result()
        src = ctypes.create_string_buffer(id_bytes, len(id_bytes))
        m = ctypes.create_string_buffer(measure_bytes, 8)
        _lib.check(self.lib.tbgpu_get_account_balance_extremes(self.h, int(t_open), int(t_close), m, src, n, out.ctypes.data, cap,
                                                               ctypes.byref(res)))
        return out[:res.count], int(res.matched), bool(res.complete)

    SERIES_ROWS_MAX = 4095  # TBGPU_SERIES_ROWS_MAX

    def get_account_statement_series(self, ids, bounds, cap=None):
        """get_account_statements cut into consecutive periods (tbgpu_get_account_statement_series):
        for each account of `ids` one STATEMENT_DTYPE row per bucket (bounds[k], bounds[k + 1]], an
        account's rows contiguous and bucket ascending, accounts in request order; each row is the row
        get_account_statements(ids, bounds[k], bounds[k + 1]) writes, from one scan of the log.
        bounds[0] 0: from before every record; a last bound of 0: up to now; an account created at or
        below the last bound has a row in every bucket.  len(ids) * (len(bounds) - 1) is at most
        SERIES_ROWS_MAX.  Returns (rows, matched, complete); `matched` is found accounts x buckets,
        `complete` is one value for the whole answer.  Invalid bounds (one at 2^64-1, an inner zero,
        a bound below its predecessor) match nothing."""
        ids = [int(i) for i in ids]
        bounds = [int(b) for b in bounds]
        if len(bounds) < 2:
            raise ValueError("bounds name at least one bucket")
        if len(ids) * (len(bounds) - 1) > self.SERIES_ROWS_MAX:
            raise ValueError("at most %d rows in one call" % self.SERIES_ROWS_MAX)
        body = b"".join(i.to_bytes(16, "little") for i in ids)
        return self.get_account_statement_series_raw(body, bounds, cap)

    def get_account_statement_series_raw(self, id_bytes, bounds, cap=None):
        """get_account_statement_series from the ids' bytes, 16 each ({lo, hi}, little-endian)."""
        id_bytes = bytes(id_bytes)
        bounds = [int(b) for b in bounds]
        if len(id_bytes) % 16 != 0:
            raise ValueError("an id is 16 bytes")
        if len(bounds) < 2:
            raise ValueError("bounds name at least one bucket")
        if any(b < 0 or b >> 64 for b in bounds):
            raise ValueError("a bound is 64 bits")
        n, n_buckets = len(id_bytes) // 16, len(bounds) - 1
        if n * n_buckets > self.SERIES_ROWS_MAX:
            raise ValueError("at most %d rows in one call" % self.SERIES_ROWS_MAX)
        if n == 0:  # the library returns at once and leaves its result alone
            return np.zeros(0, dtype=STATEMENT_DTYPE), 0, True
        cap = n * n_buckets if cap is None else int(cap)
        if cap < 0 or cap >> 32:
            raise ValueError("cap is 32 bits")
        out = np.zeros(max(cap, 1), dtype=STATEMENT_DTYPE)
        res = _lib.tbgpu_query_result()
        src = ctypes.create_string_buffer(id_bytes, len(id_bytes))
        edges = (ctypes.c_uint64 * len(bounds))(*bounds)
        _lib.check(self.lib.tbgpu_get_account_statement_series(self.h, edges, n_buckets, src, n, out.ctypes.data, cap,
                                                               ctypes.byref(res)))
        return out[:res.count], int(res.matched), bool(res.complete)

    FLOW_MATRIX_CELLS_MAX = 4095  # TBGPU_FLOW_MATRIX_CELLS_MAX

    def get_account_flow_matrix(self, debit_ids, credit_ids, t_open, t_close, out_cap_cells=None):
        """Who paid whom over the period (t_open, t_close] (tbgpu_get_account_flow_matrix): one
        FLOW_CELL_DTYPE cell per pair of a found position of `debit_ids` and a found position of
        `credit_ids`, dense and row-major (debit rank * found credits + credit rank), with the amounts
        posted from the debit to the credit account, the holds placed and released, and the number of
        records.  A position is found as get_account_statements finds it at t_close; a repeated id is
        answered once per occurrence, and an id may stand in both lists.  len(debit_ids) *
        len(credit_ids) is at most FLOW_MATRIX_CELLS_MAX.  t_open 0: from before every record;
        t_close 0: up to now.  Returns (cells, matched, complete); `complete` is False once the
        engine has evicted transfers or a post in a cell had lost its pending transfer.  An invalid
        period matches nothing.  net_positions(cells) is the multilateral net."""
        debit_ids, credit_ids = [int(i) for i in debit_ids], [int(i) for i in credit_ids]
        if len(debit_ids) * len(credit_ids) > self.FLOW_MATRIX_CELLS_MAX:
            raise ValueError("at most %d cells in one call" % self.FLOW_MATRIX_CELLS_MAX)
        return self.get_account_flow_matrix_raw(b"".join(i.to_bytes(16, "little") for i in debit_ids),
                                                b"".join(i.to_bytes(16, "little") for i in credit_ids), t_open, t_close, out_cap_cells)

    def get_account_flow_matrix_raw(self, debit_id_bytes, credit_id_bytes, t_open, t_close, out_cap_cells=None):
        """get_account_flow_matrix from the two lists' bytes, 16 an id ({lo, hi}, little-endian)."""
        debit_id_bytes, credit_id_bytes = bytes(debit_id_bytes), bytes(credit_id_bytes)
        if len(debit_id_bytes) % 16 != 0 or len(credit_id_bytes) % 16 != 0:
            raise ValueError("an id is 16 bytes")
        n_debit, n_credit = len(debit_id_bytes) // 16, len(credit_id_bytes) // 16
        if n_debit * n_credit > self.FLOW_MATRIX_CELLS_MAX:
            raise ValueError("at most %d cells in one call" % self.FLOW_MATRIX_CELLS_MAX)
        if any(int(t) < 0 or int(t) >> 64 for t in (t_open, t_close)):
            raise ValueError("a timestamp is 64 bits")
        if n_debit == 0 or n_credit == 0:  # the library returns at once and leaves its result alone
            return np.zeros(0, dtype=FLOW_CELL_DTYPE), 0, True
        cap = n_debit * n_credit if out_cap_cells is None else int(out_cap_cells)
        if cap < 0 or cap >> 32:
            raise ValueError("out_cap_cells is 32 bits")
        out = np.zeros(max(cap, 1), dtype=FLOW_CELL_DTYPE)
        res = _lib.tbgpu_query_result()
        debit = ctypes.create_string_buffer(debit_id_bytes, len(debit_id_bytes))
        credit = ctypes.create_string_buffer(credit_id_bytes, len(credit_id_bytes))
        _lib.check(self.lib.tbgpu_get_account_flow_matrix(self.h, int(t_open), int(t_close), debit, n_debit, credit, n_credit,
                                                          out.ctypes.data, cap, ctypes.byref(res)))
        return out[:res.count], int(res.matched), bool(res.complete)

    COUNTERPARTIES_ROWS_MAX = COUNTERPARTIES_ROWS_MAX  # TBGPU_COUNTERPARTIES_ROWS_MAX

    def get_account_counterparties(self, account_id, t_open=0, t_close=0, *, debits=True, credits=True, by_volume=False,
                                   id_min=0, limit=COUNTERPARTIES_ROWS_MAX, out_cap_rows=None):
        """Who `account_id` dealt with over the period (t_open, t_close] (tbgpu_get_account_counterparties):
        one COUNTERPARTY_DTYPE row per distinct counterparty at or above `id_min`, with what the account
        paid it (to_*: `debits`) and what it paid the account (from_*: `credits`) — amounts posted, holds
        placed and released, and the number of records, as a flow-matrix cell has them.  Rows come by
        counterparty id ascending (page with id_min = the last id + 1), or with `by_volume` by
        to_posted + from_posted descending, equal volumes by id.  t_open 0: from before every record;
        t_close 0: up to now.  Returns (rows, matched, complete): `matched` is the number of groups,
        `complete` is False once the engine has evicted transfers or a matching post had lost its
        pending transfer.  An invalid filter matches nothing."""
        flags = (FILTER_DEBITS if debits else 0) | (FILTER_CREDITS if credits else 0) | (COUNTERPARTIES_BY_VOLUME if by_volume else 0)
        return self.get_account_counterparties_raw(
            pack_counterparty_filter(int(account_id), int(t_open), int(t_close), int(id_min), int(limit), flags), out_cap_rows)

    def get_account_counterparties_raw(self, filter_bytes, out_cap_rows=None):
        """get_account_counterparties from the 64 bytes of a tbgpu_counterparty_filter."""
        filter_bytes = bytes(filter_bytes)
        if len(filter_bytes) != 64:
            raise ValueError("a tbgpu_counterparty_filter is 64 bytes")
        limit = int.from_bytes(filter_bytes[48:52], "little")
        cap = min(limit, COUNTERPARTIES_ROWS_MAX) if out_cap_rows is None else int(out_cap_rows)
        if cap < 0 or cap >> 32:
            raise ValueError("out_cap_rows is 32 bits")
        out = np.zeros(max(cap, 1), dtype=COUNTERPARTY_DTYPE)
        res = _lib.tbgpu_query_result()
        src = ctypes.create_string_buffer(filter_bytes, 64)
        _lib.check(self.lib.tbgpu_get_account_counterparties(self.h, src, out.ctypes.data, cap, ctypes.byref(res)))
        return out[:res.count], int(res.matched), bool(res.complete)

    def top_counterparties(self, account_id, k=10, t_open=0, t_close=0, *, debits=True, credits=True):
        """The `k` largest counterparties of `account_id` over the period by posted volume, as
        [(counterparty id, posted to it, posted from it)] of Python ints, largest first."""
        rows, _, _ = self.get_account_counterparties(account_id, t_open, t_close, debits=debits, credits=credits, by_volume=True,
                                                     limit=k)
        return [(int(r["id_lo"]) | int(r["id_hi"]) << 64, int(r["to_posted_lo"]) | int(r["to_posted_hi"]) << 64,
                 int(r["from_posted_lo"]) | int(r["from_posted_hi"]) << 64) for r in rows]

    ACTIVE_ROWS_MAX = ACTIVE_ROWS_MAX  # TBGPU_ACTIVE_ROWS_MAX

    def get_active_accounts(self, t_open=0, t_close=0, *, ledger=0, code=0, debits=True, credits=True, by=None, id_min=0,
                            limit=ACTIVE_ROWS_MAX, out_cap_rows=None):
        """The accounts the records of the period (t_open, t_close] name (tbgpu_get_active_accounts): one
        ACCOUNT_ACTIVITY_DTYPE row per distinct account at or above `id_min`, with what it paid
        (debits_*) and what it was paid (credits_*) — amounts posted, holds placed and released, and the
        number of records, as a flow-matrix cell has them.  `ledger` and `code` narrow the records (0:
        any).  Rows come by account id ascending (page with id_min = the last id + 1), or with
        by="volume" by debits_posted + credits_posted descending, or with by="transfers" by
        debits_transfers + credits_transfers descending, ties by id.  t_open 0: from before every
        record; t_close 0: up to now.  Returns (rows, matched, complete): `matched` is the number of
        groups, `complete` is False once the engine has evicted transfers or a matching post had lost
        its pending transfer.  An invalid filter matches nothing."""
        if by not in (None, "id", "volume", "transfers"):
            raise ValueError("by is None, 'id', 'volume' or 'transfers'")
        flags = (FILTER_DEBITS if debits else 0) | (FILTER_CREDITS if credits else 0)
        flags |= ACTIVE_BY_VOLUME if by == "volume" else ACTIVE_BY_TRANSFERS if by == "transfers" else 0
        return self.get_active_accounts_raw(
            pack_activity_filter(int(t_open), int(t_close), int(id_min), int(ledger), int(code), int(limit), flags), out_cap_rows)

    def get_active_accounts_raw(self, filter_bytes, out_cap_rows=None):
        """get_active_accounts from the 64 bytes of a tbgpu_activity_filter."""
        filter_bytes = bytes(filter_bytes)
        if len(filter_bytes) != 64:
            raise ValueError("a tbgpu_activity_filter is 64 bytes")
        limit = int.from_bytes(filter_bytes[40:44], "little")
        cap = min(limit, ACTIVE_ROWS_MAX) if out_cap_rows is None else int(out_cap_rows)
        if cap < 0 or cap >> 32:
            raise ValueError("out_cap_rows is 32 bits")
        out = np.zeros(max(cap, 1), dtype=ACCOUNT_ACTIVITY_DTYPE)
        res = _lib.tbgpu_query_result()
        src = ctypes.create_string_buffer(filter_bytes, 64)
        _lib.check(self.lib.tbgpu_get_active_accounts(self.h, src, out.ctypes.data, cap, ctypes.byref(res)))
        return out[:res.count], int(res.matched), bool(res.complete)

    def top_accounts(self, t_open=0, t_close=0, k=10, by="volume", *, ledger=0, code=0, debits=True, credits=True):
        """The `k` most active accounts of the period, by posted volume or (by="transfers") by record
        count, as [(account id, posted as debit account, posted as credit account, records)] of Python
        ints, the most active first."""
        rows, _, _ = self.get_active_accounts(t_open, t_close, ledger=ledger, code=code, debits=debits, credits=credits, by=by, limit=k)
        return [(int(r["id_lo"]) | int(r["id_hi"]) << 64, int(r["debits_posted_lo"]) | int(r["debits_posted_hi"]) << 64,
                 int(r["credits_posted_lo"]) | int(r["credits_posted_hi"]) << 64,
                 int(r["debits_transfers"]) + int(r["credits_transfers"])) for r in rows]

    @staticmethod
    def query_filter(user_data_128=0, user_data_64=0, user_data_32=0, ledger=0, code=0, *, reversed=False,
                     timestamp_min=0, timestamp_max=0, limit=8190):
        """The 64 bytes of a tbgpu_query_filter (QUERY_FILTER_DTYPE); a zero field is not filtered."""
        f = np.zeros(1, dtype=QUERY_FILTER_DTYPE)
        f["user_data_128_lo"], f["user_data_128_hi"] = user_data_128 & U64_MAX, user_data_128 >> 64
        f["user_data_64"], f["user_data_32"], f["ledger"], f["code"] = user_data_64, user_data_32, ledger, code
        f["timestamp_min"], f["timestamp_max"], f["limit"] = timestamp_min, timestamp_max, limit
        f["flags"] = QUERY_REVERSED if reversed else 0
        return f.tobytes()

    def query_transfers(self, *, out_cap_records=None, **filter):
        """The resident transfers whose user_data_128 / user_data_64 / user_data_32 / ledger / code
        equal the non-zero keywords (tbgpu_query_transfers), by timestamp ascending, newest first
        under `reversed`, at most `limit`.  Returns (records, matched, complete) as
        get_account_transfers does."""
        return self.query_transfers_raw(self.query_filter(**filter), out_cap_records)

    def query_accounts(self, *, out_cap_records=None, **filter):
        """The accounts that answer the same filter (tbgpu_query_accounts), with their current
        balances; `complete` is always True."""
        return self.query_accounts_raw(self.query_filter(**filter), out_cap_records)

    def query_transfers_raw(self, filter_bytes, out_cap_records=None):
        """query_transfers from the 64 bytes of a tbgpu_query_filter."""
        return self._query_raw(self.lib.tbgpu_query_transfers, TRANSFER_DTYPE, filter_bytes, out_cap_records)

    def query_accounts_raw(self, filter_bytes, out_cap_records=None):
        """query_accounts from the 64 bytes of a tbgpu_query_filter."""
        return self._query_raw(self.lib.tbgpu_query_accounts, ACCOUNT_DTYPE, filter_bytes, out_cap_records)

    def _query_raw(self, fn, dtype, filter_bytes, out_cap_records):
        filter_bytes = bytes(filter_bytes)
        if len(filter_bytes) != QUERY_FILTER_DTYPE.itemsize:
            raise ValueError("a query filter is %d bytes" % QUERY_FILTER_DTYPE.itemsize)
        limit = int(np.frombuffer(filter_bytes, dtype=QUERY_FILTER_DTYPE)["limit"][0])
        cap = min(limit, BATCH_MAX) if out_cap_records is None else int(out_cap_records)
        out = np.zeros(max(cap, 1), dtype=dtype)
        res = _lib.tbgpu_query_result()
        src = ctypes.create_string_buffer(filter_bytes, len(filter_bytes))
        _lib.check(fn(self.h, src, out.ctypes.data, cap, ctypes.byref(res)))
        return out[:res.count], int(res.matched), bool(res.complete)

    def query_select_scans(self):
        """Table scans the last query_accounts' select made (tbgpu_bench_query_select_scans)."""
        n = ctypes.c_uint64(0)
        _lib.check(self.lib.tbgpu_bench_query_select_scans(self.h, ctypes.byref(n)))
        return n.value

    def query_keys_max(self, keys):
        """Keys per round of a query over a log out of timestamp order (tbgpu_bench_query_keys_max)."""
        _lib.check(self.lib.tbgpu_bench_query_keys_max(self.h, int(keys)))

    def stats(self):
        s = _lib.tbgpu_stats()
        _lib.check(self.lib.tbgpu_get_stats(self.h, ctypes.byref(s)))
        return {f: (list(getattr(s, f)) if f in ("flow_phase_ms", "walk_dbg", "span_ms", "span_launches", "node_shard_account_bytes") else getattr(s, f)) for f, _ in s._fields_}

    def reset_stats(self):
        self.lib.tbgpu_reset_stats(self.h)

    PROF_VALIDATE, PROF_RESOLVE, PROF_REPLAY, PROF_CLEAR, PROF_PASS, PROF_APPLY, PROF_ALL = 1, 2, 4, 8, 16, 32, 63
    PROF_SPANS = 64  # the device-clock launch spans only (no HIP event pair)

    def checkpoint_delta(self, caps=None, copy=True):
        """Objects changed since the previous call (groove write-back): a Delta of accounts (in no
        particular order), transfers (by timestamp) and posted pairs {pending timestamp,
        fulfillment}.  caps: initial buffer sizes (accounts, transfers, posted); grown and retried
        when too small (the engine says what suffices).  copy=False returns views of the buffers the
        engine keeps registered for DMA: valid only until the next write-back."""
        counts = _lib.tbgpu_delta_counts()
        caps = list(caps) if caps else [1024, 1024, 1024]
        if getattr(self, "_wb_inflight", None) is not None:  # its buffers belong to the engine until the wait
            raise _lib.EngineError(_lib.STATUS_INVALID, "an asynchronous write-back is in flight "
                                                        "(checkpoint_delta_wait first)")
        while True:
            a, before, t, p = self._delta_buffers(caps, 0)
            st = self.lib.tbgpu_checkpoint_delta(self.h, a.ctypes.data, before.ctypes.data, caps[0], t.ctypes.data,
                                                 caps[1], p.ctypes.data, caps[2], ctypes.byref(counts))
            need = [counts.accounts, counts.transfers, counts.posted]
            if st == _lib.STATUS_INVALID and any(n > c for n, c in zip(need, caps)):
                caps = [max(c, n) for c, n in zip(caps, need)]
                continue
            _lib.check(st)
            return self._delta(a, before, t, p, counts, copy)

    def checkpoint_delta_async(self, caps):
        """tbgpu_checkpoint_delta_async into one of two registered buffer sets of at least `caps`
        (accounts, transfers, posted) entries — size them for a bar, as the Zig wrapper does; the
        objects land while later commits run.  checkpoint_delta_wait() returns the Delta."""
        if getattr(self, "_wb_inflight", None) is not None:  # never touch a set the engine may be copying into
            raise _lib.EngineError(_lib.STATUS_INVALID, "an asynchronous write-back is in flight "
                                                        "(checkpoint_delta_wait first)")
        which = 1 - getattr(self, "_wb_set", 1)
        a, before, t, p = self._delta_buffers(list(caps), which)
        _lib.check(self.lib.tbgpu_checkpoint_delta_async(self.h, a.ctypes.data, before.ctypes.data, caps[0],
                                                         t.ctypes.data, caps[1], p.ctypes.data, caps[2]))
        self._wb_set = which  # flipped only once the call succeeded
        self._wb_inflight = (a, before, t, p)

    def checkpoint_delta_wait(self, copy=True):
        counts = _lib.tbgpu_delta_counts()
        _lib.check(self.lib.tbgpu_checkpoint_delta_wait(self.h, ctypes.byref(counts)))
        a, before, t, p = self._wb_inflight
        self._wb_inflight = None
        return self._delta(a, before, t, p, counts, copy)

    @staticmethod
    def _delta(a, before, t, p, counts, copy):
        need = [counts.accounts, counts.transfers, counts.posted]
        parts = (a[:need[0]], t[:need[1]], p[:need[2]], before[:need[0]])
        if copy:
            parts = tuple(x.copy() for x in parts)
        return Delta(*parts, counts.created_after)

    def _delta_buffers(self, caps, which):
        """Write-back buffer set `which` (0 / 1) of at least `caps` entries, kept (and registered)
        across calls."""
        sets = getattr(self, "_delta_bufs", None) or {}
        have = sets.get(which)
        if have is not None and all(h >= c for h, c in zip(have[0], caps)):
            return have[1]
        if have is not None:
            for arr in have[1]:
                _lib.check(self.lib.tbgpu_unregister_host(self.h, arr.ctypes.data))
        caps = [max(c, 1) for c in caps]
        bufs = (np.empty(caps[0], dtype=ACCOUNT_DTYPE), np.empty((caps[0], 8), dtype=np.uint64),
                np.empty(caps[1], dtype=TRANSFER_DTYPE), np.empty((caps[2], 2), dtype=np.uint64))
        for arr in bufs:
            _lib.check(self.lib.tbgpu_register_host(self.h, arr.ctypes.data, arr.nbytes))
        sets[which] = (caps, bufs)
        self._delta_bufs = sets
        return bufs

    def ledger_summary(self):
        """{"debits_pending", "debits_posted", "credits_pending", "credits_posted": u128 sums over every
        account (every shard of a node), "accounts": live accounts, "stray": balances held by a shard
        that is not the account's owner (node engines; must be 0)} — tbgpu_bench_ledger_summary."""
        s = _lib.tbgpu_ledger_summary()
        _lib.check(self.lib.tbgpu_bench_ledger_summary(self.h, ctypes.byref(s)))
        names = ("debits_pending", "debits_posted", "credits_pending", "credits_posted")
        out = {n: int(s.sums[2 * i]) | (int(s.sums[2 * i + 1]) << 64) for i, n in enumerate(names)}
        out.update(accounts=int(s.accounts), stray=int(s.stray))
        return out

    def checkpoint_mark(self):
        """Take the current state as written back (tbgpu_bench_checkpoint_mark)."""
        _lib.check(self.lib.tbgpu_bench_checkpoint_mark(self.h))

    def shard(self, d):
        """A node engine's shard d as an Engine sharing its handle (tbgpu_bench_node_shard): device
        buffers, copies and the generators on shard d's GPU.  Never closed on its own."""
        h = ctypes.c_void_p()
        _lib.check(self.lib.tbgpu_bench_node_shard(self.h, int(d), ctypes.byref(h)))
        view = Engine.__new__(Engine)
        view.options, view.lib, view.h = self.options, self.lib, h
        view.close = lambda: None
        return view

    def node_imports(self, d):
        """{"live", "room", "flushes"} of a node engine's import gate on shard d, read with the engine
        drained (tbgpu_bench_node_imports)."""
        out = (ctypes.c_uint64 * 3)()
        _lib.check(self.lib.tbgpu_bench_node_imports(self.h, int(d), out))
        return dict(live=int(out[0]), room=int(out[1]), flushes=int(out[2]))

    def walk_merge_max(self, segments):
        """Heavy segments the limit-check sweep walks merged on one wave at most (0: a wave each)."""
        _lib.check(self.lib.tbgpu_bench_walk_merge_max(self.h, int(segments)))

    def legs_min_events(self, events):
        """Passes of >= events transfers use the sorted balance legs (0: every pass)."""
        _lib.check(self.lib.tbgpu_bench_legs_min_events(self.h, int(events)))

    MIX_PARTS = ("stream", "probe", "cas", "stream+probe", "stream+cas", "probe+cas", "all")

    def access_mix(self, transfers):
        """Mean ms of kernel 1's memory-access mix without its logic, per part (tbgpu_bench.h)."""
        out = (ctypes.c_double * 7)()
        _lib.check(self.lib.tbgpu_bench_access_mix(self.h, int(transfers), out))
        return dict(zip(self.MIX_PARTS, list(out)))

    def profile_mask(self, mask):
        """Kernels timed with HIP events when profiling (include/tbgpu_bench.h)."""
        _lib.check(self.lib.tbgpu_bench_profile_mask(self.h, mask))

    # -- multi-GPU primitives (include/tbgpu_shard.h; driven by tigerbeetle_amd.sharded) -------
    def route_init(self, world, events_max):
        _lib.check(self.lib.tbgpu_route_init(self.h, world, events_max))

    def fetch_accounts(self, ids):
        """ids: uint64 [n, 2] (lo, hi).  Returns (ACCOUNT_DTYPE[n], found uint8[n])."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1, 2)
        n = ids.shape[0]
        out = np.zeros(n, dtype=ACCOUNT_DTYPE)
        found = np.zeros(n, dtype=np.uint8)
        if n:
            _lib.check(self.lib.tbgpu_fetch_accounts(self.h, ids.ctypes.data, n, out.ctypes.data, found.ctypes.data))
        return out, found

    def fetch_transfers(self, ids):
        """ids: uint64 [n, 2].  Returns (TRANSFER_DTYPE[n], state uint8[n]: 0 absent, 1 + posted)."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1, 2)
        n = ids.shape[0]
        out = np.zeros(n, dtype=TRANSFER_DTYPE)
        state = np.zeros(n, dtype=np.uint8)
        if n:
            _lib.check(self.lib.tbgpu_fetch_transfers(self.h, ids.ctypes.data, n, out.ctypes.data, state.ctypes.data))
        return out, state

    def upsert_accounts(self, records):
        records = np.ascontiguousarray(records, dtype=ACCOUNT_DTYPE)
        if len(records):
            _lib.check(self.lib.tbgpu_upsert_accounts(self.h, records.ctypes.data, len(records)))

    def load_accounts(self, records):
        """Insert the accounts the engine lacks (replica restart warm-up, tbgpu_load_accounts)."""
        records = np.ascontiguousarray(records, dtype=ACCOUNT_DTYPE)
        if len(records):
            _lib.check(self.lib.tbgpu_load_accounts(self.h, records.ctypes.data, len(records)))

    def load_transfers(self, records, posted_state):
        records = np.ascontiguousarray(records, dtype=TRANSFER_DTYPE)
        posted_state = np.ascontiguousarray(posted_state, dtype=np.uint8)
        if len(records):
            _lib.check(self.lib.tbgpu_load_transfers(self.h, records.ctypes.data, posted_state.ctypes.data,
                                                     len(records)))

    def evict_transfers(self, keep):
        """Drop the written-back transfers older than the newest `keep` log positions
        (tbgpu_evict_transfers); returns how many left."""
        n = ctypes.c_uint64(0)
        _lib.check(self.lib.tbgpu_evict_transfers(self.h, int(keep), ctypes.byref(n)))
        return n.value

    def transfers_maybe_cold(self, ids):
        """ids: uint64 [n, 2] (lo, hi).  Returns bool[n]: not resident and maybe evicted (load them
        from the forest before the commit that names them)."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1, 2)
        out = np.zeros(len(ids), dtype=np.uint8)
        if len(ids):
            _lib.check(self.lib.tbgpu_transfers_maybe_cold(self.h, ids.ctypes.data, len(ids), out.ctypes.data))
        return out.astype(bool)

    def set_commit_timestamp(self, timestamp):
        _lib.check(self.lib.tbgpu_set_commit_timestamp(self.h, int(timestamp)))

    def upsert_transfers(self, records, state):
        records = np.ascontiguousarray(records, dtype=TRANSFER_DTYPE)
        state = np.ascontiguousarray(state, dtype=np.uint8)
        if len(records):
            _lib.check(self.lib.tbgpu_upsert_transfers(self.h, records.ctypes.data, state.ctypes.data, len(records)))

    # -- device memory + workload generation (bench) -----------------------------------------
    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        _lib.check(self.lib.tbgpu_device_alloc(self.h, nbytes, ctypes.byref(p)))
        return p.value

    def free(self, ptr):
        _lib.check(self.lib.tbgpu_device_free(self.h, ptr))

    def to_host(self, ptr, nbytes):
        out = np.empty(nbytes, dtype=np.uint8)
        _lib.check(self.lib.tbgpu_copy_to_host(self.h, out.ctypes.data, ptr, nbytes))
        return out

    def to_device(self, ptr, array):
        array = np.ascontiguousarray(array)
        _lib.check(self.lib.tbgpu_copy_to_device(self.h, ptr, array.ctypes.data, array.nbytes))

    def copy_device_async(self, dst_dev, src_dev, nbytes):
        """Device to device on the engine's stream (tbgpu_copy_device_async): time it with markers."""
        _lib.check(self.lib.tbgpu_copy_device_async(self.h, dst_dev, src_dev, int(nbytes)))

    def generate_accounts(self, out_dev, first, count, seed=42, limit_permille=0, account_count=0, hot_limited=0):
        """hot_limited > 0 (the hottest Zipf ranks get a limit flag too) needs account_count."""
        w = _lib.tbgpu_workload(seed, account_count, 0, limit_permille, 0.0, hot_limited, 0)
        _lib.check(self.lib.tbgpu_bench_generate_accounts(self.h, out_dev, first, count, ctypes.byref(w)))

    def generate_transfers(self, out_dev, first, count, account_count, seed=42, kind=0, limit_permille=0,
                           zipf_s=1.2, hot_limited=0):
        """kind 0: C2 uniform; 1: C3 Zipf + limit-account funding; 2: C4 chains / two-phase / balancing
        (include/tbgpu_bench.h).  limit_permille must match generate_accounts' for kind 1."""
        w = _lib.tbgpu_workload(seed, account_count, kind, limit_permille, zipf_s, hot_limited, 0)
        _lib.check(self.lib.tbgpu_bench_generate_transfers(self.h, out_dev, first, count, ctypes.byref(w)))

    def reset_transfers(self):
        _lib.check(self.lib.tbgpu_bench_reset_transfers(self.h))

    def pass_latencies(self, cap=1 << 20):
        out = np.zeros(cap, dtype=np.float64)
        n = ctypes.c_uint64(0)
        _lib.check(self.lib.tbgpu_bench_pass_latencies(self.h, out.ctypes.data, cap, ctypes.byref(n)))
        return out[:n.value]

    def marker(self, slot):
        _lib.check(self.lib.tbgpu_marker(self.h, slot))

    def marker_elapsed_ms(self, a, b):
        return self.lib.tbgpu_marker_elapsed_ms(self.h, a, b)


@dataclass
class Delta:
    """One groove write-back (tbgpu_checkpoint_delta)."""
    accounts: np.ndarray
    transfers: np.ndarray
    posted: np.ndarray
    # [n, 8] u64: {dp, dpost, cp, cpost} (lo, hi) of each account as of the previous write-back
    accounts_before: np.ndarray = None
    # accounts with a timestamp above this were created since the previous write-back (insert)
    created_after: int = 0


class StateMachine:
    """The reference's StateMachine interface over one Engine."""

    Operation = Operation
    batch_max = BATCH_MAX

    def __init__(self, options=None, write_back=None, **kw):
        self.engine = Engine(options, **kw)
        self.write_back = write_back  # called by checkpoint with a Delta
        self.prepare_timestamp = 0
        self.commit_timestamp = 0

    def deinit(self):
        self.engine.close()

    def reset(self):
        self.engine.reset()
        self.prepare_timestamp = 0
        self.commit_timestamp = 0

    @staticmethod
    def event_count(operation, body):
        if operation in (Operation.create_accounts, Operation.create_transfers):
            return len(body) // 128
        return 0

    def prepare(self, operation, body):
        """state_machine.zig:336-343."""
        self.prepare_timestamp += self.event_count(Operation(operation), body)

    def prefetch(self, callback, op, operation, body):
        """state_machine.zig:345-506.  Every object is HBM-resident: complete synchronously."""
        assert op != 0
        callback(self)

    def commit(self, client, op, timestamp, operation, body):
        """state_machine.zig:508-540.  Returns the reply body (bytes)."""
        del client
        assert op != 0
        reply = self.engine.commit(int(operation), timestamp, body)
        self.commit_timestamp = self.engine.commit_timestamp
        return reply

    def get_account_transfers(self, account_id, **filter):
        """The account-filter query (Engine.get_account_transfers): a read, no operation number in
        the reference's enum, so it does not go through commit."""
        return self.engine.get_account_transfers(account_id, **filter)

    def get_account_transfers_many(self, filters, out_cap_records=None):
        """Consecutive get_account_transfers requests with no write between them, answered by one
        read of the log (Engine.get_account_transfers_many): a read, not a commit."""
        return self.engine.get_account_transfers_many(filters, out_cap_records)

    def get_account_balances(self, account_id, **filter):
        """The balance history of one account (Engine.get_account_balances): a read, not a commit."""
        return self.engine.get_account_balances(account_id, **filter)

    def get_change_events(self, **filter):
        """The change stream (Engine.get_change_events): a read, not a commit."""
        return self.engine.get_change_events(**filter)

    def lookup_accounts_at(self, ids, timestamp, out_cap_records=None):
        """The accounts as they stood at a timestamp (Engine.lookup_accounts_at): a read, not a commit."""
        return self.engine.lookup_accounts_at(ids, timestamp, out_cap_records)

    def get_ledger_balances(self, ledgers, timestamp=0, out_cap_rows=None):
        """A trial balance per ledger as of a timestamp (Engine.get_ledger_balances): a read, not a commit."""
        return self.engine.get_ledger_balances(ledgers, timestamp, out_cap_rows)

    def get_pending_transfers(self, account_id=0, **filter):
        """The two-phase transfers with their state (Engine.get_pending_transfers): a read, not a commit."""
        return self.engine.get_pending_transfers(account_id, **filter)

    def get_account_statements(self, ids, t_open, t_close, out_cap_rows=None):
        """Statement headers over a period (Engine.get_account_statements): a read, not a commit."""
        return self.engine.get_account_statements(ids, t_open, t_close, out_cap_rows)

    def get_account_balance_integrals(self, ids, t_open, t_close, out_cap_rows=None):
        """Time-weighted balances over a period (Engine.get_account_balance_integrals): a read, not a commit."""
        return self.engine.get_account_balance_integrals(ids, t_open, t_close, out_cap_rows)

    def get_account_balance_extremes(self, ids, t_open, t_close, measure, out_cap_rows=None):
        """A balance's low and high over a period (Engine.get_account_balance_extremes): a read, not a commit."""
        return self.engine.get_account_balance_extremes(ids, t_open, t_close, measure, out_cap_rows)

    def get_account_statement_series(self, ids, bounds, cap=None):
        """Statement headers per bucket (Engine.get_account_statement_series): a read, not a commit."""
        return self.engine.get_account_statement_series(ids, bounds, cap)

    def get_account_flow_matrix(self, debit_ids, credit_ids, t_open, t_close, out_cap_cells=None):
        """Who paid whom over a period (Engine.get_account_flow_matrix): a read, not a commit."""
        return self.engine.get_account_flow_matrix(debit_ids, credit_ids, t_open, t_close, out_cap_cells)

    def get_account_flow_matrix_raw(self, debit_id_bytes, credit_id_bytes, t_open, t_close, out_cap_cells=None):
        """The same from the two lists' bytes (Engine.get_account_flow_matrix_raw)."""
        return self.engine.get_account_flow_matrix_raw(debit_id_bytes, credit_id_bytes, t_open, t_close, out_cap_cells)

    def get_account_counterparties(self, account_id, t_open=0, t_close=0, **kwargs):
        """Who an account dealt with over a period (Engine.get_account_counterparties): a read, not a commit."""
        return self.engine.get_account_counterparties(account_id, t_open, t_close, **kwargs)

    def top_counterparties(self, account_id, k=10, t_open=0, t_close=0, **kwargs):
        """The k largest counterparties by posted volume (Engine.top_counterparties)."""
        return self.engine.top_counterparties(account_id, k, t_open, t_close, **kwargs)

    def get_active_accounts(self, t_open=0, t_close=0, **kwargs):
        """The accounts a period's records name (Engine.get_active_accounts): a read, not a commit."""
        return self.engine.get_active_accounts(t_open, t_close, **kwargs)

    def top_accounts(self, t_open=0, t_close=0, k=10, by="volume", **kwargs):
        """The k most active accounts by posted volume or record count (Engine.top_accounts)."""
        return self.engine.top_accounts(t_open, t_close, k, by, **kwargs)

    def query_transfers(self, **filter):
        """The field-filter query over transfers (Engine.query_transfers): a read, not a commit."""
        return self.engine.query_transfers(**filter)

    def query_accounts(self, **filter):
        """The field-filter query over accounts (Engine.query_accounts): a read, not a commit."""
        return self.engine.query_accounts(**filter)

    def compact(self, callback, op):
        del op
        callback(self)

    def checkpoint(self, callback):
        delta = self.engine.checkpoint_delta()
        if self.write_back is not None:
            self.write_back(delta)
        callback(self)
