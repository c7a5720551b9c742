"""The account-filter scan (tbgpu_get_account_transfers, csrc/k_query.h) over a 16M-transfer log (2 GB)
against a device-to-device copy of the same log range, in one process.

usage: python tools/gpu/query_scan.py [transfers] [runs] [--only account|fields|balances|change_events|many|asof|ledgers|pending|statements|integrals|extremes|series|matrix]

The log is built by the device generator, committed in place (the way tools/gpu/device_pass.py builds
a pass): once with uniform C2 ids, where the queried account is a cold one (a few dozen matches), and
once with the Zipf draw, where it is the hottest account.  Each query (limit 8190, ascending and
newest first) is timed with the engine's markers, three warm-ups then the median of `runs`; so is the
copy.  Both load shapes of tb_query_count are measured (TBGPU_QUERY_COOP, read at tbgpu_init).
Prints one JSON line; the bar is query <= copy.

The field-filter queries (tbgpu_query_transfers / tbgpu_query_accounts) are measured the
same way on the uniform log and its 1M-account table: query_transfers with a selective filter (code and
ledger) and a broad one (ledger only) against the copy of the log; query_accounts with an all-match
filter (ledger only), a selective one with more matches than the limit, and one with fewer, against a
device-to-device copy of 64 B x slots (the hot and cold entries the scan reads), with the number of
table scans the select made.  `--only account` measures the account filter alone (an older library
loaded through TBGPU_AB_LIB has nothing else), `--only fields` the field filters alone.

`--only balances` (tbgpu_get_account_balances) times get_account_balances beside
get_account_transfers with the same filter on both logs, both directions, limit 8190: it scans the log
once more, so the bar is about twice the time (explain a cold-account ratio above 2.5).

`--only change_events` (tbgpu_get_change_events) times a page of limit 2730 beside
query_transfers with the same window and limit and beside the copy of the log: the newest page of the
uniform log (nothing is newer: the second scan reads timestamps only), its oldest page (the whole log
is newer) and the oldest page of the Zipf log, whose set holds the hottest account.

`--only many` (tbgpu_get_account_transfers_many) times the batched call — the C call alone,
into buffers made once — for 1, 8 and 64 cold filters on distinct accounts of the uniform log, the 64 all
newest first, and 64 filters of the Zipf log that include its hottest account, beside the copy of the
log and one single cold query of the same run; 64 x that single query's median is the yardstick.  It
also times the 64 cold filters with chunks of 8, 16, 32 and 64 tiles.

`--only asof` (tbgpu_lookup_accounts_at) times the C call alone, into buffers made once, on
both logs, beside get_change_events' oldest page and query_transfers with the same window in the same
process: a request of that page's distinct accounts (at most 5,460: the scan reads what the page's
second scan reads) and one of 8,191 ids, each with T older than every transfer (the whole log is newer)
and T newer than every transfer (the scan reads timestamps only), and the 8,191 ids with T = 0 (no
scan).  The yardstick is the page's second pass, get_change_events less query_transfers.

`--only ledgers` (tbgpu_get_ledger_balances) times the C call alone, into buffers made once,
on the uniform log and its one-ledger table: T = 0 with 1 and with 1,024 requested ledgers (the table
scan alone), T newer than every transfer (the log scan reads timestamps only), T at the log's middle
and T older than every transfer.  The yardsticks run in the same process: query_accounts with a
ledger-only all-match filter and a device-to-device copy of the bytes the table scan reads (32 B a slot
and 64 B a live account); query_transfers with an all-zero filter, timestamp_min = T + 1 and limit 1,
which takes the same liveness probe on every record of the window.  Then, on a second engine without
a log, the same table with its accounts spread over 2 and over 1,024 ledgers, every ledger asked.

`--only pending` (tbgpu_get_pending_transfers) fills the log with the C4 shape (chains,
two-phase transfers with timeouts, 2 s gaps), so that open, expired, posted and voided rows all exist,
and times the C call alone, into buffers made once, beside query_transfers with an all-zero filter over
the same window in the same process: the selection alone (any account, OPEN | EXPIRED: no row is
resolved, so no join runs), any account and all four states, the join with 4,095 resolved rows and with
one (POSTED | VOIDED, ascending: the whole log is newer than the oldest row; newest first: only the
log's end is), and one named account.

`--only statements` (tbgpu_get_account_statements) times the C call alone, into buffers made
once, on both logs: 4,095 ids (distinct accounts of the log's middle; on the Zipf log its hottest accounts
first) with the period covering the whole log, its middle half, and t_open above every record (the scan
reads timestamps only).  The yardstick runs in the same process: two tbgpu_lookup_accounts_at calls with
the same ids at T = t_open and T = t_close, timed together; the aim is below their sum.  An older library
loaded through TBGPU_AB_LIB lacks the call: the yardstick alone is timed then.

`--only integrals` (tbgpu_get_account_balance_integrals) times the C call alone, into buffers
made once, on both logs, with --only statements' ids and periods: the whole log, its middle half, and t_open
at the last record (the scan reads timestamps only).  The yardstick runs in the same process: one
tbgpu_get_account_statements call with the same ids and period.  An older library loaded through
TBGPU_AB_LIB lacks the call: its get_account_statements alone is timed then, the yardstick to hold this
build's call against.

`--only extremes` (tbgpu_get_account_balance_extremes) times the C call alone, into buffers made
once, on both logs: n = 1 (a cold and the hottest account), 64 and 4,095 ids, the whole log and its middle half,
each beside tbgpu_get_account_statements for the same ids and period, the order-free yardstick; then engines made
under TBGPU_EXTREMES_SLABS (256, 64, 16, 1) for n = 4,095 and under TBGPU_EXTREMES_EXACT=1 for n = 1 hottest and
n = 64 (three runs each; --skip-exact leaves them out).
`--only series` (tbgpu_get_account_statement_series) times the C call alone, into buffers made
once, on both logs, at (ids, buckets) = (4095, 1), (136, 30), (11, 365) and (1, 4095) with equal buckets over
the whole log and --only statements' ids.  The yardsticks run in the same process: the same question asked as
one tbgpu_get_account_statements call per bucket (three runs for 365 buckets and more), and one such call over
the whole period.  An older library loaded through TBGPU_AB_LIB lacks the call: the yardsticks alone are
timed then.

`--only matrix` (tbgpu_get_account_flow_matrix) times the C call alone, into buffers made once,
on both logs: 63 x 63 over the hottest accounts (both lists the same), 63 x 63 over random accounts of the
log's middle, 1 x 4,095 and 4,095 x 1, each over the whole log and over its middle half.  The yardstick runs in
the same process: one tbgpu_get_account_statements call over the same ids and period.  For the hot 63 x 63 leg
over the whole log the host alternative the call replaces is timed once by the wall clock: every debit
account's tbgpu_get_account_transfers pages, grouped by credit account in Python, and its cells are compared
with the call's.  An older library loaded through TBGPU_AB_LIB lacks the call: the yardstick alone is timed then.

`--only counterparties` (tbgpu_get_account_counterparties) times the C call alone, into buffers
made once, on both logs: the Zipf log's hottest account and a cold one and an account of the uniform log, both
sides, by id and by volume, limit 10 and 8,191, over the whole log; and the call's fixed cost — the group table
zeroed and selected over, whatever the log holds — as the same call over an empty period.  The yardsticks run in
the same process: one tbgpu_get_account_statements call for that one account and period (what one scan costs),
and, once per subject by the wall clock, the host alternative the call replaces: the account's
tbgpu_get_account_transfers pages grouped by counterparty in Python, whose groups are compared with the call's.
An older library loaded through TBGPU_AB_LIB lacks the call: the yardsticks alone are timed then.

`--only activity` (tbgpu_get_active_accounts) times the C call alone, into buffers made once, on
the uniform and the Zipf log and on a log whose records all name one pair of accounts (the combine's other
extreme): the whole log by id at limit 8,191, by volume and by record count at limit 10, a period newer than every
record, a ledger no record carries (the generator's codes cover all 65,535 values, so the word-14 test that
nothing passes is on the ledger) and one code (a few hundred records).  The yardsticks run in the same process:
tbgpu_query_transfers with an all-zero filter, timestamp_min = t_open + 1 and limit 1 (the same liveness probe on
every record of the window), tbgpu_get_account_counterparties for the Zipf log's hottest account and over an empty
period (what its scan reads for an empty window), and a device-to-device copy of the log.  The host alternative is
timed once by the wall clock on the uniform log: tbgpu_query_transfers pages over the whole log, grouped by account
in numpy, whose groups are compared with the call's (--skip-host leaves it out).  An older library loaded through TBGPU_AB_LIB lacks the
call: the yardsticks and the host alternative alone are timed then.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np  # noqa: E402

from tests.harness.configs import KINDS, batches, timestamps  # noqa: E402
from tigerbeetle_amd.state_machine import Engine, Options  # noqa: E402
from tigerbeetle_amd.types import ACCOUNT_DTYPE, TRANSFER_DTYPE  # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith("--")]
only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
argv = [a for a in argv if a != only]
n_xfer = int(argv[0]) if len(argv) > 0 else 1 << 24
runs = int(argv[1]) if len(argv) > 1 else 21
n_acct, batch, pb = 1_000_000, 8190, 512
WARMUPS = 3


def timed(e, fn):
    out = []
    for i in range(WARMUPS + runs):
        e.marker(0)
        fn()
        e.marker(1)
        e.sync()
        if i >= WARMUPS:
            out.append(e.marker_elapsed_ms(0, 1))
    return statistics.median(out), min(out), max(out)


def rates(ms):
    return dict(ms=round(ms, 4), log_gbs=round(n_xfer * 128 / ms / 1e6, 1), needed_gbs=round(n_xfer * 40 / ms / 1e6, 1))


def measure(coop, balances=False):
    os.environ["TBGPU_QUERY_COOP"] = "1" if coop else "0"
    e = Engine(Options(accounts_max=n_acct, transfers_max=n_xfer, pass_events_max=pb * batch, pass_batches_max=pb))
    a_lens = batches(n_acct, batch)
    a_ts, t = timestamps(a_lens, 1_000_000_000)
    acct = e.alloc(n_acct * 128)
    e.generate_accounts(acct, 0, n_acct, seed=42)
    res = e.alloc(max(n_acct, n_xfer) * 8)
    rb = e.alloc((n_xfer // batch + 2) * 4)
    e.commit_device_async(128, a_ts, a_lens, acct, res, rb)
    e.sync()
    spare = e.alloc(n_xfer * 128)
    out = {}
    for name, kind in (("uniform_cold", "c2"), ("zipf_hot", "c3")):
        if name != "uniform_cold":
            e.reset_transfers()
        log = e.log_window(n_xfer)
        e.generate_transfers(log, 0, n_xfer, n_acct, seed=42, kind=KINDS[kind])
        e.sync()
        x_lens = batches(n_xfer, batch)
        x_ts, t = timestamps(x_lens, t + 10)
        e.commit_device_async(129, x_ts, x_lens, log, res, rb)
        e.sync()
        # The queried account: the debit account of the log's middle record (cold), or the most
        # frequent debit account of a sample (hot).
        sample = e.to_host(log + (n_xfer // 2) * 128, min(n_xfer // 2, 1 << 16) * 128).view(TRANSFER_DTYPE)
        if name == "uniform_cold":
            lo, hi = int(sample["debit_account_id_lo"][0]), int(sample["debit_account_id_hi"][0])
        else:
            ids, counts = np.unique(sample[["debit_account_id_lo", "debit_account_id_hi"]], return_counts=True)
            lo, hi = (int(v) for v in ids[np.argmax(counts)])
        account = lo | (hi << 64)
        for rev in (False, True):
            recs, matched, complete = e.get_account_transfers(account, reversed=rev, limit=8190)
            ts = recs["timestamp"].astype(np.int64)
            assert complete and len(recs) == min(matched, 8190) and np.all(np.diff(ts) < 0 if rev else np.diff(ts) > 0)
            med, lo_ms, hi_ms = timed(e, lambda: e.get_account_transfers(account, reversed=rev, limit=8190))
            out["%s_%s" % (name, "reversed" if rev else "ascending")] = dict(rates(med), min_ms=round(lo_ms, 4),
                                                                             max_ms=round(hi_ms, 4), matched=matched,
                                                                             count=len(recs))
            if balances:
                rows, b_matched, b_complete = e.get_account_balances(account, reversed=rev, limit=8190)
                assert b_complete and b_matched == matched and np.array_equal(rows["timestamp"], recs["timestamp"])
                b_med, b_lo, b_hi = timed(e, lambda: e.get_account_balances(account, reversed=rev, limit=8190))
                out["%s_%s" % (name, "reversed" if rev else "ascending")].update(
                    balances_ms=round(b_med, 4), balances_min_ms=round(b_lo, 4), balances_max_ms=round(b_hi, 4),
                    balances_over_transfers=round(b_med / med, 2))
        if name == "uniform_cold":
            med, lo_ms, hi_ms = timed(e, lambda: e.copy_device_async(spare, log, n_xfer * 128))
            out["copy_d2d"] = dict(rates(med), min_ms=round(lo_ms, 4), max_ms=round(hi_ms, 4))
    e.close()
    return out


def row(med, lo_ms, hi_ms, **more):
    return dict(ms=round(med, 4), min_ms=round(lo_ms, 4), max_ms=round(hi_ms, 4), **more)


def measure_fields():
    """query_transfers and query_accounts on the uniform log and its account table."""
    os.environ["TBGPU_QUERY_COOP"] = "0"
    e = Engine(Options(accounts_max=n_acct, transfers_max=n_xfer, pass_events_max=pb * batch, pass_batches_max=pb))
    a_lens = batches(n_acct, batch)
    a_ts, t = timestamps(a_lens, 1_000_000_000)
    acct = e.alloc(n_acct * 128)
    e.generate_accounts(acct, 0, n_acct, seed=42)
    e.sync()
    # The generator leaves user_data zero: every 50th account gets user_data_64 = 5 (more than one
    # reply's worth), every 1000th user_data_64 = 7 (fewer).
    host = e.to_host(acct, n_acct * 128).view(ACCOUNT_DTYPE)
    host["user_data_64"][::50] = 5
    host["user_data_64"][::1000] = 7
    e.to_device(acct, host)
    res = e.alloc(max(n_acct, n_xfer) * 8)
    rb = e.alloc((n_xfer // batch + 2) * 4)
    e.commit_device_async(128, a_ts, a_lens, acct, res, rb)
    e.sync()
    spare = e.alloc(n_xfer * 128)
    log = e.log_window(n_xfer)
    e.generate_transfers(log, 0, n_xfer, n_acct, seed=42, kind=KINDS["c2"])
    e.sync()
    x_lens = batches(n_xfer, batch)
    x_ts, t = timestamps(x_lens, t + 10)
    e.commit_device_async(129, x_ts, x_lens, log, res, rb)
    e.sync()
    sample = e.to_host(log + (n_xfer // 2) * 128, 128).view(TRANSFER_DTYPE)
    out = {}
    med, lo_ms, hi_ms = timed(e, lambda: e.copy_device_async(spare, log, n_xfer * 128))
    out["copy_log_d2d"] = copy_log = row(med, lo_ms, hi_ms, bytes=n_xfer * 128)
    for name, flt in (("selective_code_ledger", dict(code=int(sample["code"][0]), ledger=int(sample["ledger"][0]))),
                      ("broad_ledger", dict(ledger=int(sample["ledger"][0])))):
        for rev in (False, True):
            recs, matched, complete = e.query_transfers(reversed=rev, limit=8190, **flt)
            ts = recs["timestamp"].astype(np.int64)
            assert complete and len(recs) == min(matched, 8190) and np.all(np.diff(ts) < 0 if rev else np.diff(ts) > 0)
            med, lo_ms, hi_ms = timed(e, lambda: e.query_transfers(reversed=rev, limit=8190, **flt))
            out["transfers_%s_%s" % (name, "reversed" if rev else "ascending")] = row(
                med, lo_ms, hi_ms, matched=matched, count=len(recs), query_le_copy=med <= copy_log["ms"])
    slots = e.stats()["account_table_bytes"] // 132  # hot 32 + balances 64 + cold 32 + mark 4 per slot
    med, lo_ms, hi_ms = timed(e, lambda: e.copy_device_async(spare, log, slots * 64))
    out["copy_table_d2d"] = copy_table = row(med, lo_ms, hi_ms, bytes=slots * 64, slots=slots)
    for name, flt in (("all_match_ledger", dict(ledger=2)), ("selective_user_data_64", dict(user_data_64=5)),
                      ("few_user_data_64", dict(user_data_64=7))):
        for rev in (False, True):
            recs, matched, complete = e.query_accounts(reversed=rev, limit=8190, **flt)
            ts = recs["timestamp"].astype(np.int64)
            assert complete and len(recs) == min(matched, 8190) and np.all(np.diff(ts) < 0 if rev else np.diff(ts) > 0)
            scans = e.query_select_scans()
            med, lo_ms, hi_ms = timed(e, lambda: e.query_accounts(reversed=rev, limit=8190, **flt))
            out["accounts_%s_%s" % (name, "reversed" if rev else "ascending")] = row(
                med, lo_ms, hi_ms, matched=matched, count=len(recs), select_scans=scans, table_scans=scans + 2,
                ratio_to_copy=round(med / copy_table["ms"], 2))
    e.close()
    return out


def measure_change_events():
    """get_change_events on both logs, beside query_transfers with the same window and the log's copy."""
    os.environ["TBGPU_QUERY_COOP"] = "0"
    e = Engine(Options(accounts_max=n_acct, transfers_max=n_xfer, pass_events_max=pb * batch, pass_batches_max=pb))
    a_lens = batches(n_acct, batch)
    a_ts, t = timestamps(a_lens, 1_000_000_000)
    acct = e.alloc(n_acct * 128)
    e.generate_accounts(acct, 0, n_acct, seed=42)
    res = e.alloc(max(n_acct, n_xfer) * 8)
    rb = e.alloc((n_xfer // batch + 2) * 4)
    e.commit_device_async(128, a_ts, a_lens, acct, res, rb)
    e.sync()
    spare = e.alloc(n_xfer * 128)
    out = {}
    for name, kind in (("uniform", "c2"), ("zipf", "c3")):
        if name != "uniform":
            e.reset_transfers()
        log = e.log_window(n_xfer)
        e.generate_transfers(log, 0, n_xfer, n_acct, seed=42, kind=KINDS[kind])
        e.sync()
        x_lens = batches(n_xfer, batch)
        x_ts, t = timestamps(x_lens, t + 10)
        e.commit_device_async(129, x_ts, x_lens, log, res, rb)
        e.sync()
        if name == "uniform":
            med, lo_ms, hi_ms = timed(e, lambda: e.copy_device_async(spare, log, n_xfer * 128))
            out["copy_log_d2d"] = copy_log = row(med, lo_ms, hi_ms, bytes=n_xfer * 128)
        newest, _, _ = e.query_transfers(reversed=True, limit=2730)
        pages = [("oldest_page", 0)] + ([("newest_page", int(newest["timestamp"][-1]))] if name == "uniform" else [])
        for page, ts_min in pages:
            recs, matched, complete = e.query_transfers(timestamp_min=ts_min, limit=2730)
            events, c_matched, c_complete = e.get_change_events(timestamp_min=ts_min, limit=2730)
            assert complete and c_complete and c_matched == matched and len(events) == len(recs) == 2730
            assert events["transfer"].tobytes() == recs.tobytes()
            ids = set(zip(recs["debit_account_id_lo"].tolist(), recs["debit_account_id_hi"].tolist()))
            ids |= set(zip(recs["credit_account_id_lo"].tolist(), recs["credit_account_id_hi"].tolist()))
            q_med, q_lo, q_hi = timed(e, lambda: e.query_transfers(timestamp_min=ts_min, limit=2730))
            med, lo_ms, hi_ms = timed(e, lambda: e.get_change_events(timestamp_min=ts_min, limit=2730))
            out["%s_%s" % (name, page)] = row(
                med, lo_ms, hi_ms, matched=matched, distinct_accounts=len(ids),
                query_transfers_ms=round(q_med, 4), query_transfers_min_ms=round(q_lo, 4),
                query_transfers_max_ms=round(q_hi, 4), over_query_transfers=round(med / q_med, 2),
                over_copy=round(med / copy_log["ms"], 2), le_copy=med <= copy_log["ms"])
    e.close()
    return out


def measure_many():
    """get_account_transfers_many beside the copy of the log and one single cold query, in one process."""
    import ctypes

    from tigerbeetle_amd import _lib
    os.environ["TBGPU_QUERY_COOP"] = "0"
    e = Engine(Options(accounts_max=n_acct, transfers_max=n_xfer, pass_events_max=pb * batch, pass_batches_max=pb))
    a_lens = batches(n_acct, batch)
    a_ts, t = timestamps(a_lens, 1_000_000_000)
    acct = e.alloc(n_acct * 128)
    e.generate_accounts(acct, 0, n_acct, seed=42)
    res = e.alloc(max(n_acct, n_xfer) * 8)
    rb = e.alloc((n_xfer // batch + 2) * 4)
    e.commit_device_async(128, a_ts, a_lens, acct, res, rb)
    e.sync()
    spare = e.alloc(n_xfer * 128)
    # The caller's buffers are made once, as a replica's are: the timed call is the C call alone.
    h_out = np.zeros((64, 8190), dtype=TRANSFER_DTYPE)
    h_res = (_lib.tbgpu_query_result * 64)()

    def raw_many(filters):
        src = ctypes.create_string_buffer(b"".join(filters), 64 * len(filters))
        return lambda: _lib.check(e.lib.tbgpu_get_account_transfers_many(e.h, src, len(filters), h_out.ctypes.data, 8190, h_res))

    def raw_single(f):
        src = ctypes.create_string_buffer(f, 64)
        return lambda: _lib.check(e.lib.tbgpu_get_account_transfers(e.h, src, h_out.ctypes.data, 8190, h_res))

    def many_row(filters, single_ms):
        want = [e.get_account_transfers_raw(f) for f in filters]
        got = e.get_account_transfers_many(filters)
        assert all(g[0].tobytes() == w[0].tobytes() and g[1:] == w[1:] for g, w in zip(got, want))
        med, lo_ms, hi_ms = timed(e, raw_many(filters))
        return row(med, lo_ms, hi_ms, filters=len(filters), matched=sum(w[1] for w in want), records=sum(len(w[0]) for w in want),
                   per_filter_ms=round(med / len(filters), 4), singles_ms=round(len(filters) * single_ms, 4),
                   speedup_over_singles=round(len(filters) * single_ms / med, 2))

    out = {}
    for name, kind in (("uniform", "c2"), ("zipf", "c3")):
        if name != "uniform":
            e.reset_transfers()
        log = e.log_window(n_xfer)
        e.generate_transfers(log, 0, n_xfer, n_acct, seed=42, kind=KINDS[kind])
        e.sync()
        x_lens = batches(n_xfer, batch)
        x_ts, t = timestamps(x_lens, t + 10)
        e.commit_device_async(129, x_ts, x_lens, log, res, rb)
        e.sync()
        sample = e.to_host(log + (n_xfer // 2) * 128, min(n_xfer // 2, 1 << 16) * 128).view(TRANSFER_DTYPE)
        ids, counts = np.unique(sample[["debit_account_id_lo", "debit_account_id_hi"]], return_counts=True)
        if name == "uniform":
            accounts = [int(lo) | (int(hi) << 64) for lo, hi in ids[:: max(1, len(ids) // 64)][:64]]  # distinct cold accounts
            assert len(set(accounts)) == 64
            cold = [Engine.account_filter(a, limit=8190) for a in accounts]
            med, lo_ms, hi_ms = timed(e, lambda: e.copy_device_async(spare, log, n_xfer * 128))
            out["copy_d2d"] = dict(rates(med), min_ms=round(lo_ms, 4), max_ms=round(hi_ms, 4))
            med, lo_ms, hi_ms = timed(e, lambda: e.get_account_transfers(accounts[0], limit=8190))
            out["single_cold_wrapper"] = dict(rates(med), min_ms=round(lo_ms, 4), max_ms=round(hi_ms, 4))
            med, lo_ms, hi_ms = timed(e, raw_single(cold[0]))
            out["single_cold"] = dict(rates(med), min_ms=round(lo_ms, 4), max_ms=round(hi_ms, 4))
            single_ms = med
            for n in (1, 8, 64):
                out["many_%d_cold" % n] = many_row(cold[:n], single_ms)
            out["many_64_reversed"] = many_row([Engine.account_filter(a, reversed=True, limit=8190) for a in accounts], single_ms)
            out["bar_64_cold_below_64_singles"] = out["many_64_cold"]["ms"] < 64 * single_ms
            for tiles in (8, 16, 32, 64):  # the chunk's length
                e.query_many_tiles(tiles)
                med, lo_ms, hi_ms = timed(e, raw_many(cold))
                out["many_64_cold_tiles_%d" % tiles] = row(med, lo_ms, hi_ms)
            e.query_many_tiles(0)
        else:
            order = np.argsort(-counts)
            accounts = [int(lo) | (int(hi) << 64) for lo, hi in ids[order[:1]]]  # the hottest account ...
            accounts += [int(lo) | (int(hi) << 64) for lo, hi in ids[order[len(order) // 2:][:63]]]  # ... among 63 others
            assert len(set(accounts)) == 64
            hot = [Engine.account_filter(a, limit=8190) for a in accounts]
            med, lo_ms, hi_ms = timed(e, raw_single(hot[0]))
            out["single_hot"] = dict(rates(med), min_ms=round(lo_ms, 4), max_ms=round(hi_ms, 4))
            out["many_64_with_hottest"] = many_row(hot, single_ms)
    e.close()
    return out


def measure_asof():
    """lookup_accounts_at beside get_change_events' oldest page, on both logs, in one process."""
    import ctypes

    from tigerbeetle_amd import _lib
    os.environ["TBGPU_QUERY_COOP"] = "0"
    e = Engine(Options(accounts_max=n_acct, transfers_max=n_xfer, pass_events_max=pb * batch, pass_batches_max=pb))
    a_lens = batches(n_acct, batch)
    a_ts, t = timestamps(a_lens, 1_000_000_000)
    acct = e.alloc(n_acct * 128)
    e.generate_accounts(acct, 0, n_acct, seed=42)
    res = e.alloc(max(n_acct, n_xfer) * 8)
    rb = e.alloc((n_xfer // batch + 2) * 4)
    e.commit_device_async(128, a_ts, a_lens, acct, res, rb)
    e.sync()
    h_out = np.zeros(Engine.LOOKUP_AT_MAX, dtype=ACCOUNT_DTYPE)
    h_res = _lib.tbgpu_query_result()

    def raw_at(ids, T):
        body = b"".join(i.to_bytes(16, "little") for i in ids)
        src = ctypes.create_string_buffer(body, len(body))
        return lambda: _lib.check(e.lib.tbgpu_lookup_accounts_at(e.h, T, src, len(ids), h_out.ctypes.data, len(ids), ctypes.byref(h_res)))

    out = {}
    for name, kind in (("uniform", "c2"), ("zipf", "c3")):
        if name != "uniform":
            e.reset_transfers()
        log = e.log_window(n_xfer)
        e.generate_transfers(log, 0, n_xfer, n_acct, seed=42, kind=KINDS[kind])
        e.sync()
        x_lens = batches(n_xfer, batch)
        x_ts, t = timestamps(x_lens, t + 10)
        e.commit_device_async(129, x_ts, x_lens, log, res, rb)
        e.sync()
        recs, matched, complete = e.query_transfers(limit=2730)
        events, c_matched, c_complete = e.get_change_events(limit=2730)
        assert complete and c_complete and len(events) == len(recs) == 2730
        newest, _, _ = e.query_transfers(reversed=True, limit=1)
        t_old, t_new = int(recs["timestamp"][0]) - 1, int(newest["timestamp"][0])
        page_ids = []
        for f in ("debit_account_id", "credit_account_id"):
            page_ids += [int(lo) | (int(hi) << 64) for lo, hi in zip(recs[f + "_lo"].tolist(), recs[f + "_hi"].tolist())]
        page_ids = list(dict.fromkeys(page_ids))
        # 8,191 ids: the page's accounts first, then distinct accounts of the log's middle.
        sample = e.to_host(log + (n_xfer // 2) * 128, min(n_xfer // 2, 1 << 16) * 128).view(TRANSFER_DTYPE)
        more = [int(lo) | (int(hi) << 64) for lo, hi in zip(sample["debit_account_id_lo"].tolist(), sample["debit_account_id_hi"].tolist())]
        full = list(dict.fromkeys(page_ids + more))[:Engine.LOOKUP_AT_MAX]
        assert len(full) == Engine.LOOKUP_AT_MAX
        # The page's last event is its two accounts at its timestamp; T newer than everything is now.
        last = events[-1]
        pair = [int(last["transfer"][f + "_lo"]) | (int(last["transfer"][f + "_hi"]) << 64) for f in ("debit_account_id", "credit_account_id")]
        got, _, at_complete = e.lookup_accounts_at(pair, int(last["transfer"]["timestamp"]))
        assert at_complete and got[0].tobytes() == last["debit_account"].tobytes() and got[1].tobytes() == last["credit_account"].tobytes()
        now, now_matched, _ = e.lookup_accounts_at(full, 0)
        assert now_matched == len(full) and e.lookup_accounts_at(full, t_new)[0].tobytes() == now.tobytes()
        then, _, _ = e.lookup_accounts_at(full, t_old)
        assert then.tobytes() != now.tobytes()
        q_med, q_lo, q_hi = timed(e, lambda: e.query_transfers(limit=2730))
        c_med, c_lo, c_hi = timed(e, lambda: e.get_change_events(limit=2730))
        second = c_med - q_med
        out["%s_change_events_oldest_page" % name] = row(c_med, c_lo, c_hi, distinct_accounts=len(page_ids),
                                                         query_transfers_ms=round(q_med, 4), query_transfers_min_ms=round(q_lo, 4),
                                                         query_transfers_max_ms=round(q_hi, 4), second_pass_ms=round(second, 4))
        for leg, ids, T in (("page_ids_t_old", page_ids, t_old), ("page_ids_t_new", page_ids, t_new),
                            ("8191_ids_t_old", full, t_old), ("8191_ids_t_new", full, t_new), ("8191_ids_now", full, 0)):
            med, lo_ms, hi_ms = timed(e, raw_at(ids, T))
            out["%s_asof_%s" % (name, leg)] = row(med, lo_ms, hi_ms, ids=len(ids), over_second_pass=round(med / second, 2))
    e.close()
    return out


def measure_statements():
    """get_account_statements beside two lookup_accounts_at calls with the same ids, on both logs, in one process."""
    import ctypes

    from tigerbeetle_amd import _lib
    os.environ["TBGPU_QUERY_COOP"] = "0"
    e = Engine(Options(accounts_max=n_acct, transfers_max=n_xfer, pass_events_max=pb * batch, pass_batches_max=pb))
    a_lens = batches(n_acct, batch)
    a_ts, t = timestamps(a_lens, 1_000_000_000)
    acct = e.alloc(n_acct * 128)
    e.generate_accounts(acct, 0, n_acct, seed=42)
    res = e.alloc(max(n_acct, n_xfer) * 8)
    rb = e.alloc((n_xfer // batch + 2) * 4)
    e.commit_device_async(128, a_ts, a_lens, acct, res, rb)
    e.sync()
    n_ids = 4095
    have = hasattr(e.lib, "tbgpu_get_account_statements")  # an older library (TBGPU_AB_LIB): the yardstick alone
    h_out = np.zeros(n_ids * 256, dtype=np.uint8)
    h_res = _lib.tbgpu_query_result()

    def raw(ids, t_open, t_close):
        body = b"".join(i.to_bytes(16, "little") for i in ids)
        src = ctypes.create_string_buffer(body, len(body))
        return lambda: _lib.check(e.lib.tbgpu_get_account_statements(e.h, t_open, t_close, src, len(ids), h_out.ctypes.data, len(ids),
                                                                      ctypes.byref(h_res)))

    def raw_two(ids, t_open, t_close):
        body = b"".join(i.to_bytes(16, "little") for i in ids)
        src = ctypes.create_string_buffer(body, len(body))

        def both():
            for T in (t_open, t_close):
                _lib.check(e.lib.tbgpu_lookup_accounts_at(e.h, T, src, len(ids), h_out.ctypes.data, len(ids), ctypes.byref(h_res)))
        return both

    out = {}
    for name, kind in (("uniform", "c2"), ("zipf", "c3")):
        if name != "uniform":
            e.reset_transfers()
        log = e.log_window(n_xfer)
        e.generate_transfers(log, 0, n_xfer, n_acct, seed=42, kind=KINDS[kind])
        e.sync()
        x_lens = batches(n_xfer, batch)
        x_ts, t = timestamps(x_lens, t + 10)
        e.commit_device_async(129, x_ts, x_lens, log, res, rb)
        e.sync()
        oldest, _, _ = e.query_transfers(limit=1)
        newest, _, _ = e.query_transfers(reversed=True, limit=1)
        t_first, t_last = int(oldest["timestamp"][0]), int(newest["timestamp"][0])
        quarter = (t_last - t_first) // 4
        sample = e.to_host(log + (n_xfer // 2) * 128, min(n_xfer // 2, 1 << 16) * 128).view(TRANSFER_DTYPE)
        accounts, counts = np.unique(sample[["debit_account_id_lo", "debit_account_id_hi"]], return_counts=True)
        hottest = np.argsort(-counts, kind="stable")[:n_ids]  # the Zipf log's hottest accounts; any of the uniform log's
        ids = [int(lo) | (int(hi) << 64) for lo, hi in accounts[hottest].tolist()]
        assert len(ids) == n_ids
        legs = (("whole_log", t_first - 1, t_last), ("middle_half", t_first + quarter, t_last - quarter),
                ("t_open_above_every_record", t_last, 0))
        if have:
            rows, matched, complete = e.get_account_statements(ids, t_first - 1, t_last)
            assert complete and matched == n_ids and int(rows["debit_transfers"].sum()) > n_ids
            at_close = e.lookup_accounts_at(ids, t_last - quarter)[0]
            at_open = e.lookup_accounts_at(ids, t_first + quarter)[0]
            rows, _, _ = e.get_account_statements(ids, t_first + quarter, t_last - quarter)
            for c in ("debits_pending", "debits_posted", "credits_pending", "credits_posted"):
                for w in ("_lo", "_hi"):
                    assert np.array_equal(rows["closing_" + c + w], at_close[c + w]) and np.array_equal(rows["opening_" + c + w], at_open[c + w])
        for leg, t_open, t_close in legs:
            two_med, two_lo, two_hi = timed(e, raw_two(ids, t_open, t_close))
            entry = dict(ids=n_ids, two_lookups_ms=round(two_med, 4), two_lookups_min_ms=round(two_lo, 4), two_lookups_max_ms=round(two_hi, 4))
            if have:
                med, lo_ms, hi_ms = timed(e, raw(ids, t_open, t_close))
                entry = row(med, lo_ms, hi_ms, over_two_lookups=round(med / two_med, 2), **entry)
            out["%s_statements_%s" % (name, leg)] = entry
    e.close()
    return out


def measure_integrals():
    """get_account_balance_integrals beside get_account_statements with the same ids, on both logs, in one process."""
    import ctypes

    from tigerbeetle_amd import _lib
    os.environ["TBGPU_QUERY_COOP"] = "0"
    e = Engine(Options(accounts_max=n_acct, transfers_max=n_xfer, pass_events_max=pb * batch, pass_batches_max=pb))
    a_lens = batches(n_acct, batch)
    a_ts, t = timestamps(a_lens, 1_000_000_000)
    acct = e.alloc(n_acct * 128)
    e.generate_accounts(acct, 0, n_acct, seed=42)
    res = e.alloc(max(n_acct, n_xfer) * 8)
    rb = e.alloc((n_xfer // batch + 2) * 4)
    e.commit_device_async(128, a_ts, a_lens, acct, res, rb)
    e.sync()
    n_ids = 4095
    have = hasattr(e.lib, "tbgpu_get_account_balance_integrals")  # an older library (TBGPU_AB_LIB): the yardstick alone
    h_out = np.zeros(n_ids * 256, dtype=np.uint8)
    h_res = _lib.tbgpu_query_result()

    def raw(fn, ids, t_open, t_close):
        body = b"".join(i.to_bytes(16, "little") for i in ids)
        src = ctypes.create_string_buffer(body, len(body))
        return lambda: _lib.check(fn(e.h, t_open, t_close, src, len(ids), h_out.ctypes.data, len(ids), ctypes.byref(h_res)))

    out = {}
    for name, kind in (("uniform", "c2"), ("zipf", "c3")):
        if name != "uniform":
            e.reset_transfers()
        log = e.log_window(n_xfer)
        e.generate_transfers(log, 0, n_xfer, n_acct, seed=42, kind=KINDS[kind])
        e.sync()
        x_lens = batches(n_xfer, batch)
        x_ts, t = timestamps(x_lens, t + 10)
        e.commit_device_async(129, x_ts, x_lens, log, res, rb)
        e.sync()
        oldest, _, _ = e.query_transfers(limit=1)
        newest, _, _ = e.query_transfers(reversed=True, limit=1)
        t_first, t_last = int(oldest["timestamp"][0]), int(newest["timestamp"][0])
        quarter = (t_last - t_first) // 4
        sample = e.to_host(log + (n_xfer // 2) * 128, min(n_xfer // 2, 1 << 16) * 128).view(TRANSFER_DTYPE)
        accounts, counts = np.unique(sample[["debit_account_id_lo", "debit_account_id_hi"]], return_counts=True)
        hottest = np.argsort(-counts, kind="stable")[:n_ids]  # the Zipf log's hottest accounts; any of the uniform log's
        ids = [int(lo) | (int(hi) << 64) for lo, hi in accounts[hottest].tolist()]
        assert len(ids) == n_ids
        legs = (("whole_log", t_first - 1, t_last), ("middle_half", t_first + quarter, t_last - quarter),
                ("t_open_above_every_record", t_last, t_last + 1))
        if have:
            rows, matched, complete = e.get_account_balance_integrals(ids, t_first + quarter, t_last - quarter)
            held = e.get_account_statements(ids, t_first + quarter, t_last - quarter)[0]
            assert complete and matched == n_ids and int(rows["integral_debits_posted_w0"].astype(bool).sum()) > n_ids // 2
            for c in ("debits_pending", "debits_posted", "credits_pending", "credits_posted"):
                for when in ("opening_", "closing_"):
                    for w in ("_lo", "_hi"):
                        assert np.array_equal(rows[when + c + w], held[when + c + w])
        for leg, t_open, t_close in legs:
            st_med, st_lo, st_hi = timed(e, raw(e.lib.tbgpu_get_account_statements, ids, t_open, t_close))
            entry = dict(ids=n_ids, statements_ms=round(st_med, 4), statements_min_ms=round(st_lo, 4), statements_max_ms=round(st_hi, 4))
            if have:
                med, lo_ms, hi_ms = timed(e, raw(e.lib.tbgpu_get_account_balance_integrals, ids, t_open, t_close))
                entry = row(med, lo_ms, hi_ms, over_statements=round(med / st_med, 2), **entry)
            out["%s_integrals_%s" % (name, leg)] = entry
    e.close()
    return out


def measure_extremes():
    """get_account_balance_extremes beside get_account_statements — the order-free yardstick for what ordering
    costs — with the same ids and period, on both logs, in one process; then engines made under the call's knobs:
    the walk cut into at most 256, 64, 16 and 1 slabs (n = 4,095, the whole log), and the exact path, what a caller
    has today (n = 1 hottest and n = 64, three runs each: it pages the account's history)."""
    import ctypes

    from tigerbeetle_amd import _lib
    from tigerbeetle_amd.types import MEASURE_CREDIT_NET_POSTED, pack_balance_measure
    os.environ["TBGPU_QUERY_COOP"] = "0"
    n_ids = 4095
    h_out = np.zeros(n_ids * 256, dtype=np.uint8)
    h_res = _lib.tbgpu_query_result()
    measure = ctypes.create_string_buffer(pack_balance_measure(MEASURE_CREDIT_NET_POSTED), 8)
    out = {}

    def engine_of(exact, slabs):
        os.environ["TBGPU_EXTREMES_EXACT"] = "1" if exact else "0"
        os.environ.pop("TBGPU_EXTREMES_SLABS", None)
        if slabs:
            os.environ["TBGPU_EXTREMES_SLABS"] = str(slabs)
        e = Engine(Options(accounts_max=n_acct, transfers_max=n_xfer, pass_events_max=pb * batch, pass_batches_max=pb))
        a_lens = batches(n_acct, batch)
        a_ts, t = timestamps(a_lens, 1_000_000_000)
        acct = e.alloc(n_acct * 128)
        e.generate_accounts(acct, 0, n_acct, seed=42)
        res = e.alloc(max(n_acct, n_xfer) * 8)
        rb = e.alloc((n_xfer // batch + 2) * 4)
        e.commit_device_async(128, a_ts, a_lens, acct, res, rb)
        e.sync()
        return e, res, rb, t

    def fill(e, res, rb, t, name, kind):
        if name != "uniform":
            e.reset_transfers()
        log = e.log_window(n_xfer)
        e.generate_transfers(log, 0, n_xfer, n_acct, seed=42, kind=KINDS[kind])
        e.sync()
        x_lens = batches(n_xfer, batch)
        x_ts, t = timestamps(x_lens, t + 10)
        e.commit_device_async(129, x_ts, x_lens, log, res, rb)
        e.sync()
        oldest, _, _ = e.query_transfers(limit=1)
        newest, _, _ = e.query_transfers(reversed=True, limit=1)
        t_first, t_last = int(oldest["timestamp"][0]), int(newest["timestamp"][0])
        sample = e.to_host(log + (n_xfer // 2) * 128, min(n_xfer // 2, 1 << 16) * 128).view(TRANSFER_DTYPE)
        accounts, counts = np.unique(sample[["debit_account_id_lo", "debit_account_id_hi"]], return_counts=True)
        order = np.argsort(-counts, kind="stable")
        ids = [int(lo) | (int(hi) << 64) for lo, hi in accounts[order[:n_ids]].tolist()]
        cold = [int(lo) | (int(hi) << 64) for lo, hi in accounts[order[-1:]].tolist()]
        assert len(ids) == n_ids
        return t, t_first, t_last, ids, cold

    def raw(e, fn, ids, t_open, t_close, with_measure):
        body = b"".join(i.to_bytes(16, "little") for i in ids)
        src = ctypes.create_string_buffer(body, len(body))
        if with_measure:
            return lambda: _lib.check(fn(e.h, t_open, t_close, measure, src, len(ids), h_out.ctypes.data, len(ids), ctypes.byref(h_res)))
        return lambda: _lib.check(fn(e.h, t_open, t_close, src, len(ids), h_out.ctypes.data, len(ids), ctypes.byref(h_res)))

    def few(e, fn, n=3):
        took = []
        for i in range(1 + n):
            e.marker(0)
            fn()
            e.marker(1)
            e.sync()
            if i:
                took.append(e.marker_elapsed_ms(0, 1))
        return statistics.median(took), min(took), max(took)

    e, res, rb, t = engine_of(False, 0)
    for name, kind in (("uniform", "c2"), ("zipf", "c3")):
        t, t_first, t_last, ids, cold = fill(e, res, rb, t, name, kind)
        quarter = (t_last - t_first) // 4
        rows, matched, complete = e.get_account_balance_extremes(ids, t_first + quarter, t_last - quarter, MEASURE_CREDIT_NET_POSTED)
        assert complete and matched == n_ids and int(rows["records"].sum()) > n_ids // 2
        for who, request in (("1_cold", cold), ("1_hottest", ids[:1]), ("64", ids[:64]), ("4095", ids)):
            for leg, t_open, t_close in (("whole_log", t_first - 1, t_last), ("middle_half", t_first + quarter, t_last - quarter)):
                st_med, st_lo, st_hi = timed(e, raw(e, e.lib.tbgpu_get_account_statements, request, t_open, t_close, False))
                med, lo_ms, hi_ms = timed(e, raw(e, e.lib.tbgpu_get_account_balance_extremes, request, t_open, t_close, True))
                out["%s_extremes_%s_%s" % (name, who, leg)] = row(med, lo_ms, hi_ms, ids=len(request), statements_ms=round(st_med, 4),
                                                                   statements_min_ms=round(st_lo, 4), statements_max_ms=round(st_hi, 4),
                                                                   over_statements=round(med / st_med, 2))
    e.close()
    for slabs in (256, 64, 16, 1):
        e, res, rb, t = engine_of(False, slabs)
        for name, kind in (("uniform", "c2"), ("zipf", "c3")):
            t, t_first, t_last, ids, cold = fill(e, res, rb, t, name, kind)
            med, lo_ms, hi_ms = (few if slabs == 1 else timed)(e, raw(e, e.lib.tbgpu_get_account_balance_extremes, ids, t_first - 1, t_last, True))
            out["%s_extremes_4095_whole_log_slabs_%d" % (name, slabs)] = row(med, lo_ms, hi_ms, ids=n_ids, slabs_cap=slabs)
        e.close()
    if "--skip-exact" not in sys.argv:
        e, res, rb, t = engine_of(True, 0)
        for name, kind in (("uniform", "c2"), ("zipf", "c3")):
            t, t_first, t_last, ids, cold = fill(e, res, rb, t, name, kind)
            for who, request in (("1_hottest", ids[:1]), ("64", ids[:64])):
                med, lo_ms, hi_ms = few(e, raw(e, e.lib.tbgpu_get_account_balance_extremes, request, t_first - 1, t_last, True))
                out["%s_extremes_%s_whole_log_exact_path" % (name, who)] = row(med, lo_ms, hi_ms, ids=len(request), runs=3)
        e.close()
    return out


def measure_series():
    """get_account_statement_series beside the same question asked as n_buckets get_account_statements calls
    and beside one such call over the whole period, on both logs, in one process."""
    import ctypes

    from tigerbeetle_amd import _lib
    os.environ["TBGPU_QUERY_COOP"] = "0"
    e = Engine(Options(accounts_max=n_acct, transfers_max=n_xfer, pass_events_max=pb * batch, pass_batches_max=pb))
    a_lens = batches(n_acct, batch)
    a_ts, t = timestamps(a_lens, 1_000_000_000)
    acct = e.alloc(n_acct * 128)
    e.generate_accounts(acct, 0, n_acct, seed=42)
    res = e.alloc(max(n_acct, n_xfer) * 8)
    rb = e.alloc((n_xfer // batch + 2) * 4)
    e.commit_device_async(128, a_ts, a_lens, acct, res, rb)
    e.sync()
    rows_max = 4095
    have = hasattr(e.lib, "tbgpu_get_account_statement_series")  # an older library (TBGPU_AB_LIB): the single calls alone
    h_out = np.zeros(rows_max * 256, dtype=np.uint8)
    h_res = _lib.tbgpu_query_result()

    def raw_series(ids, bounds):
        body = b"".join(i.to_bytes(16, "little") for i in ids)
        src = ctypes.create_string_buffer(body, len(body))
        edges = (ctypes.c_uint64 * len(bounds))(*bounds)
        return lambda: _lib.check(e.lib.tbgpu_get_account_statement_series(e.h, edges, len(bounds) - 1, src, len(ids), h_out.ctypes.data,
                                                                           rows_max, ctypes.byref(h_res)))

    def raw_singles(ids, bounds):
        body = b"".join(i.to_bytes(16, "little") for i in ids)
        src = ctypes.create_string_buffer(body, len(body))

        def each():
            for t_open, t_close in zip(bounds, bounds[1:]):
                _lib.check(e.lib.tbgpu_get_account_statements(e.h, t_open, t_close, src, len(ids), h_out.ctypes.data, len(ids),
                                                              ctypes.byref(h_res)))
        return each

    def timed_few(fn, warmups, n):  # the long single-call loops: fewer runs
        out = []
        for i in range(warmups + n):
            e.marker(0)
            fn()
            e.marker(1)
            e.sync()
            if i >= warmups:
                out.append(e.marker_elapsed_ms(0, 1))
        return statistics.median(out), min(out), max(out)

    out = {}
    for name, kind in (("uniform", "c2"), ("zipf", "c3")):
        if name != "uniform":
            e.reset_transfers()
        log = e.log_window(n_xfer)
        e.generate_transfers(log, 0, n_xfer, n_acct, seed=42, kind=KINDS[kind])
        e.sync()
        x_lens = batches(n_xfer, batch)
        x_ts, t = timestamps(x_lens, t + 10)
        e.commit_device_async(129, x_ts, x_lens, log, res, rb)
        e.sync()
        oldest, _, _ = e.query_transfers(limit=1)
        newest, _, _ = e.query_transfers(reversed=True, limit=1)
        t_first, t_last = int(oldest["timestamp"][0]), int(newest["timestamp"][0])
        sample = e.to_host(log + (n_xfer // 2) * 128, min(n_xfer // 2, 1 << 16) * 128).view(TRANSFER_DTYPE)
        accounts, counts = np.unique(sample[["debit_account_id_lo", "debit_account_id_hi"]], return_counts=True)
        hottest = np.argsort(-counts, kind="stable")[:rows_max]  # the Zipf log's hottest accounts; any of the uniform log's
        all_ids = [int(lo) | (int(hi) << 64) for lo, hi in accounts[hottest].tolist()]
        assert len(all_ids) == rows_max
        for n_ids, n_buckets in ((4095, 1), (136, 30), (11, 365), (1, 4095)):
            ids = all_ids[:n_ids]
            bounds = [t_first - 1 + (t_last - t_first + 1) * k // n_buckets for k in range(n_buckets + 1)]
            assert bounds[-1] == t_last and all(a < b for a, b in zip(bounds, bounds[1:]))
            if have:
                rows, matched, complete = e.get_account_statement_series(ids, bounds)
                assert complete and matched == n_ids * n_buckets == len(rows) and int(rows["debit_transfers"].sum()) > 0
                for k in sorted({0, n_buckets // 2, n_buckets - 1}):
                    assert rows[k::n_buckets].tobytes() == e.get_account_statements(ids, bounds[k], bounds[k + 1])[0].tobytes()
            few = n_buckets >= 365
            s_med, s_lo, s_hi = timed_few(raw_singles(ids, bounds), 1, 3) if few else timed(e, raw_singles(ids, bounds))
            w_med, w_lo, w_hi = timed(e, raw_singles(ids, [bounds[0], bounds[-1]]))
            entry = dict(ids=n_ids, buckets=n_buckets, single_calls_ms=round(s_med, 4), single_calls_min_ms=round(s_lo, 4),
                         single_calls_max_ms=round(s_hi, 4), single_calls_runs=3 if few else runs, whole_period_call_ms=round(w_med, 4),
                         whole_period_call_min_ms=round(w_lo, 4), whole_period_call_max_ms=round(w_hi, 4))
            if have:
                med, lo_ms, hi_ms = timed(e, raw_series(ids, bounds))
                entry = row(med, lo_ms, hi_ms, over_single_calls=round(med / s_med, 4), over_whole_period_call=round(med / w_med, 2),
                            **entry)
            out["%s_series_%d_x_%d" % (name, n_ids, n_buckets)] = entry
    e.close()
    return out


def measure_matrix():
    """get_account_flow_matrix beside get_account_statements over the same ids and period, on both logs, in one
    process; and the host alternative for one leg."""
    import ctypes
    import time

    from tigerbeetle_amd import _lib
    os.environ["TBGPU_QUERY_COOP"] = "0"
    e = Engine(Options(accounts_max=n_acct, transfers_max=n_xfer, pass_events_max=pb * batch, pass_batches_max=pb))
    a_lens = batches(n_acct, batch)
    a_ts, t = timestamps(a_lens, 1_000_000_000)
    acct = e.alloc(n_acct * 128)
    e.generate_accounts(acct, 0, n_acct, seed=42)
    res = e.alloc(max(n_acct, n_xfer) * 8)
    rb = e.alloc((n_xfer // batch + 2) * 4)
    e.commit_device_async(128, a_ts, a_lens, acct, res, rb)
    e.sync()
    cells_max = 4095
    have = hasattr(e.lib, "tbgpu_get_account_flow_matrix")  # an older library (TBGPU_AB_LIB): the yardstick alone
    h_out = np.zeros(cells_max * 256, dtype=np.uint8)
    h_res = _lib.tbgpu_query_result()
    body_of = lambda ids: b"".join(i.to_bytes(16, "little") for i in ids)

    def raw_matrix(debit, credit, t_open, t_close):
        d_src = ctypes.create_string_buffer(body_of(debit), 16 * len(debit))
        c_src = ctypes.create_string_buffer(body_of(credit), 16 * len(credit))
        return lambda: _lib.check(e.lib.tbgpu_get_account_flow_matrix(e.h, t_open, t_close, d_src, len(debit), c_src, len(credit),
                                                                      h_out.ctypes.data, cells_max, ctypes.byref(h_res)))

    def raw_statements(ids, t_open, t_close):
        src = ctypes.create_string_buffer(body_of(ids), 16 * len(ids))
        return lambda: _lib.check(e.lib.tbgpu_get_account_statements(e.h, t_open, t_close, src, len(ids), h_out.ctypes.data, len(ids),
                                                                      ctypes.byref(h_res)))

    def paged(debit, credit, t_open, t_close):
        """The host alternative: {(d, c): records}, from every debit account's pages of its debit side."""
        wanted, groups = set(credit), {}
        for d in debit:
            t_min = t_open + 1
            while True:
                page, _, _ = e.get_account_transfers(d, credits=False, timestamp_min=t_min, timestamp_max=t_close, limit=8190)
                for lo, hi in zip(page["credit_account_id_lo"].tolist(), page["credit_account_id_hi"].tolist()):
                    c = lo | hi << 64
                    if c in wanted:
                        groups[(d, c)] = groups.get((d, c), 0) + 1
                if len(page) < 8190:
                    break
                t_min = int(page["timestamp"][-1]) + 1
        return groups

    out = {}
    for name, kind in (("uniform", "c2"), ("zipf", "c3")):
        if name != "uniform":
            e.reset_transfers()
        log = e.log_window(n_xfer)
        e.generate_transfers(log, 0, n_xfer, n_acct, seed=42, kind=KINDS[kind])
        e.sync()
        x_lens = batches(n_xfer, batch)
        x_ts, t = timestamps(x_lens, t + 10)
        e.commit_device_async(129, x_ts, x_lens, log, res, rb)
        e.sync()
        oldest, _, _ = e.query_transfers(limit=1)
        newest, _, _ = e.query_transfers(reversed=True, limit=1)
        t_first, t_last = int(oldest["timestamp"][0]), int(newest["timestamp"][0])
        quarter = (t_last - t_first) // 4
        sample = e.to_host(log + (n_xfer // 2) * 128, min(n_xfer // 2, 1 << 16) * 128).view(TRANSFER_DTYPE)
        accounts, counts = np.unique(sample[["debit_account_id_lo", "debit_account_id_hi"]], return_counts=True)
        hottest = np.argsort(-counts, kind="stable")[:cells_max]  # the Zipf log's hottest accounts; any of the uniform log's
        hot = [int(lo) | (int(hi) << 64) for lo, hi in accounts[hottest].tolist()]
        assert len(hot) == cells_max
        pick = np.random.default_rng(7).choice(len(accounts), 63, replace=False)
        anyone = [int(lo) | (int(hi) << 64) for lo, hi in accounts[pick].tolist()]
        shapes = (("hot_63_x_63", hot[:63], hot[:63]), ("random_63_x_63", anyone, anyone), ("1_x_4095", hot[:1], hot),
                  ("4095_x_1", hot, hot[:1]))
        periods = (("whole_log", t_first - 1, t_last), ("middle_half", t_first + quarter, t_last - quarter))
        for shape, debit, credit in shapes:
            ids = list(dict.fromkeys(debit + credit))[:cells_max]
            for leg, t_open, t_close in periods:
                y_med, y_lo, y_hi = timed(e, raw_statements(ids, t_open, t_close))
                entry = dict(debit_ids=len(debit), credit_ids=len(credit), statements_ms=round(y_med, 4), statements_min_ms=round(y_lo, 4),
                             statements_max_ms=round(y_hi, 4))
                if have:
                    cells, matched, complete = e.get_account_flow_matrix(debit, credit, t_open, t_close)
                    assert complete and matched == len(debit) * len(credit) == len(cells)
                    med, lo_ms, hi_ms = timed(e, raw_matrix(debit, credit, t_open, t_close))
                    entry = row(med, lo_ms, hi_ms, over_statements=round(med / y_med, 2), records_in_cells=int(cells["transfers"].sum()),
                                **entry)
                    if shape == "hot_63_x_63" and leg == "whole_log":
                        start = time.perf_counter()
                        groups = paged(debit, credit, t_open, t_close)
                        entry["paged_on_host_ms"] = round((time.perf_counter() - start) * 1e3, 1)
                        entry["over_paged_on_host"] = round(med / entry["paged_on_host_ms"], 5)
                        mine = {}
                        for c in cells[cells["transfers"] > 0]:
                            key = (int(c["debit_id_lo"]) | int(c["debit_id_hi"]) << 64, int(c["credit_id_lo"]) | int(c["credit_id_hi"]) << 64)
                            mine[key] = int(c["transfers"])
                        assert mine == groups, (len(mine), len(groups))
                        entry["cells_with_records"] = len(mine)
                out["%s_matrix_%s_%s" % (name, shape, leg)] = entry
    e.close()
    return out


def measure_counterparties():
    """get_account_counterparties beside get_account_statements for the same account and period, and beside the
    account's pages grouped on the host, on both logs, in one process."""
    import ctypes
    import time

    from tigerbeetle_amd import _lib
    from tigerbeetle_amd.types import pack_counterparty_filter
    os.environ["TBGPU_QUERY_COOP"] = "0"
    e = Engine(Options(accounts_max=n_acct, transfers_max=n_xfer, pass_events_max=pb * batch, pass_batches_max=pb))
    a_lens = batches(n_acct, batch)
    a_ts, t = timestamps(a_lens, 1_000_000_000)
    acct = e.alloc(n_acct * 128)
    e.generate_accounts(acct, 0, n_acct, seed=42)
    res = e.alloc(max(n_acct, n_xfer) * 8)
    rb = e.alloc((n_xfer // batch + 2) * 4)
    e.commit_device_async(128, a_ts, a_lens, acct, res, rb)
    e.sync()
    rows_max = 8191
    have = hasattr(e.lib, "tbgpu_get_account_counterparties")  # an older library (TBGPU_AB_LIB): the yardsticks alone
    h_out = np.zeros(rows_max * 256, dtype=np.uint8)
    h_res = _lib.tbgpu_query_result()

    def raw_counterparties(account, t_open, t_close, limit, by_volume):
        f = pack_counterparty_filter(account, t_open, t_close, 0, limit, 3 | (256 if by_volume else 0))
        src = ctypes.create_string_buffer(f, 64)
        return lambda: _lib.check(e.lib.tbgpu_get_account_counterparties(e.h, src, h_out.ctypes.data, rows_max, ctypes.byref(h_res)))

    def raw_statements(account, t_open, t_close):
        src = ctypes.create_string_buffer(account.to_bytes(16, "little"), 16)
        return lambda: _lib.check(e.lib.tbgpu_get_account_statements(e.h, t_open, t_close, src, 1, h_out.ctypes.data, 1, ctypes.byref(h_res)))

    def paged(account, t_open, t_close):
        """The host alternative: {counterparty: [records to it, records from it]}, from the account's pages."""
        groups = {}
        t_min = t_open + 1
        while True:
            page, _, _ = e.get_account_transfers(account, timestamp_min=t_min, timestamp_max=t_close, limit=8190)
            ids = zip(page["debit_account_id_lo"].tolist(), page["debit_account_id_hi"].tolist(), page["credit_account_id_lo"].tolist(),
                      page["credit_account_id_hi"].tolist())
            for dl, dh, cl, ch in ids:
                d, c = dl | dh << 64, cl | ch << 64
                if d == account:
                    groups.setdefault(c, [0, 0])[0] += 1
                if c == account:
                    groups.setdefault(d, [0, 0])[1] += 1
            if len(page) < 8190:
                break
            t_min = int(page["timestamp"][-1]) + 1
        return groups

    out = {}
    if have:
        out["group_table_bytes"] = 128 * (1 << (2 * n_acct - 1).bit_length())  # 128-B slots, 2 x accounts_max rounded up to a power of two
    for name, kind in (("uniform", "c2"), ("zipf", "c3")):
        if name != "uniform":
            e.reset_transfers()
        log = e.log_window(n_xfer)
        e.generate_transfers(log, 0, n_xfer, n_acct, seed=42, kind=KINDS[kind])
        e.sync()
        x_lens = batches(n_xfer, batch)
        x_ts, t = timestamps(x_lens, t + 10)
        e.commit_device_async(129, x_ts, x_lens, log, res, rb)
        e.sync()
        oldest, _, _ = e.query_transfers(limit=1)
        newest, _, _ = e.query_transfers(reversed=True, limit=1)
        t_first, t_last = int(oldest["timestamp"][0]), int(newest["timestamp"][0])
        sample = e.to_host(log + (n_xfer // 2) * 128, min(n_xfer // 2, 1 << 16) * 128).view(TRANSFER_DTYPE)
        accounts, counts = np.unique(sample[["debit_account_id_lo", "debit_account_id_hi"]], return_counts=True)
        order = np.argsort(-counts, kind="stable")
        id_at = lambda k: int(accounts[order[k]][0]) | (int(accounts[order[k]][1]) << 64)
        subjects = (("hot", id_at(0)), ("cold", id_at(len(order) - 1))) if name == "zipf" else (("account", id_at(0)),)
        for who, account in subjects:
            t_open, t_close = t_first - 1, t_last
            y_med, y_lo, y_hi = timed(e, raw_statements(account, t_open, t_close))
            start = time.perf_counter()
            groups = paged(account, t_open, t_close)
            paged_ms = round((time.perf_counter() - start) * 1e3, 1)
            base = dict(statements_ms=round(y_med, 4), statements_min_ms=round(y_lo, 4), statements_max_ms=round(y_hi, 4),
                        paged_on_host_ms=paged_ms, groups=len(groups), records=sum(a + b for a, b in groups.values()))
            if not have:
                out["%s_counterparties_%s" % (name, who)] = base
                continue
            rows, matched, complete = e.get_account_counterparties(account, t_open, t_close)
            assert complete and matched == len(groups)
            mine = {int(r["id_lo"]) | int(r["id_hi"]) << 64: [int(r["to_transfers"]), int(r["from_transfers"])] for r in rows}
            assert all(groups[x] == v for x, v in mine.items()) and len(mine) == min(matched, rows_max)
            for order_name, by_volume in (("by_id", False), ("by_volume", True)):
                for limit in (10, rows_max):
                    med, lo_ms, hi_ms = timed(e, raw_counterparties(account, t_open, t_close, limit, by_volume))
                    out["%s_counterparties_%s_%s_limit_%d" % (name, who, order_name, limit)] = row(
                        med, lo_ms, hi_ms, over_statements=round(med / y_med, 2), over_paged_on_host=round(med / paged_ms, 5), **base)
            # The fixed cost: the same call over an empty period (the scan reads timestamps only).
            y_med, y_lo, y_hi = timed(e, raw_statements(account, t_last, t_last + 1))
            for order_name, by_volume in (("by_id", False), ("by_volume", True)):
                med, lo_ms, hi_ms = timed(e, raw_counterparties(account, t_last, t_last + 1, rows_max, by_volume))
                out["%s_counterparties_%s_%s_empty_period" % (name, who, order_name)] = row(
                    med, lo_ms, hi_ms, statements_ms=round(y_med, 4), statements_min_ms=round(y_lo, 4), statements_max_ms=round(y_hi, 4),
                    over_statements=round(med / y_med, 2))
    e.close()
    return out


def measure_activity():
    """get_active_accounts beside query_transfers over the same window, get_account_counterparties and the log's
    copy, on three logs, in one process."""
    import ctypes
    import time

    from tigerbeetle_amd import _lib
    from tigerbeetle_amd.types import pack_counterparty_filter
    os.environ["TBGPU_QUERY_COOP"] = "0"
    e = Engine(Options(accounts_max=n_acct, transfers_max=n_xfer, pass_events_max=pb * batch, pass_batches_max=pb))
    a_lens = batches(n_acct, batch)
    a_ts, t = timestamps(a_lens, 1_000_000_000)
    acct = e.alloc(n_acct * 128)
    e.generate_accounts(acct, 0, n_acct, seed=42)
    res = e.alloc(max(n_acct, n_xfer) * 8)
    rb = e.alloc((n_xfer // batch + 2) * 4)
    e.commit_device_async(128, a_ts, a_lens, acct, res, rb)
    e.sync()
    spare = e.alloc(n_xfer * 128)
    rows_max = 8191
    have = hasattr(e.lib, "tbgpu_get_active_accounts")  # an older library (TBGPU_AB_LIB): the yardsticks alone
    h_out = np.zeros(rows_max * 128, dtype=np.uint8)
    h_recs = np.zeros(8190, dtype=TRANSFER_DTYPE)
    h_res = _lib.tbgpu_query_result()

    def raw_active(t_open, t_close, limit, order=0, ledger=0, code=0):
        from tigerbeetle_amd.types import pack_activity_filter
        f = pack_activity_filter(t_open, t_close, 0, ledger, code, limit, 3 | order)
        src = ctypes.create_string_buffer(f, 64)
        return lambda: _lib.check(e.lib.tbgpu_get_active_accounts(e.h, src, h_out.ctypes.data, rows_max, ctypes.byref(h_res)))

    def raw_counterparties(account, t_open, t_close, limit):
        f = pack_counterparty_filter(account, t_open, t_close, 0, limit, 3)
        src = ctypes.create_string_buffer(f, 64)
        return lambda: _lib.check(e.lib.tbgpu_get_account_counterparties(e.h, src, h_out.ctypes.data, rows_max, ctypes.byref(h_res)))

    def raw_query(**filter):
        f = Engine.query_filter(**filter)
        src = ctypes.create_string_buffer(f, len(f))
        return lambda: _lib.check(e.lib.tbgpu_query_transfers(e.h, src, h_recs.ctypes.data, 8190, ctypes.byref(h_res)))

    def paged(t_open):
        """The host alternative: {account: records that name it}, from the whole log's pages."""
        names = []
        t_min = t_open + 1
        while True:
            page, _, _ = e.query_transfers(timestamp_min=t_min, limit=8190)
            for side in ("debit_account_id", "credit_account_id"):
                names.append(np.stack([page[side + "_lo"], page[side + "_hi"]], axis=1))
            if len(page) < 8190:
                break
            t_min = int(page["timestamp"][-1]) + 1
        ids, counts = np.unique(np.concatenate(names), axis=0, return_counts=True)
        return {int(lo) | int(hi) << 64: int(c) for (lo, hi), c in zip(ids.tolist(), counts.tolist())}

    out = {}
    for name, kind, accounts in (("uniform", "c2", n_acct), ("zipf", "c3", n_acct), ("one_pair", "c2", 2)):
        if name != "uniform":
            e.reset_transfers()
        log = e.log_window(n_xfer)
        e.generate_transfers(log, 0, n_xfer, accounts, seed=42, kind=KINDS[kind])
        e.sync()
        x_lens = batches(n_xfer, batch)
        x_ts, t = timestamps(x_lens, t + 10)
        e.commit_device_async(129, x_ts, x_lens, log, res, rb)
        e.sync()
        oldest, _, _ = e.query_transfers(limit=1)
        newest, _, _ = e.query_transfers(reversed=True, limit=1)
        t_first, t_last = int(oldest["timestamp"][0]), int(newest["timestamp"][0])
        t_open = t_first - 1
        sample = e.to_host(log + (n_xfer // 2) * 128, min(n_xfer // 2, 1 << 16) * 128).view(TRANSFER_DTYPE)
        ids, counts = np.unique(sample[["debit_account_id_lo", "debit_account_id_hi"]], return_counts=True)
        hot = int(ids[np.argmax(counts)][0]) | int(ids[np.argmax(counts)][1]) << 64
        code = int(sample["code"][0])
        if name == "uniform":
            med, lo_ms, hi_ms = timed(e, lambda: e.copy_device_async(spare, log, n_xfer * 128))
            out["copy_log_d2d"] = row(med, lo_ms, hi_ms, bytes=n_xfer * 128)
            groups = None
            if "--skip-host" not in sys.argv:
                start = time.perf_counter()
                groups = paged(t_open)
                out["uniform_paged_on_host"] = dict(ms=round((time.perf_counter() - start) * 1e3, 1), groups=len(groups),
                                                    records=sum(groups.values()) // 2)
        _, q_matched, _ = e.query_transfers(timestamp_min=t_open + 1, limit=1)
        q_med, q_lo, q_hi = timed(e, raw_query(timestamp_min=t_open + 1, limit=1))
        out["%s_query_transfers_limit_1" % name] = row(q_med, q_lo, q_hi, matched=q_matched)
        c_med, c_lo, c_hi = timed(e, raw_counterparties(hot, t_open, t_last, rows_max))
        out["%s_counterparties_hottest" % name] = row(c_med, c_lo, c_hi, matched=int(h_res.matched))
        ce_med, ce_lo, ce_hi = timed(e, raw_counterparties(hot, t_last, t_last + 1, rows_max))
        out["%s_counterparties_empty_period" % name] = row(ce_med, ce_lo, ce_hi)
        if not have:
            continue
        rows, matched, complete = e.get_active_accounts(t_open, t_last)
        assert complete and len(rows) == min(matched, rows_max)
        if name == "uniform" and groups is not None:
            assert matched == len(groups)
            mine = {int(r["id_lo"]) | int(r["id_hi"]) << 64: int(r["debits_transfers"]) + int(r["credits_transfers"]) for r in rows}
            assert all(groups[x] == v for x, v in mine.items())
        out["%s_most_active" % name] = [list(r) for r in e.top_accounts(t_open, t_last, 3, "transfers")]
        for leg, fn in (("by_id_limit_8191", raw_active(t_open, t_last, rows_max)),
                        ("by_volume_limit_10", raw_active(t_open, t_last, 10, 1 << 8)),
                        ("by_transfers_limit_10", raw_active(t_open, t_last, 10, 1 << 9)),
                        ("one_code", raw_active(t_open, t_last, rows_max, code=code))):
            med, lo_ms, hi_ms = timed(e, fn)
            out["%s_active_%s" % (name, leg)] = row(med, lo_ms, hi_ms, matched=int(h_res.matched), over_query_transfers=round(med / q_med, 2),
                                                     over_counterparties_hottest=round(med / c_med, 2))
        for leg, fn in (("empty_period", raw_active(t_last, t_last + 1, rows_max)),
                        ("ledger_no_record_carries", raw_active(t_open, t_last, rows_max, ledger=3))):
            med, lo_ms, hi_ms = timed(e, fn)
            assert h_res.matched == 0
            out["%s_active_%s" % (name, leg)] = row(med, lo_ms, hi_ms, counterparties_empty_period_ms=round(ce_med, 4),
                                                     over_counterparties_empty_period=round(med / ce_med, 2))
    e.close()
    return out


def measure_ledgers():
    """get_ledger_balances beside query_accounts, query_transfers and the copies, in one process."""
    import ctypes

    from tigerbeetle_amd import _lib
    from tigerbeetle_amd.types import LEDGER_BALANCE_DTYPE
    os.environ["TBGPU_QUERY_COOP"] = "0"
    h_out = np.zeros(Engine.LEDGERS_MAX, dtype=LEDGER_BALANCE_DTYPE)
    h_res = _lib.tbgpu_query_result()

    def raw(e, ledgers, T):
        body = np.array(ledgers, dtype="<u4").tobytes()
        src = ctypes.create_string_buffer(body, len(body))
        return lambda: _lib.check(e.lib.tbgpu_get_ledger_balances(e.h, T, src, len(ledgers), h_out.ctypes.data, len(ledgers), ctypes.byref(h_res)))

    out = {}
    e = Engine(Options(accounts_max=n_acct, transfers_max=n_xfer, pass_events_max=pb * batch, pass_batches_max=pb))
    a_lens = batches(n_acct, batch)
    a_ts, t = timestamps(a_lens, 1_000_000_000)
    acct = e.alloc(n_acct * 128)
    e.generate_accounts(acct, 0, n_acct, seed=42)
    res = e.alloc(max(n_acct, n_xfer) * 8)
    rb = e.alloc((n_xfer // batch + 2) * 4)
    e.commit_device_async(128, a_ts, a_lens, acct, res, rb)
    e.sync()
    spare = e.alloc(n_xfer * 128)
    log = e.log_window(n_xfer)
    e.generate_transfers(log, 0, n_xfer, n_acct, seed=42, kind=KINDS["c2"])
    e.sync()
    x_lens = batches(n_xfer, batch)
    x_ts, t = timestamps(x_lens, t + 10)
    e.commit_device_async(129, x_ts, x_lens, log, res, rb)
    e.sync()
    oldest, _, _ = e.query_transfers(limit=1)
    newest, _, _ = e.query_transfers(reversed=True, limit=1)
    t_old, t_new = int(oldest["timestamp"][0]) - 1, int(newest["timestamp"][0])
    t_mid = (t_old + t_new) // 2
    many = [2] + list(range(1000, 1000 + Engine.LEDGERS_MAX - 1))
    # What is timed is right: the every-ledger row is the summary, and every T balances.
    summary = e.ledger_summary()
    for T in (0, t_new, t_mid, t_old):
        rows, matched, complete = e.get_ledger_balances([2, 0, 9], T)
        assert matched == 3 and complete and rows[0].tobytes()[:72] == rows[1].tobytes()[:72] and not rows[2]["accounts"]
        for c in ("pending", "posted"):
            assert rows["debits_%s_lo" % c][0] == rows["credits_%s_lo" % c][0] and rows["debits_%s_hi" % c][0] == rows["credits_%s_hi" % c][0]
        if T in (0, t_new):
            assert int(rows["accounts"][1]) == summary["accounts"] == n_acct
            assert int(rows["debits_posted_lo"][1]) | int(rows["debits_posted_hi"][1]) << 64 == summary["debits_posted"]
        if T == t_old:
            assert not rows["debits_posted_lo"][0] and not rows["debits_pending_lo"][0]
    slots = e.stats()["account_table_bytes"] // 132  # hot 32 + balances 64 + cold 32 + mark 4 per slot
    table_bytes = slots * 32 + n_acct * 64
    med, lo_ms, hi_ms = timed(e, lambda: e.copy_device_async(spare, log, table_bytes))
    out["copy_table_d2d"] = copy_table = row(med, lo_ms, hi_ms, bytes=table_bytes, slots=slots)
    med, lo_ms, hi_ms = timed(e, lambda: e.copy_device_async(spare, log, n_xfer * 128))
    out["copy_log_d2d"] = row(med, lo_ms, hi_ms, bytes=n_xfer * 128)
    recs, matched, _ = e.query_accounts(ledger=2, limit=8190)
    assert matched == n_acct
    med, lo_ms, hi_ms = timed(e, lambda: e.query_accounts(ledger=2, limit=8190))
    out["query_accounts_all_match"] = qa = row(med, lo_ms, hi_ms, matched=matched, table_scans=e.query_select_scans() + 2)
    for name, ledgers in (("now_1_ledger", [2]), ("now_1024_ledgers", many)):
        med, lo_ms, hi_ms = timed(e, raw(e, ledgers, 0))
        out[name] = now = row(med, lo_ms, hi_ms, ledgers=len(ledgers), over_query_accounts=round(med / qa["ms"], 2),
                              over_copy_table=round(med / copy_table["ms"], 2))
        if len(ledgers) == 1:
            now_1 = now
    for name, T in (("t_new", t_new), ("t_mid", t_mid), ("t_old", t_old)):
        _, q_matched, _ = e.query_transfers(timestamp_min=T + 1, limit=1)
        q_med, q_lo, q_hi = timed(e, lambda: e.query_transfers(timestamp_min=T + 1, limit=1))
        for req, ledgers in (("1_ledger", [2]), ("1024_ledgers", many), ("ledger_0", [0])):
            med, lo_ms, hi_ms = timed(e, raw(e, ledgers, T))
            scan = med - now_1["ms"]  # the log scan's share: the call less the table scan
            out["%s_%s" % (name, req)] = row(med, lo_ms, hi_ms, ledgers=len(ledgers), newer_records=q_matched,
                                             query_transfers_ms=round(q_med, 4), query_transfers_min_ms=round(q_lo, 4),
                                             query_transfers_max_ms=round(q_hi, 4), log_scan_ms=round(scan, 4),
                                             log_scan_over_query_transfers=round(scan / q_med, 2))
    e.close()
    # The same table with its accounts over 2 and over 1,024 ledgers, no log.
    for name, n_ledgers in (("table_2_ledgers", 2), ("table_1024_ledgers", Engine.LEDGERS_MAX)):
        e = Engine(Options(accounts_max=n_acct, transfers_max=1 << 14, pass_events_max=pb * batch, pass_batches_max=pb))
        acct = e.alloc(n_acct * 128)
        e.generate_accounts(acct, 0, n_acct, seed=42)
        e.sync()
        host = e.to_host(acct, n_acct * 128).view(ACCOUNT_DTYPE)
        host["ledger"] = 1 + np.arange(n_acct) % n_ledgers
        e.to_device(acct, host)
        res = e.alloc(n_acct * 8)
        rb = e.alloc((n_acct // batch + 2) * 4)
        e.commit_device_async(128, a_ts, a_lens, acct, res, rb)
        e.sync()
        ledgers = list(range(1, n_ledgers + 1))
        rows, _, _ = e.get_ledger_balances(ledgers + [0], 0) if n_ledgers < Engine.LEDGERS_MAX else e.get_ledger_balances(ledgers, 0)
        assert int(rows["accounts"][:n_ledgers].sum()) == n_acct and int(rows["accounts"].min()) >= n_acct // n_ledgers
        med, lo_ms, hi_ms = timed(e, raw(e, ledgers, 0))
        out[name] = row(med, lo_ms, hi_ms, ledgers=n_ledgers, over_one_ledger_table=round(med / now_1["ms"], 2))
        e.close()
    return out


def measure_pending():
    """get_pending_transfers beside query_transfers over the same window, on a C4 log, in one process."""
    import ctypes

    from tests.harness.configs import SETTINGS
    from tigerbeetle_amd import _lib
    from tigerbeetle_amd.types import (PENDING_EXPIRED, PENDING_OPEN, PENDING_POSTED, PENDING_ROW_DTYPE, PENDING_STATES,
                                       PENDING_VOIDED)
    os.environ["TBGPU_QUERY_COOP"] = "0"
    e = Engine(Options(accounts_max=n_acct, transfers_max=n_xfer, pass_events_max=pb * batch, pass_batches_max=pb))
    a_lens = batches(n_acct, batch)
    a_ts, t = timestamps(a_lens, 1_000_000_000)
    acct = e.alloc(n_acct * 128)
    e.generate_accounts(acct, 0, n_acct, seed=42)
    res = e.alloc(max(n_acct, n_xfer) * 8)
    rb = e.alloc((n_xfer // batch + 2) * 4)
    e.commit_device_async(128, a_ts, a_lens, acct, res, rb)
    e.sync()
    log = e.log_window(n_xfer)
    e.generate_transfers(log, 0, n_xfer, n_acct, seed=42, kind=KINDS["c4"])
    e.sync()
    x_lens = batches(n_xfer, batch)
    x_ts, t = timestamps(x_lens, t + 10, gap_every=SETTINGS["c4"]["gap_every"])
    e.commit_device_async(129, x_ts, x_lens, log, res, rb)
    e.sync()
    h_rows = np.zeros(Engine.PENDING_ROWS_MAX, dtype=PENDING_ROW_DTYPE)
    h_states = np.zeros(Engine.PENDING_ROWS_MAX, dtype=np.uint8)
    h_recs = np.zeros(8190, dtype=TRANSFER_DTYPE)
    h_res = _lib.tbgpu_query_result()

    def raw(**filter):
        f = Engine.pending_filter(**filter)
        src = ctypes.create_string_buffer(f, len(f))
        return lambda: _lib.check(e.lib.tbgpu_get_pending_transfers(e.h, src, h_rows.ctypes.data, h_states.ctypes.data,
                                                                    Engine.PENDING_ROWS_MAX, ctypes.byref(h_res)))

    def raw_query(**filter):
        f = Engine.query_filter(**filter)
        src = ctypes.create_string_buffer(f, len(f))
        return lambda: _lib.check(e.lib.tbgpu_query_transfers(e.h, src, h_recs.ctypes.data, 8190, ctypes.byref(h_res)))

    out = {}
    resolved, unresolved = PENDING_POSTED | PENDING_VOIDED, PENDING_OPEN | PENDING_EXPIRED
    counts = {}
    for name, bit in (("open", PENDING_OPEN), ("expired", PENDING_EXPIRED), ("posted", PENDING_POSTED), ("voided", PENDING_VOIDED)):
        rows, states, counts[name], complete = e.get_pending_transfers(states=bit, limit=1)
        assert complete and counts[name] > 0 and states.tolist() == [bit]
    out["rows_by_state"] = counts
    # What is timed is right where it can be said without a checker: ordered, resolved by its own id.
    for rev in (False, True):
        rows, states, matched, complete = e.get_pending_transfers(reversed=rev)
        ts = rows["pending"]["timestamp"].astype(np.int64)
        assert complete and matched == sum(counts.values()) and np.all(np.diff(ts) < 0 if rev else np.diff(ts) > 0)
        hit = (states & resolved) != 0
        assert hit.any() and (rows["resolution"]["pending_id_lo"][hit] == rows["pending"]["id_lo"][hit]).all()
        assert not rows["resolution"]["timestamp"][~hit].any()
    q_med, q_lo, q_hi = timed(e, raw_query(limit=4095))
    out["query_transfers_all_zero"] = row(q_med, q_lo, q_hi, bytes_per_record=48)
    s_med, s_lo, s_hi = timed(e, raw(states=unresolved))
    out["selection_open_expired"] = row(s_med, s_lo, s_hi, bytes_per_record=32, over_query_transfers=round(s_med / q_med, 2))
    for name, flt in (("all_states_ascending", dict()), ("all_states_reversed", dict(reversed=True)),
                      ("join_4095_ascending", dict(states=resolved)), ("join_4095_reversed", dict(states=resolved, reversed=True)),
                      ("join_1_ascending", dict(states=resolved, limit=1)), ("join_1_reversed", dict(states=resolved, limit=1, reversed=True))):
        rows, states, matched, _ = e.get_pending_transfers(**flt)
        med, lo_ms, hi_ms = timed(e, raw(**flt))
        out[name] = row(med, lo_ms, hi_ms, matched=matched, rows=len(rows), resolved_rows=int(((states & resolved) != 0).sum()),
                        less_selection_ms=round(med - s_med, 4), over_query_transfers=round(med / q_med, 2))
    sample = e.to_host(log + (n_xfer // 2) * 128, 128).view(TRANSFER_DTYPE)
    account = int(sample["debit_account_id_lo"][0]) | int(sample["debit_account_id_hi"][0]) << 64
    rows, states, matched, _ = e.get_pending_transfers(account)
    med, lo_ms, hi_ms = timed(e, raw(account_id=account))
    out["one_account_all_states"] = row(med, lo_ms, hi_ms, matched=matched, over_query_transfers=round(med / q_med, 2))
    e.close()
    return out


result = dict(transfers=n_xfer, log_bytes=n_xfer * 128, runs=runs, warmups=WARMUPS)
if only == "asof":
    result["asof"] = measure_asof()
elif only == "ledgers":
    result["ledgers"] = measure_ledgers()
elif only == "pending":
    result["pending"] = measure_pending()
elif only == "statements":
    result["statements"] = measure_statements()
elif only == "integrals":
    result["integrals"] = measure_integrals()
elif only == "extremes":
    result["extremes"] = measure_extremes()
elif only == "series":
    result["series"] = measure_series()
elif only == "matrix":
    result["matrix"] = measure_matrix()
elif only == "counterparties":
    result["counterparties"] = measure_counterparties()
elif only == "activity":
    result["activity"] = measure_activity()
elif only == "many":
    result["many"] = measure_many()
elif only == "balances":
    result["balances"] = measure(False, balances=True)
elif only == "change_events":
    result["change_events"] = measure_change_events()
elif only != "fields":
    result.update(lane_per_record=measure(False), cooperative=measure(True))
    for shape in ("lane_per_record", "cooperative"):
        r = result[shape]
        r["bar_query_le_copy"] = all(v["ms"] <= r["copy_d2d"]["ms"] for k, v in r.items() if k != "copy_d2d")
if only not in ("account", "balances", "change_events", "many", "asof", "ledgers", "pending", "statements", "integrals", "extremes", "series", "matrix", "counterparties", "activity"):
    result["field_filters"] = measure_fields()
print(json.dumps(result))
