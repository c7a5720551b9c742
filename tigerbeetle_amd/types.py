"""Account / Transfer layouts, flags, operations and result codes.

Mirrors src/tigerbeetle.zig:7-249 and src/state_machine.zig:208-214 of the reference (and the C
header src/clients/c/tb_client.h:17-165).  u128 fields are stored little-endian as two u64 words
(`<name>_lo`, `<name>_hi`); the structured dtypes below are byte-identical to the 128-byte extern
structs.
"""
import enum
import struct

import numpy as np

U128_MAX = (1 << 128) - 1
U64_MAX = (1 << 64) - 1

# Operation (state_machine.zig:208-214; vsr_operations_reserved = 128, constants.zig:38).
class Operation(enum.IntEnum):
    create_accounts = 128
    create_transfers = 129
    lookup_accounts = 130
    lookup_transfers = 131


# batch_max (state_machine.zig:46-65) for the production config: message_body_size_max =
# 1 MiB - 128 B header (config.zig:137, vsr.zig:401, constants.zig:167-168).
MESSAGE_BODY_SIZE_MAX = (1 << 20) - 128
BATCH_MAX = MESSAGE_BODY_SIZE_MAX // 128  # 8191


class AccountFlags(enum.IntFlag):
    linked = 1 << 0
    debits_must_not_exceed_credits = 1 << 1
    credits_must_not_exceed_debits = 1 << 2


class TransferFlags(enum.IntFlag):
    linked = 1 << 0
    pending = 1 << 1
    post_pending_transfer = 1 << 2
    void_pending_transfer = 1 << 3
    balancing_debit = 1 << 4
    balancing_credit = 1 << 5


# Values == declaration index (asserted at tigerbeetle.zig:139-143, :224-228).
CreateAccountResult = enum.IntEnum("CreateAccountResult", [(n, i) for i, n in enumerate("""
ok linked_event_failed linked_event_chain_open timestamp_must_be_zero reserved_field reserved_flag
id_must_not_be_zero id_must_not_be_int_max flags_are_mutually_exclusive debits_pending_must_be_zero
debits_posted_must_be_zero credits_pending_must_be_zero credits_posted_must_be_zero
ledger_must_not_be_zero code_must_not_be_zero exists_with_different_flags
exists_with_different_user_data_128 exists_with_different_user_data_64
exists_with_different_user_data_32 exists_with_different_ledger exists_with_different_code exists
""".split())])

CreateTransferResult = enum.IntEnum("CreateTransferResult", [(n, i) for i, n in enumerate("""
ok linked_event_failed linked_event_chain_open timestamp_must_be_zero reserved_flag
id_must_not_be_zero id_must_not_be_int_max flags_are_mutually_exclusive
debit_account_id_must_not_be_zero debit_account_id_must_not_be_int_max
credit_account_id_must_not_be_zero credit_account_id_must_not_be_int_max accounts_must_be_different
pending_id_must_be_zero pending_id_must_not_be_zero pending_id_must_not_be_int_max
pending_id_must_be_different timeout_reserved_for_pending_transfer amount_must_not_be_zero
ledger_must_not_be_zero code_must_not_be_zero debit_account_not_found credit_account_not_found
accounts_must_have_the_same_ledger transfer_must_have_the_same_ledger_as_accounts
pending_transfer_not_found pending_transfer_not_pending
pending_transfer_has_different_debit_account_id pending_transfer_has_different_credit_account_id
pending_transfer_has_different_ledger pending_transfer_has_different_code
exceeds_pending_transfer_amount pending_transfer_has_different_amount
pending_transfer_already_posted pending_transfer_already_voided pending_transfer_expired
exists_with_different_flags exists_with_different_debit_account_id
exists_with_different_credit_account_id exists_with_different_amount
exists_with_different_pending_id exists_with_different_user_data_128
exists_with_different_user_data_64 exists_with_different_user_data_32
exists_with_different_timeout exists_with_different_code exists overflows_debits_pending
overflows_credits_pending overflows_debits_posted overflows_credits_posted overflows_debits
overflows_credits overflows_timeout exceeds_credits exceeds_debits
""".split())])

assert len(CreateAccountResult) == 22 and len(CreateTransferResult) == 56


def _u128(name):
    return [(name + "_lo", "<u8"), (name + "_hi", "<u8")]


# Account (tigerbeetle.zig:7-29): 128 bytes, align 16, no padding.
ACCOUNT_DTYPE = np.dtype(
    _u128("id") + _u128("debits_pending") + _u128("debits_posted") + _u128("credits_pending")
    + _u128("credits_posted") + _u128("user_data_128")
    + [("user_data_64", "<u8"), ("user_data_32", "<u4"), ("reserved", "<u4"), ("ledger", "<u4"),
       ("code", "<u2"), ("flags", "<u2"), ("timestamp", "<u8")])

# Transfer (tigerbeetle.zig:64-89).
TRANSFER_DTYPE = np.dtype(
    _u128("id") + _u128("debit_account_id") + _u128("credit_account_id") + _u128("amount")
    + _u128("pending_id") + _u128("user_data_128")
    + [("user_data_64", "<u8"), ("user_data_32", "<u4"), ("timeout", "<u4"), ("ledger", "<u4"),
       ("code", "<u2"), ("flags", "<u2"), ("timestamp", "<u8")])

# {index: u32, result: u32} (tigerbeetle.zig:231-249).
RESULT_DTYPE = np.dtype([("index", "<u4"), ("result", "<u4")])

assert ACCOUNT_DTYPE.itemsize == 128 and TRANSFER_DTYPE.itemsize == 128 and RESULT_DTYPE.itemsize == 8

# tbgpu_account_filter (include/tbgpu.h tbgpu_get_account_transfers): 64 bytes, no padding.
ACCOUNT_FILTER_DTYPE = np.dtype(
    _u128("account_id") + [("timestamp_min", "<u8"), ("timestamp_max", "<u8"), ("limit", "<u4"), ("flags", "<u4"),
                           ("reserved", "u1", (24,))])
assert ACCOUNT_FILTER_DTYPE.itemsize == 64
FILTER_DEBITS, FILTER_CREDITS, FILTER_REVERSED = 1, 2, 4

# tbgpu_account_balance (include/tbgpu.h tbgpu_get_account_balances): 128 bytes, no padding.
ACCOUNT_BALANCE_DTYPE = np.dtype(
    _u128("debits_pending") + _u128("debits_posted") + _u128("credits_pending") + _u128("credits_posted")
    + [("timestamp", "<u8"), ("reserved", "u1", (56,))])
assert ACCOUNT_BALANCE_DTYPE.itemsize == 128

# tbgpu_ledger_balance (include/tbgpu.h tbgpu_get_ledger_balances): 128 bytes, no padding.
LEDGER_BALANCE_DTYPE = np.dtype(
    _u128("debits_pending") + _u128("debits_posted") + _u128("credits_pending") + _u128("credits_posted")
    + [("accounts", "<u8"), ("ledger", "<u4"), ("reserved", "u1", (52,))])
assert LEDGER_BALANCE_DTYPE.itemsize == 128
LEDGERS_MAX = 1024

# tbgpu_pending_filter and tbgpu_pending_row (include/tbgpu.h tbgpu_get_pending_transfers): 64 and 256
# bytes, no padding; a row is the pending transfer and the post or void record that resolved it.
PENDING_FILTER_DTYPE = np.dtype(
    _u128("account_id") + [("timestamp_min", "<u8"), ("timestamp_max", "<u8"), ("now", "<u8"), ("limit", "<u4"),
                           ("flags", "<u4"), ("reserved", "u1", (16,))])
PENDING_ROW_DTYPE = np.dtype([("pending", TRANSFER_DTYPE), ("resolution", TRANSFER_DTYPE)])
assert PENDING_FILTER_DTYPE.itemsize == 64 and PENDING_ROW_DTYPE.itemsize == 256
PENDING_OPEN, PENDING_EXPIRED, PENDING_POSTED, PENDING_VOIDED = 1 << 4, 1 << 5, 1 << 6, 1 << 7
PENDING_STATES = PENDING_OPEN | PENDING_EXPIRED | PENDING_POSTED | PENDING_VOIDED
PENDING_ROWS_MAX = 4095

# tbgpu_account_statement (include/tbgpu.h tbgpu_get_account_statements): 256 bytes, no padding; the
# balances at the period's start and end in ACCOUNT_DTYPE's column order, the period's gross flows and
# its transfer counts.
_BALANCE_COLUMNS = ("debits_pending", "debits_posted", "credits_pending", "credits_posted")
STATEMENT_DTYPE = np.dtype(
    _u128("id")
    + [f for when in ("opening", "closing") for c in _BALANCE_COLUMNS for f in _u128(when + "_" + c)]
    + [f for side in ("debits", "credits") for c in ("pending_in", "pending_out", "posted_in") for f in _u128(side + "_" + c)]
    + [("debit_transfers", "<u8"), ("credit_transfers", "<u8")])
assert STATEMENT_DTYPE.itemsize == 256
STATEMENTS_MAX = 4095

# tbgpu_account_balance_integral (include/tbgpu.h tbgpu_get_account_balance_integrals): 256 bytes, no
# padding; the balances at the period's start and end as STATEMENT_DTYPE has them, each column's time
# integral over the period in three words (low word first, modulo 2^192) and the period as used.
INTEGRAL_DTYPE = np.dtype(
    _u128("id")
    + [f for when in ("opening", "closing") for c in _BALANCE_COLUMNS for f in _u128(when + "_" + c)]
    + [("integral_" + c + w, "<u8") for c in _BALANCE_COLUMNS for w in ("_w0", "_w1", "_w2")]
    + [("t_open", "<u8"), ("t_end", "<u8")])
assert INTEGRAL_DTYPE.itemsize == 256
INTEGRALS_MAX = 4095

# tbgpu_account_balance_extreme (include/tbgpu.h tbgpu_get_account_balance_extremes): 192 bytes, no
# padding; the measure at the period's start and end, its minimum and maximum over the period (signed,
# two's complement, 192 bits, low word first), when each was first reached, the period's records, the
# period as used and the request's measure.
EXTREME_DTYPE = np.dtype(
    _u128("id")
    + [(v + w, "<u8") for v in ("opening", "closing", "low", "high") for w in ("_w0", "_w1", "_w2")]
    + [("t_low", "<u8"), ("t_high", "<u8"), ("records", "<u8"), ("t_open", "<u8"), ("t_end", "<u8"), ("measure", "<u8"),
       ("reserved", "<u8", (4,))])
assert EXTREME_DTYPE.itemsize == 192
EXTREMES_MAX = 4095
# The usual measures (TBGPU_MEASURE_*): the coefficients of (debits_pending, debits_posted,
# credits_pending, credits_posted), each -1, 0 or +1.
MEASURE_CREDIT_NET_POSTED = (0, -1, 0, 1)
MEASURE_CREDIT_AVAILABLE = (-1, -1, 0, 1)
MEASURE_DEBIT_NET_POSTED = (0, 1, 0, -1)
MEASURE_DEBIT_AVAILABLE = (0, 1, -1, -1)
MEASURE_DEBITS_PENDING = (1, 0, 0, 0)
MEASURE_DEBITS_POSTED = (0, 1, 0, 0)
MEASURE_CREDITS_PENDING = (0, 0, 1, 0)
MEASURE_CREDITS_POSTED = (0, 0, 0, 1)


def pack_balance_measure(measure, reserved=b"\0\0\0\0"):
    """The 8 bytes of a tbgpu_balance_measure from four coefficients (each must fit a signed byte; the
    library checks the rest)."""
    coefficients = [int(c) for c in measure]
    reserved = bytes(reserved)
    if len(coefficients) != 4 or len(reserved) != 4 or not all(-128 <= c <= 127 for c in coefficients):
        raise ValueError("a measure is four coefficients, each a signed byte, and four reserved bytes")
    return bytes(c & 0xFF for c in coefficients) + reserved


def extreme_value(row, name):
    """Field `name` ("opening", "closing", "low" or "high") of an EXTREME_DTYPE row as a Python int."""
    v = sum(int(row["%s_w%d" % (name, k)]) << (64 * k) for k in range(3))
    return v - (1 << 192) if v >> 191 else v


# tbgpu_get_account_statement_series: STATEMENT_DTYPE rows, ids x buckets of them at most.
SERIES_ROWS_MAX = 4095

# tbgpu_flow_cell (include/tbgpu.h tbgpu_get_account_flow_matrix): 96 bytes, no padding; what the debit
# account paid the credit account over the period — posted amounts, holds placed, holds released — and
# the number of records.
FLOW_CELL_DTYPE = np.dtype(
    _u128("debit_id") + _u128("credit_id") + _u128("posted") + _u128("pending_in") + _u128("pending_out")
    + [("transfers", "<u8"), ("reserved", "<u8")])
assert FLOW_CELL_DTYPE.itemsize == 96
FLOW_MATRIX_CELLS_MAX = 4095

# tbgpu_counterparty_filter and tbgpu_counterparty (include/tbgpu.h tbgpu_get_account_counterparties): 64
# and 128 bytes, no padding; a row is a counterparty's id, what the subject paid it (`to`) and what it
# paid the subject (`from`), each a flow cell's seven sum words.
COUNTERPARTY_FILTER_DTYPE = np.dtype(
    _u128("account_id") + [("t_open", "<u8"), ("t_close", "<u8")] + _u128("id_min")
    + [("limit", "<u4"), ("flags", "<u4"), ("reserved", "u1", (8,))])
COUNTERPARTY_DTYPE = np.dtype(
    _u128("id")
    + [f for d in ("to", "from") for c in ("posted", "pending_in", "pending_out") for f in _u128(d + "_" + c)][:6]
    + [("to_transfers", "<u8")]
    + [f for c in ("posted", "pending_in", "pending_out") for f in _u128("from_" + c)]
    + [("from_transfers", "<u8")])
assert COUNTERPARTY_FILTER_DTYPE.itemsize == 64 and COUNTERPARTY_DTYPE.itemsize == 128
COUNTERPARTIES_BY_VOLUME = 1 << 8
COUNTERPARTIES_ROWS_MAX = 8191


def pack_counterparty_filter(account_id, t_open=0, t_close=0, id_min=0, limit=COUNTERPARTIES_ROWS_MAX,
                             flags=FILTER_DEBITS | FILTER_CREDITS):
    """The 64 bytes of a tbgpu_counterparty_filter."""
    f = np.zeros(1, dtype=COUNTERPARTY_FILTER_DTYPE)
    f["account_id_lo"], f["account_id_hi"] = account_id & U64_MAX, account_id >> 64
    f["t_open"], f["t_close"] = t_open, t_close
    f["id_min_lo"], f["id_min_hi"] = id_min & U64_MAX, id_min >> 64
    f["limit"], f["flags"] = limit, flags
    return f.tobytes()


# tbgpu_activity_filter and tbgpu_account_activity (include/tbgpu.h tbgpu_get_active_accounts): 64 and
# 128 bytes, no padding; a row is an account's id, what it paid (`debits`) and what it was paid
# (`credits`), each a flow cell's seven sum words.
ACTIVITY_FILTER_DTYPE = np.dtype(
    [("t_open", "<u8"), ("t_close", "<u8")] + _u128("id_min")
    + [("ledger", "<u4"), ("code", "<u2"), ("reserved0", "u1", (2,)), ("limit", "<u4"), ("flags", "<u4"), ("reserved", "u1", (16,))])
ACCOUNT_ACTIVITY_DTYPE = np.dtype(
    _u128("id")
    + [f for c in ("posted", "pending_in", "pending_out") for f in _u128("debits_" + c)] + [("debits_transfers", "<u8")]
    + [f for c in ("posted", "pending_in", "pending_out") for f in _u128("credits_" + c)] + [("credits_transfers", "<u8")])
assert ACTIVITY_FILTER_DTYPE.itemsize == 64 and ACCOUNT_ACTIVITY_DTYPE.itemsize == 128
ACTIVE_BY_VOLUME = 1 << 8
ACTIVE_BY_TRANSFERS = 1 << 9
ACTIVE_ROWS_MAX = 8191


def pack_activity_filter(t_open=0, t_close=0, id_min=0, ledger=0, code=0, limit=ACTIVE_ROWS_MAX, flags=FILTER_DEBITS | FILTER_CREDITS):
    """The 64 bytes of a tbgpu_activity_filter."""
    f = np.zeros(1, dtype=ACTIVITY_FILTER_DTYPE)
    f["t_open"], f["t_close"] = t_open, t_close
    f["id_min_lo"], f["id_min_hi"] = id_min & U64_MAX, id_min >> 64
    f["ledger"], f["code"], f["limit"], f["flags"] = ledger, code, limit, flags
    return f.tobytes()


# tbgpu_query_filter (include/tbgpu.h tbgpu_query_transfers / tbgpu_query_accounts): 64 bytes, no padding.
QUERY_FILTER_DTYPE = np.dtype(
    _u128("user_data_128") + [("user_data_64", "<u8"), ("user_data_32", "<u4"), ("ledger", "<u4"), ("code", "<u2"),
                              ("reserved", "u1", (6,)), ("timestamp_min", "<u8"), ("timestamp_max", "<u8"),
                              ("limit", "<u4"), ("flags", "<u4")])
assert QUERY_FILTER_DTYPE.itemsize == 64
QUERY_REVERSED = 1

# tbgpu_change_events_filter and tbgpu_change_event (include/tbgpu.h tbgpu_get_change_events): 64 and
# 384 bytes, no padding; an event is the transfer and its two accounts right after it.
CHANGE_EVENTS_FILTER_DTYPE = np.dtype(
    [("timestamp_min", "<u8"), ("timestamp_max", "<u8"), ("limit", "<u4"), ("reserved", "u1", (44,))])
CHANGE_EVENT_DTYPE = np.dtype(
    [("transfer", TRANSFER_DTYPE), ("debit_account", ACCOUNT_DTYPE), ("credit_account", ACCOUNT_DTYPE)])
assert CHANGE_EVENTS_FILTER_DTYPE.itemsize == 64 and CHANGE_EVENT_DTYPE.itemsize == 384
CHANGE_EVENTS_MAX = 2730


def pack_change_events_filter(timestamp_min=0, timestamp_max=0, limit=CHANGE_EVENTS_MAX):
    """The 64 bytes of a tbgpu_change_events_filter."""
    f = np.zeros(1, dtype=CHANGE_EVENTS_FILTER_DTYPE)
    f["timestamp_min"], f["timestamp_max"], f["limit"] = timestamp_min, timestamp_max, limit
    return f.tobytes()


ACCOUNT_FIELDS = ("id", "debits_pending", "debits_posted", "credits_pending", "credits_posted",
                  "user_data_128", "user_data_64", "user_data_32", "reserved", "ledger", "code",
                  "flags", "timestamp")
TRANSFER_FIELDS = ("id", "debit_account_id", "credit_account_id", "amount", "pending_id",
                   "user_data_128", "user_data_64", "user_data_32", "timeout", "ledger", "code",
                   "flags", "timestamp")
_U128_FIELDS = {"id", "debits_pending", "debits_posted", "credits_pending", "credits_posted",
                "user_data_128", "debit_account_id", "credit_account_id", "amount", "pending_id"}

_ACCOUNT_STRUCT = struct.Struct("<" + "QQ" * 6 + "QIIIHHQ")
_TRANSFER_STRUCT = struct.Struct("<" + "QQ" * 6 + "QIIIHHQ")


def _split(v):
    return (v & U64_MAX, v >> 64)


def pack_account(id, debits_pending=0, debits_posted=0, credits_pending=0, credits_posted=0,
                 user_data_128=0, user_data_64=0, user_data_32=0, reserved=0, ledger=0, code=0,
                 flags=0, timestamp=0):
    return _ACCOUNT_STRUCT.pack(*_split(id), *_split(debits_pending), *_split(debits_posted),
                                *_split(credits_pending), *_split(credits_posted),
                                *_split(user_data_128), user_data_64, user_data_32, reserved,
                                ledger, code, flags, timestamp)


def pack_transfer(id, debit_account_id=0, credit_account_id=0, amount=0, pending_id=0,
                  user_data_128=0, user_data_64=0, user_data_32=0, timeout=0, ledger=0, code=0,
                  flags=0, timestamp=0):
    return _TRANSFER_STRUCT.pack(*_split(id), *_split(debit_account_id),
                                 *_split(credit_account_id), *_split(amount), *_split(pending_id),
                                 *_split(user_data_128), user_data_64, user_data_32, timeout,
                                 ledger, code, flags, timestamp)


def unpack_account(b):
    v = _ACCOUNT_STRUCT.unpack(b)
    out, i = {}, 0
    for f in ACCOUNT_FIELDS:
        if f in _U128_FIELDS:
            out[f] = v[i] | (v[i + 1] << 64)
            i += 2
        else:
            out[f] = v[i]
            i += 1
    return out


def unpack_transfer(b):
    v = _TRANSFER_STRUCT.unpack(b)
    out, i = {}, 0
    for f in TRANSFER_FIELDS:
        if f in _U128_FIELDS:
            out[f] = v[i] | (v[i + 1] << 64)
            i += 2
        else:
            out[f] = v[i]
            i += 1
    return out


def u128_column(arr, name):
    """Python ints of a u128 column of a structured array."""
    lo = arr[name + "_lo"].astype(object)
    hi = arr[name + "_hi"].astype(object)
    return [int(a) | (int(b) << 64) for a, b in zip(lo, hi)]
