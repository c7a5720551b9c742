// query.h — the host side of the queries (include/tbgpu.h): get_account_transfers and its batched form
// get_account_transfers_many, get_account_balances, query_transfers, query_accounts,
// get_change_events, lookup_accounts_at, get_ledger_balances, get_pending_transfers,
// get_account_statements, get_account_balance_integrals, get_account_statement_series,
// get_account_flow_matrix, get_account_counterparties and get_active_accounts; their buffers, made at tbgpu_init, and their entry points.  Included by engine.hip after the engine's own helpers and before node.h.
//
// Every query is written once, over a list of engines (QueryCall): the one engine, or a node's shards.
// A transfer lives on its home shard only and an account is answered by its owner only, so every
// engine scans its own log or table on its own device and stream, side by side, and the host merges
// the engines' answers — each its first k by timestamp, its last k under `reversed` — under the
// limit, summing the matches.  One engine's answer goes straight into the caller's buffer.  The
// sequencer's engine of a node is never asked.
#pragma once

#include "account_scan_host.h"

// tbgpu_get_account_transfers and tbgpu_query_transfers (k_query.h; one scan, two predicates): every
// buffer made at tbgpu_init, none shared with the write-back or the lookups (a write-back may be in
// flight beside a query).
#define QUERY_KEYS_CAP (1u << 16)  // {timestamp, position} keys of one round of the unordered path
struct QueryBufs {
    u64 nb_cap = 0;            // tiles of QUERY_THREADS log positions in the whole log
    u32* d_counts = nullptr;   // [nb_cap] matches per tile
    u64* d_mins = nullptr;     // [nb_cap] their smallest timestamp
    u64* d_maxs = nullptr;     // [nb_cap] ... and largest
    u32* d_ordered = nullptr;  // [nb_cap] 1: the tile's matches rise with position
    u64* d_base = nullptr;     // [nb_cap] exclusive prefix of d_counts
    u64* d_res = nullptr;      // {total, ordered}
    u64* h_res = nullptr;      // pinned mirror
    u8* d_out = nullptr;       // [BATCH_EVENTS_MAX] the answer's records
    u64* d_keys = nullptr;     // [QUERY_KEYS_CAP][2] unordered path: a round's keys; then the chosen positions
    u64* h_keys = nullptr;     // pinned mirror
    u64* h_base = nullptr;     // pinned [nb_cap + 1]: the bases, read back on the unordered path only
    u32 keys_max = QUERY_KEYS_CAP;  // tbgpu_bench_query_keys_max
    bool coop = false;         // tb_query_count's load shape (TBGPU_QUERY_COOP=1: cooperative 16-B chunks)
    // One query in flight between query_enqueue and query_collect.
    QueryFilter F{};
    QueryFieldFilter FF{};   // by_fields: tbgpu_query_transfers' predicate instead
    bool by_fields = false;
    QueryPendingFilter FP{};  // by_pending: tbgpu_get_pending_transfers' predicate instead
    bool by_pending = false;
    u32 k = 0;
    bool reversed = false;
    u64 n = 0;
};

// tbgpu_get_account_balances (k_balances.h): the rows' timestamps and the bins, on the device and
// pinned; made at tbgpu_init and shared with nothing.  The rows themselves are chosen through QueryBufs.
struct BalanceBufs {
    u64* d_ts = nullptr;    // [BATCH_EVENTS_MAX] the rows' timestamps, ascending
    u64* h_ts = nullptr;    // pinned mirror (a node hands every shard the merged rows' here)
    u64* d_bins = nullptr;  // [BALANCE_SLOTS(BATCH_EVENTS_MAX)][BALANCE_SLOT_WORDS]
    u64* h_bins = nullptr;  // pinned mirror
};

// tbgpu_query_accounts (k_query_filter.h): O(slots / 256 + histogram + k) device memory, made at
// tbgpu_init and shared with nothing.
struct AccountQueryBufs {
    u64 nb = 0;               // tiles of QUERY_THREADS slots in the account table
    u32* d_counts = nullptr;  // [nb] matches per tile
    u64* d_mins = nullptr;    // [nb] their smallest timestamp
    u64* d_maxs = nullptr;    // [nb] ... and largest
    u64* d_state = nullptr;   // [QA_WORDS], then the select's histograms: u32 [QA_PASSES][SEL_BINS]
    u64* h_state = nullptr;   // pinned mirror of the QA_WORDS
    u64* d_keys = nullptr;    // [BATCH_EVENTS_MAX][2] {value, slot} of the selected matches
    u8* d_out = nullptr;      // [BATCH_EVENTS_MAX] the answer's records
    u32 k = 0;                // one query in flight between account_query_enqueue and _collect
    u64 last_scans = 0;       // select passes of the last query (tbgpu_bench_query_select_scans)
};

// tbgpu_get_change_events (k_change_events.h): the page's account set, the bins, the accounts' records
// and the post rows' pending amounts, on the device and pinned; made by query_init and shared with
// nothing.  The rows themselves are chosen through QueryBufs.
struct ChangeBufs {
    u32* d_set = nullptr;     // [CHANGE_SET_SLOTS_MAX] the set's entries
    u64* d_ids = nullptr;     // [CHANGE_ACCOUNTS_MAX][2] the accounts' ids by index
    u64* d_pids = nullptr;    // [CHANGE_EVENTS_MAX][2] the post rows' pending ids
    u64* d_bins = nullptr;    // [CHANGE_ACCOUNTS_MAX + 1][BALANCE_SLOT_WORDS] the bins, then the flag slot
    u8* d_accounts = nullptr; // [CHANGE_ACCOUNTS_MAX] the accounts' records
    u32* d_found = nullptr;   // [CHANGE_ACCOUNTS_MAX] ... and whether the owner holds them
    u64* d_p = nullptr;       // [CHANGE_EVENTS_MAX][2] the post rows' pending amounts
    u32* d_found_p = nullptr; // [CHANGE_EVENTS_MAX] ... and whether the pending transfer is resident
    u32* h_set = nullptr;     // pinned mirrors (a node hands every shard the page's set here)
    u64* h_ids = nullptr;
    u64* h_pids = nullptr;
    u64* h_bins = nullptr;
    u8* h_accounts = nullptr;
    u32* h_found = nullptr;
    u64* h_p = nullptr;
    u32* h_found_p = nullptr;
    u8* h_rows = nullptr;     // pinned [CHANGE_EVENTS_MAX] the rows, before they are assembled into `out`
    u32* h_row_idx = nullptr; // host [CHANGE_EVENTS_MAX][2] the rows' debit and credit account index
};

// tbgpu_get_account_transfers_many (k_query_many.h): the filter set, per-chunk counts, bases and bounds,
// the totals and the answer area; made by query_init and shared with nothing.
// Every word a query reads is a word it wrote, so tbgpu_reset clears none of them.
#define QUERY_MANY_CHUNKS_MIN 4096u  // room for this many chunks whatever the log: a test's shrunk chunks
#define QUERY_MANY_STAGE (1u << 15)  // records of one copy to the host (4 MiB)
struct QueryManyBufs {
    u64 nc_cap = 0;                  // chunks the per-chunk buffers hold
    u32 tiles = QUERY_MANY_TILES;    // tiles of a chunk (tbgpu_bench_query_many_tiles)
    QueryManyTable* d_tab = nullptr; // the filter set
    QueryManyTable* h_tab = nullptr; // pinned: the host builds it here
    u32* d_counts = nullptr;         // [nc_cap][64] matches per chunk and filter
    u32* d_base = nullptr;           // [nc_cap][64] their exclusive prefix per filter
    u64* d_cmin = nullptr;           // [nc_cap] the smallest timestamp of a chunk's hits
    u64* d_cmax = nullptr;           // [nc_cap] ... and the largest (0: no hit)
    u32* d_cord = nullptr;           // [nc_cap] 1: the chunk's hits rise with position
    u64* d_ctiles = nullptr;         // [nc_cap] the chunk's tiles that hold a hit
    u64* d_res = nullptr;            // [QM_RES_WORDS] totals, `ordered`, where each answer starts in d_out, their sum
    u64* h_res = nullptr;            // pinned mirror
    u8* d_out = nullptr;             // [64 x BATCH_EVENTS_MAX] the answers' records, packed
    u8* h_stage = nullptr;           // pinned [QUERY_MANY_STAGE]: the records on their way to the caller's slots
    u64 n = 0;                       // one batch in flight between query_many_enqueue and _collect
};

// One set of the account-set scan's buffers (k_account_scan.h; the driver is further down): the
// request's ids, the set built from them, the bins, the accounts' records and found flags, the answer
// and the result words; made by query_init and shared with nothing outside the family.  Every word a
// query reads is a word it wrote, so tbgpu_reset clears none of them.  tbgpu_lookup_accounts_at has
// its own (ql: 8,191 ids, 128-B records, 8-word bins); tbgpu_get_account_statements' (qt: 4,095 ids,
// 256-B rows, 22-word bins) also serve the integrals and the series call, which are synchronous like
// it and bring only their own bins.
struct AccountScanBufs {
    u64* d_ids = nullptr;      // [ids][2] the request
    u64* h_ids = nullptr;      // pinned: the caller's ids on their way up (a node copies them into every shard's)
    u32* d_set = nullptr;      // [tb_change_set_slots(ids)] the set's entries
    u64* d_bins = nullptr;     // the bins by request position, then the flag word
    u8* d_accounts = nullptr;  // [ids] the records as the owners hold them
    u32* d_found = nullptr;    // [ids] 1: the position yields a row
    u8* d_out = nullptr;       // [ids] the answer's rows (one engine)
    u64* d_res = nullptr;      // [SCAN_RES_WORDS]
    u64* h_res = nullptr;      // pinned mirror
    u64* h_bins = nullptr;     // pinned mirrors, read by a node's host only: it adds the shards' bins
    u8* h_accounts = nullptr;
    u32* h_found = nullptr;
};
#define ASOF_BIN_BYTES(n) (((u64)(n) + 1) * BALANCE_SLOT_WORDS * 8)  // the flag word has a slot of its own
#define STATEMENT_BIN_BYTES(n) (((u64)(n) * STATEMENT_BIN_WORDS + 1) * 8)

// tbgpu_get_ledger_balances (k_ledgers.h): the ledger set and the bins, on the device and pinned; made
// by query_init and shared with nothing.  The host builds the set and writes the rows.
struct LedgerBufs {
    u32* d_set = nullptr;   // [LEDGER_SET_SLOTS_MAX] the set's entries
    u32* h_set = nullptr;   // pinned: the host builds it here (a node copies it into every shard's)
    u64* d_bins = nullptr;  // [LEDGER_BINS(LEDGER_SET_SLOTS_MAX)][LEDGER_BIN_WORDS]
    u64* h_bins = nullptr;  // pinned mirror
};

// tbgpu_get_pending_transfers (k_pending.h): the kept rows' states, the set of the resolved rows' ids,
// the ids and the resolution slots, on the device and pinned; made by query_init and shared with
// nothing.  The rows themselves are chosen through QueryBufs.
struct PendingBufs {
    u8* d_states = nullptr;   // [PENDING_ROWS_MAX] the kept rows' states, written with the rows
    u8* h_states = nullptr;   // pinned mirror
    u8* h_rows = nullptr;     // pinned [PENDING_ROWS_MAX] this engine's kept records, before they are placed into the rows
    u32* d_set = nullptr;     // [tb_change_set_slots(PENDING_ROWS_MAX)] the set's entries
    u32* h_set = nullptr;     // pinned: the host builds it here (a node copies it into every shard's)
    u64* d_ids = nullptr;     // [PENDING_ROWS_MAX][2] the resolved rows' ids by index
    u64* h_ids = nullptr;     // pinned, likewise
    u8* d_slots = nullptr;    // [PENDING_ROWS_MAX] the resolving records by index; zero: none on this engine
    u8* h_slots = nullptr;    // pinned mirror
    u32* h_row_of = nullptr;  // pinned [PENDING_ROWS_MAX] the row an index stands for
};

// tbgpu_get_account_balance_integrals (k_integral.h): the same request, set, records, flags, rows and
// result words as a statements call, at the same sizes — it works in QueryState::qt.  Only its bins are
// wider (INTEGRAL_BIN_WORDS), so they are its own.
struct IntegralBufs {
    u64* d_bins = nullptr;  // [INTEGRAL_IDS_MAX][INTEGRAL_BIN_WORDS] the bins by request position, then the flag word
    u64* h_bins = nullptr;  // pinned mirror, read by a node's host only: it adds the shards' bins
};
#define INTEGRAL_BIN_BYTES(n) (((u64)(n) * INTEGRAL_BIN_WORDS + 1) * 8)

// tbgpu_get_account_balance_extremes (k_extremes.h): a statements call's request, set, records, flags,
// rows and result words (QueryState::qt; its rows are narrower), and its own: the [S][n] element array
// the slabs fill, the zone 0 sums with the flag words behind them, and the two knobs read at init.
// The array has room for one slab per CU of the largest part at the largest request, 4,095 ids: 292
// slabs of 458,640 B in 128 MB — fewer where the log cannot hold that many spans of
// CHANGE_THREADS * CHANGE_TILES records.  A smaller request gets more, shorter slabs from the same
// bytes, down to one per span and up to EXTREME_SLABS_MAX.
struct ExtremeBufs {
    u64* d_elems = nullptr;  // [slabs][n][EXTREME_ELEM_WORDS]
    u64 elem_bytes = 0;
    u64* d_zone0 = nullptr;  // [EXTREME_IDS_MAX][3] the sums of the records above t_end, then EXTREME_FLAG_WORDS
    u64* h_flags = nullptr;  // pinned: the flag words, back after the emit
    u32 slabs_cap = 0;       // TBGPU_EXTREMES_SLABS: at most that many slabs (0: no cap) — tests force 1, 2 or many
    bool exact = false;      // TBGPU_EXTREMES_EXACT=1: the exact path on an ordered single engine too
};
#define EXTREME_ELEM_BYTES ((u64)EXTREME_ELEM_WORDS * 8)
#define EXTREME_ZONE0_BYTES(n) (((u64)(n) * 3 + EXTREME_FLAG_WORDS) * 8)
#define EXTREME_ARRAY_BYTES (128ull << 20)

// tbgpu_get_account_statement_series (k_series.h): a statements call's request, set, records, flags,
// rows and result words (QueryState::qt: n * n_buckets rows are at most STATEMENT_IDS_MAX), its own
// bounds and its own bins, one per key.
struct SeriesBufs {
    u64* d_bounds = nullptr;  // [SERIES_ROWS_MAX + 1] the request's bounds
    u64* h_bounds = nullptr;  // pinned: the caller's bounds on their way up
    u64* d_bins = nullptr;    // [SERIES_KEYS_MAX][SERIES_BIN_WORDS] the bins by key, then the flag word
    u64* h_bins = nullptr;    // pinned mirror, read by a node's host only: it adds the shards' bins
};
#define SERIES_BIN_BYTES(keys) (((u64)(keys) * SERIES_BIN_WORDS + 1) * 8)

// tbgpu_get_account_flow_matrix (k_matrix.h): an AccountScanBufs of its own (QueryState::qx) — its
// request is two lists, up to MATRIX_IDS_MAX positions, one more than the statements call's hold —
// with bins by key and 96-B cells, and the two maps that go up with the ids.
struct MatrixBufs {
    u16* d_maps = nullptr;  // [2][MATRIX_IDS_MAX] row_of, then col_of, each as long as the request
    u16* h_maps = nullptr;  // pinned: the host builds them here (a node: in every shard's)
};
#define MATRIX_BIN_BYTES(keys) (((u64)(keys) * MATRIX_BIN_WORDS + 1) * 8)

// tbgpu_get_account_counterparties (k_counterparties.h) and tbgpu_get_active_accounts (k_activity.h): the
// group table, the select's per-tile counts, state words and histograms, the collected keys and the
// answer; made by query_init and shared by the two calls alone (calls are synchronous, so two never
// overlap).  The table has room for `groups` counterparties, or accounts, at a load of at most one half: the engine's
// accounts_max, on a node's shard the node's (query_groups_hint: a peer's table is folded into the
// first shard's slot for slot, and a group's sums must be whole before the order is applied).
struct CounterpartyBufs {
    u64 groups = 0;           // the capacity the header promises
    u64 slots = 0;            // a power of two, at least 2 * groups
    u64* d_table = nullptr;   // [slots][CP_SLOT_WORDS]
    u32* d_counts = nullptr;  // [slots / QUERY_THREADS, rounded up] occupied slots per tile
    u64* d_state = nullptr;   // [CP_WORDS], then the select's histograms: u32 [CP_PASSES_MAX][SEL_BINS]
    u64* h_state = nullptr;   // pinned mirror of the CP_WORDS
    u64* d_keys = nullptr;    // [CP_ROWS_MAX][CP_KEY_STRIDE] the selected groups' keys and slots
    u8* d_out = nullptr;      // [CP_ROWS_MAX] the answer's rows
};
// Set by node_init around its shards' tbgpu_init: the groups a shard's table must hold (0: its own accounts_max).
static thread_local u64 query_groups_hint = 0;

// One engine's query buffers (tbgpu::qs), in the order query_init makes them.
struct QueryState {
    QueryBufs q;
    BalanceBufs qb;
    AccountQueryBufs qa;
    ChangeBufs qc;
    QueryManyBufs qm;
    AccountScanBufs ql;
    LedgerBufs qg;
    PendingBufs qp;
    AccountScanBufs qt;
    IntegralBufs qi;
    SeriesBufs qr;
    AccountScanBufs qx;
    MatrixBufs qxm;
    CounterpartyBufs qk;
    ExtremeBufs qe;
};

// One AccountScanBufs for `ids` request ids: in this order, which tests/test_gpu_alloc.py counts by.
static int account_scan_bufs_init(tbgpu* E, AccountScanBufs& B, u64 ids, u64 set_slots, u64 bin_bytes, u64 row_bytes) {
    HIPCK(tbMalloc(E->own, &B.d_ids, ids * 16));
    HIPCK(tbHostMalloc(E->own, &B.h_ids, ids * 16, hipHostMallocDefault));
    HIPCK(tbMalloc(E->own, &B.d_set, set_slots * 4));
    HIPCK(tbMalloc(E->own, &B.d_bins, bin_bytes));
    HIPCK(tbMalloc(E->own, &B.d_accounts, ids * 128));
    HIPCK(tbMalloc(E->own, &B.d_found, ids * 4));
    HIPCK(tbMalloc(E->own, &B.d_out, ids * row_bytes));
    HIPCK(tbMalloc(E->own, &B.d_res, SCAN_RES_WORDS * 8));
    HIPCK(tbHostMalloc(E->own, &B.h_res, SCAN_RES_WORDS * 8, hipHostMallocDefault));
    HIPCK(tbHostMalloc(E->own, &B.h_bins, bin_bytes, hipHostMallocDefault));
    HIPCK(tbHostMalloc(E->own, &B.h_accounts, ids * 128, hipHostMallocDefault));
    HIPCK(tbHostMalloc(E->own, &B.h_found, ids * 4, hipHostMallocDefault));
    return TBGPU_STATUS_OK;
}

// Called by engine_init on the engine's device, after every other buffer.  The buffers go into the
// engine's owner, which releases as many as were made; query_free deletes the host struct only.
static int query_init(tbgpu* E) {
    E->qs = new QueryState();
    {  // the log scan: per-tile counts and bounds, the answer, the unordered path's keys
        QueryBufs& Q = E->qs->q;
        Q.nb_cap = (E->xlog_cap + QUERY_THREADS - 1) / QUERY_THREADS;
        HIPCK(tbMalloc(E->own, &Q.d_counts, Q.nb_cap * 4));
        HIPCK(tbMalloc(E->own, &Q.d_mins, Q.nb_cap * 8));
        HIPCK(tbMalloc(E->own, &Q.d_maxs, Q.nb_cap * 8));
        HIPCK(tbMalloc(E->own, &Q.d_ordered, Q.nb_cap * 4));
        HIPCK(tbMalloc(E->own, &Q.d_base, Q.nb_cap * 8));
        HIPCK(tbMalloc(E->own, &Q.d_res, 16));
        HIPCK(tbHostMalloc(E->own, &Q.h_res, 16, hipHostMallocDefault));
        HIPCK(tbMalloc(E->own, &Q.d_out, (u64)BATCH_EVENTS_MAX * 128));
        HIPCK(tbMalloc(E->own, &Q.d_keys, (u64)QUERY_KEYS_CAP * 16));
        HIPCK(tbHostMalloc(E->own, &Q.h_keys, (u64)QUERY_KEYS_CAP * 16, hipHostMallocDefault));
        HIPCK(tbHostMalloc(E->own, &Q.h_base, (Q.nb_cap + 1) * 8, hipHostMallocDefault));
        if (const char* v = getenv("TBGPU_QUERY_COOP")) Q.coop = atoi(v) != 0;  // the load-shape measurement
    }
    {  // tbgpu_get_account_balances: the rows' timestamps and the bins
        BalanceBufs& B = E->qs->qb;
        HIPCK(tbMalloc(E->own, &B.d_ts, (u64)BATCH_EVENTS_MAX * 8));
        HIPCK(tbHostMalloc(E->own, &B.h_ts, (u64)BATCH_EVENTS_MAX * 8, hipHostMallocDefault));
        HIPCK(tbMalloc(E->own, &B.d_bins, BALANCE_SLOTS(BATCH_EVENTS_MAX) * BALANCE_SLOT_WORDS * 8));
        HIPCK(tbHostMalloc(E->own, &B.h_bins, BALANCE_SLOTS(BATCH_EVENTS_MAX) * BALANCE_SLOT_WORDS * 8, hipHostMallocDefault));
    }
    {  // tbgpu_query_accounts: per-tile counts and bounds, the select's state and histograms, keys, the answer
        AccountQueryBufs& A = E->qs->qa;
        A.nb = (E->account_cap + QUERY_THREADS - 1) / QUERY_THREADS;
        HIPCK(tbMalloc(E->own, &A.d_counts, A.nb * 4));
        HIPCK(tbMalloc(E->own, &A.d_mins, A.nb * 8));
        HIPCK(tbMalloc(E->own, &A.d_maxs, A.nb * 8));
        HIPCK(tbMalloc(E->own, &A.d_state, QA_STATE_BYTES));
        HIPCK(tbHostMalloc(E->own, &A.h_state, (u64)QA_WORDS * 8, hipHostMallocDefault));
        HIPCK(tbMalloc(E->own, &A.d_keys, (u64)BATCH_EVENTS_MAX * 16));
        HIPCK(tbMalloc(E->own, &A.d_out, (u64)BATCH_EVENTS_MAX * 128));
    }
    {  // tbgpu_get_change_events: the set, the bins, the accounts, the pending amounts, the rows
        ChangeBufs& C = E->qs->qc;
        const u64 na = CHANGE_ACCOUNTS_MAX, nr = CHANGE_EVENTS_MAX;
        HIPCK(tbMalloc(E->own, &C.d_set, (u64)CHANGE_SET_SLOTS_MAX * 4));
        HIPCK(tbMalloc(E->own, &C.d_ids, na * 16));
        HIPCK(tbMalloc(E->own, &C.d_pids, nr * 16));
        HIPCK(tbMalloc(E->own, &C.d_bins, (na + 1) * BALANCE_SLOT_WORDS * 8));
        HIPCK(tbMalloc(E->own, &C.d_accounts, na * 128));
        HIPCK(tbMalloc(E->own, &C.d_found, na * 4));
        HIPCK(tbMalloc(E->own, &C.d_p, nr * 16));
        HIPCK(tbMalloc(E->own, &C.d_found_p, nr * 4));
        HIPCK(tbHostMalloc(E->own, &C.h_set, (u64)CHANGE_SET_SLOTS_MAX * 4, hipHostMallocDefault));
        HIPCK(tbHostMalloc(E->own, &C.h_ids, na * 16, hipHostMallocDefault));
        HIPCK(tbHostMalloc(E->own, &C.h_pids, nr * 16, hipHostMallocDefault));
        HIPCK(tbHostMalloc(E->own, &C.h_bins, (na + 1) * BALANCE_SLOT_WORDS * 8, hipHostMallocDefault));
        HIPCK(tbHostMalloc(E->own, &C.h_accounts, na * 128, hipHostMallocDefault));
        HIPCK(tbHostMalloc(E->own, &C.h_found, na * 4, hipHostMallocDefault));
        HIPCK(tbHostMalloc(E->own, &C.h_p, nr * 16, hipHostMallocDefault));
        HIPCK(tbHostMalloc(E->own, &C.h_found_p, nr * 4, hipHostMallocDefault));
        HIPCK(tbHostMalloc(E->own, &C.h_rows, nr * 128, hipHostMallocDefault));
        HIPCK(tbHostMalloc(E->own, &C.h_row_idx, nr * 8, hipHostMallocDefault));
    }
    {  // tbgpu_get_account_transfers_many: the set, per-chunk counts, bases and bounds, the totals, the answers
        QueryManyBufs& M = E->qs->qm;
        const u64 nb_cap = E->qs->q.nb_cap;
        M.nc_cap = std::max<u64>((nb_cap + QUERY_MANY_TILES - 1) / QUERY_MANY_TILES, std::min<u64>(nb_cap, QUERY_MANY_CHUNKS_MIN));
        HIPCK(tbMalloc(E->own, &M.d_tab, sizeof(QueryManyTable)));
        HIPCK(tbHostMalloc(E->own, &M.h_tab, sizeof(QueryManyTable), hipHostMallocDefault));
        HIPCK(tbMalloc(E->own, &M.d_counts, M.nc_cap * QUERY_MANY_FILTERS * 4));
        HIPCK(tbMalloc(E->own, &M.d_base, M.nc_cap * QUERY_MANY_FILTERS * 4));
        HIPCK(tbMalloc(E->own, &M.d_cmin, M.nc_cap * 8));
        HIPCK(tbMalloc(E->own, &M.d_cmax, M.nc_cap * 8));
        HIPCK(tbMalloc(E->own, &M.d_cord, M.nc_cap * 4));
        HIPCK(tbMalloc(E->own, &M.d_ctiles, M.nc_cap * 8));
        HIPCK(tbMalloc(E->own, &M.d_res, QM_RES_WORDS * 8));
        HIPCK(tbHostMalloc(E->own, &M.h_res, QM_RES_WORDS * 8, hipHostMallocDefault));
        HIPCK(tbHostMalloc(E->own, &M.h_stage, (u64)QUERY_MANY_STAGE * 128, hipHostMallocDefault));
        HIPCK(tbMalloc(E->own, &M.d_out, (u64)QUERY_MANY_FILTERS * BATCH_EVENTS_MAX * 128));
    }
    // tbgpu_lookup_accounts_at: the ids, the set, the bins, the accounts, the answer, the result words
    if (const int st = account_scan_bufs_init(E, E->qs->ql, ASOF_IDS_MAX, CHANGE_SET_SLOTS_MAX, ASOF_BIN_BYTES(ASOF_IDS_MAX), 128)) return st;
    {  // tbgpu_get_ledger_balances: the set and the bins
        LedgerBufs& G = E->qs->qg;
        const u64 bin_bytes = LEDGER_BINS(LEDGER_SET_SLOTS_MAX) * LEDGER_BIN_WORDS * 8;
        HIPCK(tbMalloc(E->own, &G.d_set, (u64)LEDGER_SET_SLOTS_MAX * 4));
        HIPCK(tbHostMalloc(E->own, &G.h_set, (u64)LEDGER_SET_SLOTS_MAX * 4, hipHostMallocDefault));
        HIPCK(tbMalloc(E->own, &G.d_bins, bin_bytes));
        HIPCK(tbHostMalloc(E->own, &G.h_bins, bin_bytes, hipHostMallocDefault));
    }
    {  // tbgpu_get_pending_transfers: the states, the kept records, the set, the ids, the resolution slots
        PendingBufs& P = E->qs->qp;
        const u64 nr = PENDING_ROWS_MAX, set_bytes = (u64)tb_change_set_slots(PENDING_ROWS_MAX) * 4;
        HIPCK(tbMalloc(E->own, &P.d_states, nr + 1));
        HIPCK(tbHostMalloc(E->own, &P.h_states, nr + 1, hipHostMallocDefault));
        HIPCK(tbHostMalloc(E->own, &P.h_rows, nr * 128, hipHostMallocDefault));
        HIPCK(tbMalloc(E->own, &P.d_set, set_bytes));
        HIPCK(tbHostMalloc(E->own, &P.h_set, set_bytes, hipHostMallocDefault));
        HIPCK(tbMalloc(E->own, &P.d_ids, nr * 16));
        HIPCK(tbHostMalloc(E->own, &P.h_ids, nr * 16, hipHostMallocDefault));
        HIPCK(tbMalloc(E->own, &P.d_slots, nr * 128));
        HIPCK(tbHostMalloc(E->own, &P.h_slots, nr * 128, hipHostMallocDefault));
        HIPCK(tbHostMalloc(E->own, &P.h_row_of, nr * 4, hipHostMallocDefault));
    }
    // tbgpu_get_account_statements: the ids, the set, the bins, the accounts, the rows, the result words
    if (const int st = account_scan_bufs_init(E, E->qs->qt, STATEMENT_IDS_MAX, tb_change_set_slots(STATEMENT_IDS_MAX),
                                              STATEMENT_BIN_BYTES(STATEMENT_IDS_MAX), STATEMENT_ROW_BYTES)) {
        return st;
    }
    {  // tbgpu_get_account_balance_integrals: its bins; the rest is the statements call's
        IntegralBufs& I = E->qs->qi;
        HIPCK(tbMalloc(E->own, &I.d_bins, INTEGRAL_BIN_BYTES(INTEGRAL_IDS_MAX)));
        HIPCK(tbHostMalloc(E->own, &I.h_bins, INTEGRAL_BIN_BYTES(INTEGRAL_IDS_MAX), hipHostMallocDefault));
    }
    {  // tbgpu_get_account_statement_series: its bounds and its bins; the rest is the statements call's
        SeriesBufs& R = E->qs->qr;
        HIPCK(tbMalloc(E->own, &R.d_bounds, (u64)(SERIES_ROWS_MAX + 1) * 8));
        HIPCK(tbHostMalloc(E->own, &R.h_bounds, (u64)(SERIES_ROWS_MAX + 1) * 8, hipHostMallocDefault));
        HIPCK(tbMalloc(E->own, &R.d_bins, SERIES_BIN_BYTES(SERIES_KEYS_MAX)));
        HIPCK(tbHostMalloc(E->own, &R.h_bins, SERIES_BIN_BYTES(SERIES_KEYS_MAX), hipHostMallocDefault));
    }
    // tbgpu_get_account_flow_matrix: the ids of both lists, the set, the bins by key, the accounts, the cells, the result words
    if (const int st = account_scan_bufs_init(E, E->qs->qx, MATRIX_IDS_MAX, tb_change_set_slots(MATRIX_IDS_MAX),
                                              MATRIX_BIN_BYTES(MATRIX_CELLS_MAX), MATRIX_CELL_BYTES)) {
        return st;
    }
    {  // ... and its maps
        MatrixBufs& X = E->qs->qxm;
        HIPCK(tbMalloc(E->own, &X.d_maps, (u64)MATRIX_IDS_MAX * 4));
        HIPCK(tbHostMalloc(E->own, &X.h_maps, (u64)MATRIX_IDS_MAX * 4, hipHostMallocDefault));
    }
    {  // tbgpu_get_account_counterparties: the group table, the select's counts, state and keys, the rows
        CounterpartyBufs& K = E->qs->qk;
        K.groups = std::min<u64>(query_groups_hint ? query_groups_hint : E->cfg.accounts_max, 1ULL << 29);
        K.slots = pow2_at_least(2 * K.groups);
        HIPCK(tbMalloc(E->own, &K.d_table, K.slots * CP_SLOT_WORDS * 8));
        HIPCK(tbMalloc(E->own, &K.d_counts, (K.slots + QUERY_THREADS - 1) / QUERY_THREADS * 4));
        HIPCK(tbMalloc(E->own, &K.d_state, CP_STATE_BYTES));
        HIPCK(tbHostMalloc(E->own, &K.h_state, (u64)CP_WORDS * 8, hipHostMallocDefault));
        HIPCK(tbMalloc(E->own, &K.d_keys, (u64)CP_ROWS_MAX * CP_KEY_STRIDE * 8));
        HIPCK(tbMalloc(E->own, &K.d_out, (u64)CP_ROWS_MAX * CP_ROW_BYTES));
    }
    {  // tbgpu_get_account_balance_extremes: the element array, zone 0 and the flag words; the rest is the statements call's
        ExtremeBufs& X = E->qs->qe;
        const u64 per = (u64)CHANGE_THREADS * CHANGE_TILES, spans = std::max<u64>((E->xlog_cap + per - 1) / per, 1);
        X.elem_bytes = std::min<u64>(EXTREME_ARRAY_BYTES, std::min<u64>(spans, EXTREME_SLABS_MAX) * EXTREME_IDS_MAX * EXTREME_ELEM_BYTES);
        HIPCK(tbMalloc(E->own, &X.d_elems, X.elem_bytes));
        HIPCK(tbMalloc(E->own, &X.d_zone0, EXTREME_ZONE0_BYTES(EXTREME_IDS_MAX)));
        HIPCK(tbHostMalloc(E->own, &X.h_flags, EXTREME_FLAG_WORDS * 8, hipHostMallocDefault));
        if (const char* v = getenv("TBGPU_EXTREMES_SLABS")) X.slabs_cap = (u32)std::max(atoi(v), 0);
        if (const char* v = getenv("TBGPU_EXTREMES_EXACT")) X.exact = atoi(v) != 0;
    }
    return TBGPU_STATUS_OK;
}

static void query_free(tbgpu* E) { delete E->qs; }

// ---- the engine list and what every entry point does first and last --------------------------------
struct QueryCall {
    tbgpu* Es[NODE_WORLD_MAX];  // the engine itself, or a node's shards
    u32 world = 0;
    u32 k = 0;                  // records asked for: the filter's limit under the caller's room and k_max
};

// Lists the engines a query asks: the engine itself, or a node's shards.  Returns `complete`: of a log
// query (`evictable`), 1 while no listed engine has evicted a transfer; of the account table, always 1
// (accounts are never evicted).
static u32 query_engines(tbgpu* E, bool evictable, QueryCall* c) {
    u32 complete = 1;
    c->world = E->node ? node_world(E->node) : 1;
    for (u32 d = 0; d < c->world; d++) {
        c->Es[d] = E->node ? node_engine(E->node, d) : E;
        if (evictable && c->Es[d]->evicted_total) complete = 0;
    }
    return complete;
}

// A read: legal on a stopped engine, like the exports.  Zeroes `result`, lists the engines and sets
// `complete`.
template <typename FILTER>
static int query_begin(tbgpu* E, const char* name, const FILTER* filter, const void* out, u32 out_cap, u32 k_max,
                       bool evictable, tbgpu_query_result* result, QueryCall* c) {
    API_ENTER(E, false);
    if (!filter || !out || !result) return fail(TBGPU_STATUS_INVALID, "%s: a NULL filter, out or result", name);
    result->count = 0;
    result->matched = 0;
    result->complete = query_engines(E, evictable, c);
    c->k = std::min<u32>(std::min<u32>(filter->limit, out_cap), k_max);  // one reply is one message body
    return TBGPU_STATUS_OK;
}

// After any failing status the result names no records.
static int query_end(tbgpu_query_result* result, int status) {
    if (status) result->count = 0, result->matched = 0;
    return status;
}

// The first k records of `world` answers by their last word, the timestamp (the last k, newest first,
// under `reversed`): answer d is cnt[d] records of 128 B at recs + d * stride, in that order itself.
static u32 query_merge(const u8* recs, u64 stride, const u32* cnt, u32 world, u32 k, bool reversed, u8* out) {
    u32 at[NODE_WORLD_MAX] = {};
    u32 w = 0;
    for (; w < k; w++) {
        u32 pick = world;
        u64 best = 0;
        for (u32 d = 0; d < world; d++) {
            if (at[d] == cnt[d]) continue;
            u64 ts;
            memcpy(&ts, recs + d * stride + (u64)at[d] * 128 + 120, 8);
            if (pick == world || (reversed ? ts > best : ts < best)) pick = d, best = ts;
        }
        if (pick == world) break;
        memcpy(out + (u64)w * 128, recs + pick * stride + (u64)at[pick] * 128, 128);
        at[pick]++;
    }
    return w;
}

// The answers of the engines' enqueued scans into `out` (room for c.k records): one engine's as it
// is, a node's merged.  Every engine is waited for, whatever an earlier one returned.
template <typename COLLECT>
static int query_collect_all(const QueryCall& c, bool reversed, u8* out, tbgpu_query_result* result, COLLECT collect) {
    u32 cnt[NODE_WORLD_MAX] = {};
    u64 matched = 0;
    if (c.world == 1) {
        const int st = collect(c.Es[0], out, &cnt[0], &matched);
        if (st) return st;
        result->count = cnt[0];
        result->matched = matched;
        return TBGPU_STATUS_OK;
    }
    const u64 stride = (u64)std::max<u32>(c.k, 1) * 128;
    std::vector<u8> recs(c.world * stride);
    int status = TBGPU_STATUS_OK;
    for (u32 d = 0; d < c.world; d++) {
        u64 m = 0;
        const int st = collect(c.Es[d], recs.data() + d * stride, &cnt[d], &m);
        if (st && status == TBGPU_STATUS_OK) status = st;
        matched += m;
    }
    if (status) return status;
    result->count = query_merge(recs.data(), stride, cnt, c.world, c.k, reversed, out);
    result->matched = matched;
    return TBGPU_STATUS_OK;
}

// ---- get_account_transfers (k_query.h, include/tbgpu.h) -------------------------------------------
// The scan of one engine's log in two halves, so that a node runs its shards' scans side by side:
// query_enqueue puts count -> scan -> scatter on the engine stream (nothing crosses PCIe but the
// {total, ordered} word); query_collect waits, copies the answer's records, and runs the exact path
// of a log out of timestamp order when the scan found one.  The stream is drained before (a pending
// tbgpu_commit_device_async), so log_next is the log's end and nothing writes beside the scan.
static void query_keep_filter(QueryBufs& Q, const QueryFilter& F) { Q.F = F, Q.by_fields = false, Q.by_pending = false; }
static void query_keep_filter(QueryBufs& Q, const QueryFieldFilter& F) { Q.FF = F, Q.by_fields = true, Q.by_pending = false; }
static void query_keep_filter(QueryBufs& Q, const QueryPendingFilter& F) { Q.FP = F, Q.by_fields = false, Q.by_pending = true; }

template <typename FILTER>
static int query_enqueue(tbgpu* E, const FILTER& F, u32 k, bool reversed) {
    constexpr bool by_account = std::is_same<FILTER, QueryFilter>::value;
    QueryBufs& Q = E->qs->q;
    HIPCK(hipSetDevice(E->device));
    if (E->pending) {
        int st = engine_sync(E);
        if (st) return st;
    }
    query_keep_filter(Q, F);
    Q.k = k;
    Q.reversed = reversed;
    Q.n = E->log_next;
    Q.h_res[0] = Q.h_res[1] = 0;
    const u64 nb = (Q.n + QUERY_THREADS - 1) / QUERY_THREADS;
    if (nb == 0) return TBGPU_STATUS_OK;
    if (nb > Q.nb_cap) return fail(TBGPU_STATUS_PANIC, "query: the log's end %llu is past its capacity", (unsigned long long)Q.n);
    if constexpr (by_account) {
        if (Q.coop) {
            hipLaunchKernelGGL((tb_query_count<true, QueryFilter>), dim3((unsigned)nb), dim3(QUERY_THREADS), 0, E->stream, E->T,
                               F, Q.n, Q.d_counts, Q.d_mins, Q.d_maxs, Q.d_ordered);
        } else {
            hipLaunchKernelGGL((tb_query_count<false, QueryFilter>), dim3((unsigned)nb), dim3(QUERY_THREADS), 0, E->stream, E->T,
                               F, Q.n, Q.d_counts, Q.d_mins, Q.d_maxs, Q.d_ordered);
        }
    } else {
        hipLaunchKernelGGL((tb_query_count<false, FILTER>), dim3((unsigned)nb), dim3(QUERY_THREADS), 0, E->stream, E->T, F, Q.n,
                           Q.d_counts, Q.d_mins, Q.d_maxs, Q.d_ordered);
    }
    hipLaunchKernelGGL(tb_query_scan, dim3(1), dim3(1024), 0, E->stream, Q.d_counts, Q.d_mins, Q.d_maxs, Q.d_ordered, nb,
                       Q.d_base, Q.d_res);
    hipLaunchKernelGGL(tb_query_scatter<FILTER>, dim3((unsigned)nb), dim3(QUERY_THREADS), 0, E->stream, E->T, F, Q.n,
                       Q.d_counts, Q.d_base, Q.d_res, k, reversed ? 1u : 0u, Q.d_out);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(Q.h_res, Q.d_res, 16, hipMemcpyDeviceToHost, E->stream));
    return TBGPU_STATUS_OK;
}

// out: room for the enqueued k records.  *count = records written, *matched = every match.
static int query_collect(tbgpu* E, u8* out, u32* count, u64* matched) {
    QueryBufs& Q = E->qs->q;
    *count = 0;
    *matched = 0;
    const u64 nb = (Q.n + QUERY_THREADS - 1) / QUERY_THREADS;
    if (nb == 0) return TBGPU_STATUS_OK;
    HIPCK(hipSetDevice(E->device));
    HIPCK(hipStreamSynchronize(E->stream));
    const u64 total = Q.h_res[0];
    const bool ordered = Q.h_res[1] != 0;
    const u32 m = (u32)std::min<u64>(Q.k, total);
    *matched = total;
    if (m == 0) return TBGPU_STATUS_OK;
    if (!ordered) {
        // Exact with bounded memory: rounds over ranges of tiles whose matches fit the key buffer (the
        // bases say which), the best m keys kept across rounds, then one gather of their records.
        HIPCK(hipMemcpyAsync(Q.h_base, Q.d_base, nb * 8, hipMemcpyDeviceToHost, E->stream));
        HIPCK(hipStreamSynchronize(E->stream));
        Q.h_base[nb] = total;
        typedef std::pair<u64, u64> Key;  // {timestamp, position}
        std::vector<Key> best;
        const bool rev = Q.reversed;
        auto before = [rev](const Key& a, const Key& b) { return rev ? a > b : a < b; };
        auto cut = [&]() {
            if (best.size() <= m) return;
            std::nth_element(best.begin(), best.begin() + m, best.end(), before);
            best.resize(m);
        };
        u64 b0 = 0;
        while (b0 < nb && Q.h_base[b0] < total) {
            // Skip tiles without a match, then take tiles while their matches fit (a tile holds at most
            // QUERY_THREADS <= keys_max, so every round advances).
            b0 = (u64)(std::upper_bound(Q.h_base + b0, Q.h_base + nb + 1, Q.h_base[b0]) - Q.h_base) - 1;
            const u64 b1 = (u64)(std::upper_bound(Q.h_base + b0, Q.h_base + nb + 1, Q.h_base[b0] + Q.keys_max) - Q.h_base) - 1;
            const u64 keys = Q.h_base[b1] - Q.h_base[b0];
            if (b1 <= b0 || keys > Q.keys_max) return fail(TBGPU_STATUS_PANIC, "query: a round of %llu keys", (unsigned long long)keys);
            if (Q.by_pending) {
                hipLaunchKernelGGL(tb_query_keys<QueryPendingFilter>, dim3((unsigned)(b1 - b0)), dim3(QUERY_THREADS), 0, E->stream,
                                   E->T, Q.FP, Q.n, b0, Q.d_counts, Q.d_base, Q.d_keys, (u64)Q.keys_max);
            } else if (Q.by_fields) {
                hipLaunchKernelGGL(tb_query_keys<QueryFieldFilter>, dim3((unsigned)(b1 - b0)), dim3(QUERY_THREADS), 0, E->stream,
                                   E->T, Q.FF, Q.n, b0, Q.d_counts, Q.d_base, Q.d_keys, (u64)Q.keys_max);
            } else {
                hipLaunchKernelGGL(tb_query_keys<QueryFilter>, dim3((unsigned)(b1 - b0)), dim3(QUERY_THREADS), 0, E->stream, E->T,
                                   Q.F, Q.n, b0, Q.d_counts, Q.d_base, Q.d_keys, (u64)Q.keys_max);
            }
            HIPCK(hipGetLastError());
            HIPCK(hipMemcpyAsync(Q.h_keys, Q.d_keys, keys * 16, hipMemcpyDeviceToHost, E->stream));
            HIPCK(hipStreamSynchronize(E->stream));
            for (u64 i = 0; i < keys; i++) best.push_back(Key(Q.h_keys[2 * i], Q.h_keys[2 * i + 1]));
            if (best.size() > 2 * (size_t)m + Q.keys_max) cut();
            b0 = b1;
        }
        cut();
        std::sort(best.begin(), best.end(), before);
        if (best.size() != m) return fail(TBGPU_STATUS_PANIC, "query: %zu keys for %u matches", best.size(), m);
        for (u32 i = 0; i < m; i++) Q.h_keys[i] = best[i].second;
        HIPCK(hipMemcpyAsync(Q.d_keys, Q.h_keys, (u64)m * 8, hipMemcpyHostToDevice, E->stream));
        if (Q.by_pending) {  // the records and, beside them, their states
            hipLaunchKernelGGL(tb_pending_gather, dim3((m + QUERY_THREADS - 1) / QUERY_THREADS), dim3(QUERY_THREADS), 0, E->stream,
                               E->T, Q.FP, (const u64*)Q.d_keys, m, Q.n, Q.d_out);
        } else {
            hipLaunchKernelGGL(tb_query_gather, dim3((m + QUERY_THREADS - 1) / QUERY_THREADS), dim3(QUERY_THREADS), 0, E->stream,
                               E->T, Q.d_keys, m, Q.n, Q.d_out);
        }
        HIPCK(hipGetLastError());
    }
    if (Q.by_pending) HIPCK(hipMemcpyAsync(E->qs->qp.h_states, Q.FP.states, m, hipMemcpyDeviceToHost, E->stream));
    HIPCK(hipMemcpyAsync(out, Q.d_out, (u64)m * 128, hipMemcpyDeviceToHost, E->stream));
    HIPCK(hipStreamSynchronize(E->stream));
    *count = m;
    return TBGPU_STATUS_OK;
}

// The log scan under either predicate on every listed engine: result->count rows in `out`.
template <typename FILTER>
static int query_log_rows(const QueryCall& c, const FILTER& F, bool reversed, u8* out, tbgpu_query_result* result) {
    for (u32 d = 0; d < c.world; d++) {
        const int st = query_enqueue(c.Es[d], F, c.k, reversed);
        if (st) return st;
    }
    return query_collect_all(c, reversed, out, result, query_collect);
}

// The filter's rules (tbgpu.h): an invalid filter answers nothing, it is never a status.
static bool query_filter_valid(const tbgpu_account_filter* f) {
    if (tb_id_reserved(f->account_id_lo, f->account_id_hi)) return false;
    if (f->timestamp_min == ~0ULL || f->timestamp_max == ~0ULL) return false;
    if (f->timestamp_max != 0 && f->timestamp_max < f->timestamp_min) return false;
    if (f->limit == 0) return false;
    if (!(f->flags & (TBGPU_FILTER_DEBITS | TBGPU_FILTER_CREDITS))) return false;
    if (f->flags & ~(TBGPU_FILTER_DEBITS | TBGPU_FILTER_CREDITS | TBGPU_FILTER_REVERSED)) return false;
    for (u8 b : f->reserved) if (b) return false;
    return true;
}

static QueryFilter query_account_filter_of(const tbgpu_account_filter* f) {
    QueryFilter F{};
    F.id_lo = f->account_id_lo;
    F.id_hi = f->account_id_hi;
    F.ts_min = f->timestamp_min;
    F.ts_max = f->timestamp_max ? f->timestamp_max : ~0ULL;
    F.debits = (f->flags & TBGPU_FILTER_DEBITS) != 0;
    F.credits = (f->flags & TBGPU_FILTER_CREDITS) != 0;
    return F;
}

extern "C" int tbgpu_get_account_transfers(tbgpu_t* E, const tbgpu_account_filter* filter, void* out,
                                           uint32_t out_cap_records, tbgpu_query_result* result) {
    QueryCall c;
    if (const int st = query_begin(E, "get_account_transfers", filter, out, out_cap_records, BATCH_EVENTS_MAX, true, result, &c)) {
        return st;
    }
    if (!query_filter_valid(filter)) return TBGPU_STATUS_OK;
    const bool reversed = (filter->flags & TBGPU_FILTER_REVERSED) != 0;
    return query_end(result, query_log_rows(c, query_account_filter_of(filter), reversed, (u8*)out, result));
}

// ---- get_account_transfers_many (k_query_many.h, include/tbgpu.h) ----------------------------------
// A batch of account filters over one read of every listed engine's log.  The host builds the filter
// set once; query_many_enqueue puts the set's copy and count -> scan -> scatter on the engine stream
// and query_many_collect waits and copies each filter's records, as query_enqueue / query_collect do
// for one.  When the union of the hits is out of timestamp order (loads, upserts) the totals stand and
// each filter with a match is answered through query_enqueue / query_collect, which has the exact
// keyed rounds: rare, exact, and in the single query's buffers.
struct QueryManyCall {
    u32 nf = 0;
    const tbgpu_account_filter* filters = nullptr;
    bool valid[QUERY_MANY_FILTERS];
    u32 k[QUERY_MANY_FILTERS];  // records asked for: the limit under the caller's room and one message body
};

// The set of the call's valid filters: invalid ones are in no mask and match nothing.
static void query_many_table(const QueryManyCall& M, QueryManyTable* tab) {
    memset(tab, 0, sizeof *tab);
    for (u32 i = 0; i < M.nf; i++) {
        if (!M.valid[i]) continue;
        const QueryFilter F = query_account_filter_of(&M.filters[i]);
        u32 h = tb_qm_slot(F.id_lo, F.id_hi);  // at most 64 ids in 128 slots: an empty slot ends the probe
        while ((tab->id[h].x | tab->id[h].y) != 0 && !(tab->id[h].x == F.id_lo && tab->id[h].y == F.id_hi)) {
            h = (h + 1) & (QUERY_MANY_SLOTS - 1);
        }
        tab->id[h].x = F.id_lo, tab->id[h].y = F.id_hi;
        tab->mask[h] |= 1ULL << i;
        tab->ts_min[i] = F.ts_min, tab->ts_max[i] = F.ts_max;
        tab->k[i] = M.k[i];
        if (F.debits) tab->debits |= 1ULL << i;
        if (F.credits) tab->credits |= 1ULL << i;
        if (M.filters[i].flags & TBGPU_FILTER_REVERSED) tab->reversed |= 1ULL << i;
        if (F.ts_min != 0 || F.ts_max != ~0ULL) tab->windows = 1;
    }
}

// The set is in E's pinned h_tab.
static int query_many_enqueue(tbgpu* E) {
    QueryManyBufs& M = E->qs->qm;
    HIPCK(hipSetDevice(E->device));
    if (E->pending) {
        int st = engine_sync(E);
        if (st) return st;
    }
    M.n = E->log_next;
    for (u32 i = 0; i < QM_RES_WORDS; i++) M.h_res[i] = 0;
    const u64 nb = (M.n + QUERY_THREADS - 1) / QUERY_THREADS, nc = (nb + M.tiles - 1) / M.tiles;
    if (nc == 0) return TBGPU_STATUS_OK;
    if (nc > M.nc_cap) return fail(TBGPU_STATUS_PANIC, "query: the log's end %llu is past its capacity", (unsigned long long)M.n);
    HIPCK(hipMemcpyAsync(M.d_tab, M.h_tab, sizeof(QueryManyTable), hipMemcpyHostToDevice, E->stream));
    hipLaunchKernelGGL(tb_qm_count, dim3((unsigned)nc), dim3(QUERY_THREADS), 0, E->stream, E->T, (const QueryManyTable*)M.d_tab,
                       M.n, M.tiles, M.d_counts, M.d_cmin, M.d_cmax, M.d_cord, M.d_ctiles);
    hipLaunchKernelGGL(tb_qm_scan, dim3(1), dim3(1024), 0, E->stream, (const QueryManyTable*)M.d_tab, M.d_counts, M.d_cmin,
                       M.d_cmax, M.d_cord, nc, M.d_base, M.d_res);
    hipLaunchKernelGGL(tb_qm_scatter, dim3((unsigned)nc), dim3(QUERY_THREADS), 0, E->stream, E->T, (const QueryManyTable*)M.d_tab,
                       M.n, M.tiles, M.d_counts, M.d_base, M.d_ctiles, M.d_res, M.d_out);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(M.h_res, M.d_res, QM_RES_WORDS * 8, hipMemcpyDeviceToHost, E->stream));
    return TBGPU_STATUS_OK;
}

// Filter i's records go to out + off[i] (room for its k records); count[i] = records written,
// matched[i] = every match.
static int query_many_collect(tbgpu* E, const QueryManyCall& C, u8* out, const u64* off, u32* count, u64* matched) {
    QueryManyBufs& M = E->qs->qm;
    for (u32 i = 0; i < C.nf; i++) count[i] = 0, matched[i] = 0;
    HIPCK(hipSetDevice(E->device));
    HIPCK(hipStreamSynchronize(E->stream));
    if (M.n == 0) return TBGPU_STATUS_OK;
    const bool ordered = M.h_res[QM_RES_ORDERED] != 0;
    u64 totals[QUERY_MANY_FILTERS];
    for (u32 i = 0; i < C.nf; i++) totals[i] = C.valid[i] ? M.h_res[i] : 0;
    if (!ordered) {
        for (u32 i = 0; i < C.nf; i++) {
            if (totals[i] == 0) continue;
            const bool reversed = (C.filters[i].flags & TBGPU_FILTER_REVERSED) != 0;
            int st = query_enqueue(E, query_account_filter_of(&C.filters[i]), C.k[i], reversed);
            if (st == TBGPU_STATUS_OK) st = query_collect(E, out + off[i], &count[i], &matched[i]);
            if (st) return st;
            if (matched[i] != totals[i]) {
                return fail(TBGPU_STATUS_PANIC, "query: filter %u matched %llu records, then %llu", i,
                            (unsigned long long)totals[i], (unsigned long long)matched[i]);
            }
        }
        return TBGPU_STATUS_OK;
    }
    // The answers lie packed on the device: a copy per QUERY_MANY_STAGE records into the pinned stage,
    // and from there each filter's part into its slot.
    u64 start[QUERY_MANY_FILTERS + 1];
    start[0] = 0;
    for (u32 i = 0; i < C.nf; i++) {
        count[i] = (u32)std::min<u64>(C.k[i], totals[i]);
        matched[i] = totals[i];
        start[i + 1] = start[i] + count[i];
        if (count[i] && M.h_res[QM_RES_START + i] != start[i]) {
            return fail(TBGPU_STATUS_PANIC, "query: filter %u's records start at %llu, not %llu", i,
                        (unsigned long long)M.h_res[QM_RES_START + i], (unsigned long long)start[i]);
        }
    }
    const u64 all = start[C.nf];
    for (u64 p0 = 0; p0 < all; p0 += QUERY_MANY_STAGE) {
        const u64 p1 = std::min<u64>(all, p0 + QUERY_MANY_STAGE);
        HIPCK(hipMemcpyAsync(M.h_stage, M.d_out + p0 * 128, (p1 - p0) * 128, hipMemcpyDeviceToHost, E->stream));
        HIPCK(hipStreamSynchronize(E->stream));
        for (u32 i = 0; i < C.nf; i++) {
            const u64 a = std::max(p0, start[i]), b = std::min(p1, start[i + 1]);
            if (a < b) memcpy(out + off[i] + (a - start[i]) * 128, M.h_stage + (a - p0) * 128, (b - a) * 128);
        }
    }
    return TBGPU_STATUS_OK;
}

// Every listed engine scans its own log for the whole batch, side by side; one engine's answers go
// straight into the caller's buffer, a node's are merged per filter.  Every engine is waited for,
// whatever an earlier one returned.
static int query_many_rows(const QueryCall& c, const QueryManyCall& C, u8* out, u64 out_stride, tbgpu_query_result* results) {
    QueryManyTable* tab = c.Es[0]->qs->qm.h_tab;
    query_many_table(C, tab);
    for (u32 d = 0; d < c.world; d++) {
        if (d) memcpy(c.Es[d]->qs->qm.h_tab, tab, sizeof *tab);
        const int st = query_many_enqueue(c.Es[d]);
        if (st) return st;
    }
    u64 off[QUERY_MANY_FILTERS];
    u32 cnt[NODE_WORLD_MAX][QUERY_MANY_FILTERS];
    u64 matched[QUERY_MANY_FILTERS];
    if (c.world == 1) {
        for (u32 i = 0; i < C.nf; i++) off[i] = i * out_stride;
        const int st = query_many_collect(c.Es[0], C, out, off, cnt[0], matched);
        if (st) return st;
        for (u32 i = 0; i < C.nf; i++) results[i].count = cnt[0][i], results[i].matched = matched[i];
        return TBGPU_STATUS_OK;
    }
    u64 per = 0;  // one engine's answers: filter i's room of k records at off[i]
    for (u32 i = 0; i < C.nf; i++) off[i] = per, per += (u64)std::max<u32>(C.k[i], 1) * 128;
    std::vector<u8> recs(c.world * per);
    u64 sums[QUERY_MANY_FILTERS] = {};
    int status = TBGPU_STATUS_OK;
    for (u32 d = 0; d < c.world; d++) {
        const int st = query_many_collect(c.Es[d], C, recs.data() + d * per, off, cnt[d], matched);
        if (st && status == TBGPU_STATUS_OK) status = st;
        for (u32 i = 0; i < C.nf; i++) sums[i] += matched[i];
    }
    if (status) return status;
    for (u32 i = 0; i < C.nf; i++) {
        u32 ci[NODE_WORLD_MAX];
        for (u32 d = 0; d < c.world; d++) ci[d] = cnt[d][i];
        const bool reversed = (C.filters[i].flags & TBGPU_FILTER_REVERSED) != 0;
        results[i].count = query_merge(recs.data() + off[i], per, ci, c.world, C.k[i], reversed, out + i * out_stride);
        results[i].matched = sums[i];
    }
    return TBGPU_STATUS_OK;
}

extern "C" int tbgpu_get_account_transfers_many(tbgpu_t* E, const tbgpu_account_filter* filters, uint32_t n_filters, void* out,
                                                uint32_t out_cap_records, tbgpu_query_result* results) {
    API_ENTER(E, false);
    if (n_filters > TBGPU_QUERY_FILTERS_MAX) {
        return fail(TBGPU_STATUS_INVALID, "get_account_transfers_many: %u filters (at most %u)", n_filters, TBGPU_QUERY_FILTERS_MAX);
    }
    if (n_filters == 0) return TBGPU_STATUS_OK;
    if (!filters || !out || !results) return fail(TBGPU_STATUS_INVALID, "get_account_transfers_many: NULL filters, out or results");
    QueryCall c;
    const u32 complete = query_engines(E, true, &c);
    QueryManyCall C;
    C.nf = n_filters;
    C.filters = filters;
    bool any = false;
    for (u32 i = 0; i < n_filters; i++) {
        results[i].count = 0, results[i].matched = 0, results[i].complete = complete;
        C.valid[i] = query_filter_valid(&filters[i]);
        C.k[i] = C.valid[i] ? std::min<u32>(std::min<u32>(filters[i].limit, out_cap_records), BATCH_EVENTS_MAX) : 0;
        any |= C.valid[i];
    }
    if (!any) return TBGPU_STATUS_OK;
    const int st = query_many_rows(c, C, (u8*)out, (u64)out_cap_records * 128, results);
    if (st) {
        for (u32 i = 0; i < n_filters; i++) results[i].count = 0, results[i].matched = 0;
    }
    return st;
}

extern "C" int tbgpu_bench_query_many_tiles(tbgpu_t* E, uint32_t tiles) {
    API_ENTER(E, false);
    if (E->node) {
        for (u32 d = 0; d < node_world(E->node); d++) tbgpu_bench_query_many_tiles(node_engine(E->node, d), tiles);
        return TBGPU_STATUS_OK;
    }
    QueryManyBufs& M = E->qs->qm;
    M.tiles = tiles ? std::min<u32>(tiles, QUERY_MANY_TILES) : QUERY_MANY_TILES;
    while ((E->qs->q.nb_cap + M.tiles - 1) / M.tiles > M.nc_cap) M.tiles++;  // the chunks fit the buffers made at init
    return TBGPU_STATUS_OK;
}

// ---- get_account_balances (k_balances.h, include/tbgpu.h) -----------------------------------------
// The rows are get_account_transfers' answer, left in `out`; the second scan runs in two halves like
// the first, so that a node's shards scan side by side.  balance_enqueue: the rows' ascending
// timestamps (in B.h_ts) go to the device, the bins are zeroed, tb_balance_effects runs over this
// engine's log, and the k + 1 bins, the account's balances and the two flag words come back.
// NT: every engine whose log may hold a post's pending transfer (a single engine: itself).
static int balance_enqueue(tbgpu* E, const NodeTablesArgs& NT, u32 self, const QueryFilter& rows, u32 k) {
    BalanceBufs& B = E->qs->qb;
    HIPCK(hipSetDevice(E->device));
    QueryFilter F = rows;
    F.debits = F.credits = 1;  // the flags and the window choose rows, not what is summed
    F.ts_min = B.h_ts[0] + 1;
    F.ts_max = ~0ULL;
    const u64 n = E->log_next, per = (u64)QUERY_THREADS * BALANCE_TILES, nb = (n + per - 1) / per;
    const u64 bytes = BALANCE_SLOTS(k) * BALANCE_SLOT_WORDS * 8;
    HIPCK(hipMemcpyAsync(B.d_ts, B.h_ts, (u64)k * 8, hipMemcpyHostToDevice, E->stream));
    HIPCK(hipMemsetAsync(B.d_bins, 0, bytes, E->stream));
    // A shard without a record still answers for the account it may own: one workgroup.
    hipLaunchKernelGGL(tb_balance_effects, dim3((unsigned)std::max<u64>(nb, 1)), dim3(QUERY_THREADS), 0, E->stream, NT, self, F,
                       n, B.d_ts, k, B.d_bins);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(B.h_bins, B.d_bins, bytes, hipMemcpyDeviceToHost, E->stream));
    return TBGPU_STATUS_OK;
}

static int query_wait(tbgpu* E) {
    HIPCK(hipSetDevice(E->device));
    HIPCK(hipStreamSynchronize(E->stream));
    return TBGPU_STATUS_OK;
}

// `enqueue(d)` on every listed engine in turn, until one fails; then every engine that launched is
// waited for, whatever an earlier one returned.
template <typename ENQUEUE>
static int query_side_by_side(tbgpu* const* Es, u32 world, ENQUEUE enqueue) {
    int status = TBGPU_STATUS_OK;
    u32 issued = 0;
    for (; issued < world && status == TBGPU_STATUS_OK; issued++) status = enqueue(issued);
    for (u32 d = 0; d < issued; d++) {
        const int st = query_wait(Es[d]);
        if (st && status == TBGPU_STATUS_OK) status = st;
    }
    return status;
}

// The k rows' ascending timestamps from the k records of an answer (their last word).
static void balance_row_timestamps(const u8* out, u32 k, bool reversed, u64* ts) {
    for (u32 i = 0; i < k; i++) memcpy(&ts[i], out + (u64)(reversed ? k - 1 - i : i) * 128 + 120, 8);
}

// bins: [k + 1][4] summed over every engine that scanned; cur: the account's current balances.  Row i
// by timestamp holds cur minus the bins above i, per column modulo 2^128, and goes where record i was.
static void balance_write_rows(u8* out, u32 k, bool reversed, const u64* ts, const u128* bins, const u128 cur[4]) {
    u128 later[4] = {0, 0, 0, 0};
    for (u32 i = k; i-- > 0;) {
        tbgpu_account_balance row{};
        u64* w = &row.debits_pending_lo;
        for (u32 c = 0; c < 4; c++) {
            later[c] += bins[((u64)i + 1) * 4 + c];
            const u128 v = cur[c] - later[c];
            w[2 * c] = (u64)v, w[2 * c + 1] = (u64)(v >> 64);
        }
        row.timestamp = ts[i];
        memcpy(out + (u64)(reversed ? k - 1 - i : i) * 128, &row, 128);
    }
}

// The m rows in `out` become their balance rows.  Every listed engine gets the rows' timestamps in its
// own pinned buffer and scans its own log on its own stream; a post's pending transfer is read on
// home(pending_id) through the peers' tables, as tb_node_import reads owners.  The host adds the
// engines' bins into Es[0]'s in place (modulo 2^128, like the device; a slot is 4 x {lo, hi},
// little-endian, so the bins are u128s as they lie) and anchors them at the balances the account's
// owner holds.
static int balances_finish(const QueryCall& c, const QueryFilter& F, bool reversed, u32 m, u8* out, tbgpu_query_result* result) {
    BalanceBufs& B = c.Es[0]->qs->qb;
    balance_row_timestamps(out, m, reversed, B.h_ts);
    NodeTablesArgs NT{};
    NT.world = c.world;
    for (u32 d = 0; d < c.world; d++) NT.T[d] = c.Es[d]->T;
    const int status = query_side_by_side(c.Es, c.world, [&](u32 d) -> int {
        if (d) memcpy(c.Es[d]->qs->qb.h_ts, B.h_ts, (u64)m * 8);
        return balance_enqueue(c.Es[d], NT, d, F, m);
    });
    if (status) return status;
    const u64 flag_words = ((u64)m + 2) * BALANCE_SLOT_WORDS;  // behind the bins and the balances' slot
    const u64* owner = c.Es[tb_home(F.id_lo, F.id_hi, c.world)]->qs->qb.h_bins;
    if (!owner[flag_words + 1]) return fail(TBGPU_STATUS_PANIC, "get_account_balances: transfers name an account its owner lacks");
    u128 cur[4];
    memcpy(cur, owner + flag_words - BALANCE_SLOT_WORDS, sizeof cur);
    u128* bins = (u128*)B.h_bins;
    bool orphan = B.h_bins[flag_words] != 0;
    for (u32 d = 1; d < c.world; d++) {
        const u64* h = c.Es[d]->qs->qb.h_bins;
        for (u64 i = 0; i < ((u64)m + 1) * 4; i++) bins[i] += ((const u128*)h)[i];
        orphan |= h[flag_words] != 0;
    }
    balance_write_rows(out, m, reversed, B.h_ts, bins, cur);
    if (orphan) result->complete = 0;
    result->count = m;
    return TBGPU_STATUS_OK;
}

extern "C" int tbgpu_get_account_balances(tbgpu_t* E, const tbgpu_account_filter* filter, void* out,
                                          uint32_t out_cap_records, tbgpu_query_result* result) {
    QueryCall c;
    if (const int st = query_begin(E, "get_account_balances", filter, out, out_cap_records, BATCH_EVENTS_MAX, true, result, &c)) {
        return st;
    }
    if (!query_filter_valid(filter)) return TBGPU_STATUS_OK;
    const QueryFilter F = query_account_filter_of(filter);
    const bool reversed = (filter->flags & TBGPU_FILTER_REVERSED) != 0;
    int st = query_log_rows(c, F, reversed, (u8*)out, result);
    const u32 m = result->count;
    result->count = 0;
    if (st == TBGPU_STATUS_OK && m) st = balances_finish(c, F, reversed, m, (u8*)out, result);
    return query_end(result, st);
}

// ---- query_transfers / query_accounts (k_query.h, k_query_filter.h, include/tbgpu.h) --------------
static bool query_fields_valid(const tbgpu_query_filter* f) {
    if (f->timestamp_min == ~0ULL || f->timestamp_max == ~0ULL) return false;
    if (f->timestamp_max != 0 && f->timestamp_max < f->timestamp_min) return false;
    if (f->limit == 0) return false;
    if (f->flags & ~TBGPU_QUERY_REVERSED) return false;
    for (u8 b : f->reserved) if (b) return false;
    return true;
}

static QueryFieldFilter query_fields_of(const tbgpu_query_filter* f) {
    QueryFieldFilter F{};
    F.u128_lo = f->user_data_128_lo;
    F.u128_hi = f->user_data_128_hi;
    F.u64v = f->user_data_64;
    F.u32v = f->user_data_32;
    F.ledger = f->ledger;
    F.code = f->code;
    F.ts_min = f->timestamp_min;
    F.ts_max = f->timestamp_max ? f->timestamp_max : ~0ULL;
    return F;
}

extern "C" int tbgpu_query_transfers(tbgpu_t* E, const tbgpu_query_filter* filter, void* out, uint32_t out_cap_records,
                                     tbgpu_query_result* result) {
    QueryCall c;
    if (const int st = query_begin(E, "query_transfers", filter, out, out_cap_records, BATCH_EVENTS_MAX, true, result, &c)) return st;
    if (!query_fields_valid(filter)) return TBGPU_STATUS_OK;
    const bool reversed = (filter->flags & TBGPU_QUERY_REVERSED) != 0;
    return query_end(result, query_log_rows(c, query_fields_of(filter), reversed, (u8*)out, result));
}

// k_select.h's passes and its collect on `stream`, back to back, over source S's nb tiles (a pass with
// nothing to decide exits on the device).  st: the state the caller started; hist: `passes` zeroed histograms.
template <typename SRC>
static void select_enqueue(hipStream_t stream, const SRC& S, u64 nb, u32 k, u32 passes, u64* st, u32* hist, const u32* counts, u64* keys) {
    const unsigned wide = (unsigned)((nb + SEL_TILES - 1) / SEL_TILES);
    for (u32 pass = 0; pass < passes; pass++) {
        hipLaunchKernelGGL(tb_select_hist<SRC>, dim3(wide), dim3(QUERY_THREADS), 0, stream, S, counts, nb, k, pass, (const u64*)st, hist);
        hipLaunchKernelGGL(tb_select_pick, dim3(1), dim3(1024), 0, stream, k, pass, (const u32*)hist, st);
    }
    hipLaunchKernelGGL(tb_select_collect<SRC>, dim3(wide), dim3(QUERY_THREADS), 0, stream, S, counts, nb, k, st, keys);
}

// The select's state words, back on the host: it collected the m = min(k, total) entries asked for.
static int select_check(const char* name, const char* what, const u64* h_state, u32 k, u32 m) {
    if (std::min<u64>(k, h_state[SEL_NKEYS]) == m) return TBGPU_STATUS_OK;
    return fail(TBGPU_STATUS_PANIC, "%s: %llu keys selected for %u of %llu %s", name, (unsigned long long)h_state[SEL_NKEYS], m,
                (unsigned long long)h_state[SEL_TOTAL], what);
}

// The account table in two halves, as the log scan: account_query_enqueue puts count -> scan -> the
// select's passes -> collect -> emit on the engine stream, back to back (a pass that has nothing to
// decide exits on the device); account_query_collect waits for the state words, then copies the
// answer's records.  Nothing else crosses PCIe.  world != 0: a node shard answers for what it owns.
static int account_query_enqueue(tbgpu* E, const QueryFieldFilter& F, u32 world, u32 self, u32 k, bool reversed) {
    AccountQueryBufs& A = E->qs->qa;
    HIPCK(hipSetDevice(E->device));
    if (E->pending) {
        int st = engine_sync(E);
        if (st) return st;
    }
    A.k = k;
    QaPred P{};
    P.f = F;
    P.world = world;
    P.self = self;
    P.cold = F.wants_u128() || F.u64v || F.u32v;
    const u64 cap = E->account_cap, nb = A.nb;
    HIPCK(hipMemsetAsync(A.d_state, 0, QA_STATE_BYTES, E->stream));
    hipLaunchKernelGGL(tb_qa_count, dim3((unsigned)nb), dim3(QUERY_THREADS), 0, E->stream, E->T, P, cap, A.d_counts, A.d_mins,
                       A.d_maxs);
    hipLaunchKernelGGL(tb_qa_scan, dim3(1), dim3(1024), 0, E->stream, A.d_counts, A.d_mins, A.d_maxs, nb, k, A.d_state);
    if (k) {
        select_enqueue(E->stream, QaSource{E->T, P, cap, reversed ? 1u : 0u, A.d_state}, nb, k, QA_PASSES, A.d_state,
                       (u32*)(A.d_state + QA_WORDS), A.d_counts, A.d_keys);
        hipLaunchKernelGGL(tb_qa_emit, dim3((k + SEL_EMIT_KEYS - 1) / SEL_EMIT_KEYS), dim3(QUERY_THREADS), 0, E->stream, E->T, cap, k,
                           A.d_state, A.d_keys, A.d_out);
    }
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(A.h_state, A.d_state, (u64)QA_WORDS * 8, hipMemcpyDeviceToHost, E->stream));
    return TBGPU_STATUS_OK;
}

static int account_query_collect(tbgpu* E, u8* out, u32* count, u64* matched) {
    AccountQueryBufs& A = E->qs->qa;
    *count = 0;
    *matched = 0;
    HIPCK(hipSetDevice(E->device));
    HIPCK(hipStreamSynchronize(E->stream));
    const u64 total = A.h_state[SEL_TOTAL];
    const u32 m = (u32)std::min<u64>(A.k, total);
    A.last_scans = A.h_state[SEL_SCANS];
    *matched = total;
    if (m == 0) return TBGPU_STATUS_OK;
    if (const int st = select_check("query_accounts", "matches", A.h_state, A.k, m)) return st;
    HIPCK(hipMemcpyAsync(out, A.d_out, (u64)m * 128, hipMemcpyDeviceToHost, E->stream));
    HIPCK(hipStreamSynchronize(E->stream));
    *count = m;
    return TBGPU_STATUS_OK;
}

// A node's shard d answers for the accounts with tb_home(id, world) == d — a home's imported copies of
// foreign accounts do not match; the one engine owns every account and makes no owner test (world 0).
extern "C" int tbgpu_query_accounts(tbgpu_t* E, const tbgpu_query_filter* filter, void* out, uint32_t out_cap_records,
                                    tbgpu_query_result* result) {
    QueryCall c;
    if (const int st = query_begin(E, "query_accounts", filter, out, out_cap_records, BATCH_EVENTS_MAX, false, result, &c)) return st;
    if (!query_fields_valid(filter)) return TBGPU_STATUS_OK;
    const QueryFieldFilter F = query_fields_of(filter);
    const bool reversed = (filter->flags & TBGPU_QUERY_REVERSED) != 0;
    for (u32 d = 0; d < c.world; d++) {
        const int st = account_query_enqueue(c.Es[d], F, c.world > 1 ? c.world : 0, d, c.k, reversed);
        if (st) return st;
    }
    return query_end(result, query_collect_all(c, reversed, (u8*)out, result, account_query_collect));
}

extern "C" int tbgpu_bench_query_select_scans(tbgpu_t* E, uint64_t* scans) {
    API_ENTER(E, false);
    if (E->node) E = node_engine(E->node, 0);
    *scans = E->qs->qa.last_scans;
    return TBGPU_STATUS_OK;
}

extern "C" int tbgpu_bench_query_keys_max(tbgpu_t* E, uint32_t keys) {
    API_ENTER(E, false);
    if (E->node) {
        for (u32 d = 0; d < node_world(E->node); d++) tbgpu_bench_query_keys_max(node_engine(E->node, d), keys);
        return TBGPU_STATUS_OK;
    }
    E->qs->q.keys_max = keys ? std::min<u32>(std::max<u32>(keys, QUERY_THREADS), QUERY_KEYS_CAP) : QUERY_KEYS_CAP;
    return TBGPU_STATUS_OK;
}

// ---- get_change_events (k_change_events.h, include/tbgpu.h) ---------------------------------------
// The rows are query_transfers' answer for an all-zero field filter.  change_events_finish takes them
// (m > 0, ascending by timestamp, on the host) with the engines whose logs hold the ledger — one, or a
// node's shards — and writes the m events into `out`:
//   the set      the rows' distinct accounts, an index each, in an open-addressing table the host
//                builds in Es[0]'s pinned buffers (a node copies it into every shard's);
//   the scans    every engine, on its own device and stream, side by side: set and ids up, bins zeroed,
//                tb_change_effects over its own log for the records above the last row, bins back;
//   the gather   Es[0]'s stream: each account's record from its owner, each post row's pending amount
//                from home(pending_id), through the peers' tables as tb_balance_effects reads them;
//   the walk     end(a) = current(a) - the engines' bins; the rows from the newest to the oldest, each
//                written with its two accounts' balances and then taken out of them.
static u32 change_set_insert(u32* set, u32 mask, u64* ids, u32* count, u64 lo, u64 hi) {
    const u64 h = tb_change_hash(lo, hi);
    const u32 tag = (u32)(h >> 48);
    u32 s = (u32)h & mask;
    for (;;) {  // the table is at most half full: an empty slot ends the probe
        const u32 e = set[s];
        if (e == 0) break;
        if ((e >> 16) == tag) {
            const u32 index = (e & 0xFFFFu) - 1;
            if (ids[2 * (u64)index] == lo && ids[2 * (u64)index + 1] == hi) return index;
        }
        s = (s + 1) & mask;
    }
    const u32 index = (*count)++;
    ids[2 * (u64)index] = lo, ids[2 * (u64)index + 1] = hi;
    set[s] = tb_change_entry(h, index);
    return index;
}

static u64 change_row_word(const u8* row, u32 word) {
    u64 v;
    memcpy(&v, row + 8 * word, 8);
    return v;
}

// The walk.  rows: m records, ascending; row_idx: [m][2] their debit and credit account's index;
// accounts, found: the indexed accounts' records and whether their owner holds them; p, found_p: the
// post rows' pending amounts and whether they were resident; bal: [accounts][4] the balances after the
// newest row, taken apart row by row.  Writes the m events of 384 B; false: an orphan post among the rows.
static bool change_walk(const u8* rows, u32 m, const u32* row_idx, const u8* accounts, const u32* found, const u64* p,
                        const u32* found_p, u128* bal, u8* out) {
    bool complete = true;
    for (u32 i = m; i-- > 0;) {
        const u8* r = rows + (u64)i * 128;
        u8* ev = out + (u64)i * 384;
        memcpy(ev, r, 128);
        for (u32 side = 0; side < 2; side++) {
            const u32 a = row_idx[2 * i + side];
            u8* block = ev + 128 + 128 * side;
            if (!found[a]) {
                memset(block, 0, 128);
                continue;
            }
            memcpy(block, accounts + (u64)a * 128, 128);
            memcpy(block + 16, &bal[(u64)a * 4], 64);
        }
        // The row's own effect leaves its two accounts: the balances of the next older row.
        const u128 amount = tb_u128(change_row_word(r, 6), change_row_word(r, 7));
        const u32 tf = (u32)(change_row_word(r, 14) >> 48);
        u128 pending = amount;
        if (tb_effect_is_post(tf)) {
            if (found_p[i]) pending = tb_u128(p[2 * (u64)i], p[2 * (u64)i + 1]);
            else complete = false;
        }
        const BalanceEffect e = tb_balance_effect(tf, amount, pending);
        for (u32 side = 0; side < 2; side++) {
            u128* b = &bal[(u64)row_idx[2 * i + side] * 4 + 2 * side];
            b[0] -= e.pend, b[1] -= e.post;
        }
    }
    return complete;
}

static int change_events_finish(tbgpu* const* Es, u32 world, const u8* rows, u32 m, u8* out, tbgpu_query_result* result) {
    ChangeBufs& C = Es[0]->qs->qc;
    u32 slots = tb_change_set_slots(2 * m), mask = slots - 1;  // for now: the accounts are at most 2m
    memset(C.h_set, 0, (u64)slots * 4);
    u32 na = 0;
    for (u32 i = 0; i < m; i++) {
        const u8* r = rows + (u64)i * 128;
        for (u32 side = 0; side < 2; side++) {
            C.h_row_idx[2 * i + side] =
                change_set_insert(C.h_set, mask, C.h_ids, &na, change_row_word(r, 2 + 2 * side), change_row_word(r, 3 + 2 * side));
        }
        const bool post = tb_effect_is_post((u32)(change_row_word(r, 14) >> 48));
        C.h_pids[2 * (u64)i] = post ? change_row_word(r, 8) : 0;
        C.h_pids[2 * (u64)i + 1] = post ? change_row_word(r, 9) : 0;
    }
    if (tb_change_set_slots(na) < slots) {  // fewer distinct accounts: the smaller table, the same indices
        slots = tb_change_set_slots(na), mask = slots - 1;
        memset(C.h_set, 0, (u64)slots * 4);
        u32 again = 0;
        for (u32 a = 0; a < na; a++) change_set_insert(C.h_set, mask, C.h_ids, &again, C.h_ids[2 * (u64)a], C.h_ids[2 * (u64)a + 1]);
    }
    const u32 lds_bins = tb_change_lds_bins(slots);
    const u64 t_last = change_row_word(rows + (u64)(m - 1) * 128, 15);
    const u64 bin_bytes = ((u64)na + 1) * BALANCE_SLOT_WORDS * 8;
    NodeTablesArgs NT{};
    NT.world = world;
    for (u32 d = 0; d < world; d++) NT.T[d] = Es[d]->T;
    const int status = query_side_by_side(Es, world, [&](u32 d) -> int {
        tbgpu* E = Es[d];
        ChangeBufs& D = E->qs->qc;
        HIPCK(hipSetDevice(E->device));
        if (d) {
            memcpy(D.h_set, C.h_set, (u64)slots * 4);
            memcpy(D.h_ids, C.h_ids, (u64)na * 16);
        }
        HIPCK(hipMemcpyAsync(D.d_set, D.h_set, (u64)slots * 4, hipMemcpyHostToDevice, E->stream));
        HIPCK(hipMemcpyAsync(D.d_ids, D.h_ids, (u64)na * 16, hipMemcpyHostToDevice, E->stream));
        HIPCK(hipMemsetAsync(D.d_bins, 0, bin_bytes, E->stream));
        const u64 n = E->log_next, per = (u64)CHANGE_THREADS * CHANGE_TILES, nb = (n + per - 1) / per;
        if (nb) {
            hipLaunchKernelGGL((tb_change_effects<u32, false>), dim3((unsigned)nb), dim3(CHANGE_THREADS),
                               (size_t)slots * 4 + (size_t)lds_bins * BALANCE_SLOT_WORDS * 8, E->stream, NT, d, n, t_last,
                               (const u32*)D.d_set, mask, (const u64*)D.d_ids, na, D.d_bins, lds_bins);
            HIPCK(hipGetLastError());
        }
        HIPCK(hipMemcpyAsync(D.h_bins, D.d_bins, bin_bytes, hipMemcpyDeviceToHost, E->stream));
        if (d == 0) {
            HIPCK(hipMemcpyAsync(D.d_pids, D.h_pids, (u64)m * 16, hipMemcpyHostToDevice, E->stream));
            hipLaunchKernelGGL(tb_change_gather, dim3((std::max(na, m) + QUERY_THREADS - 1) / QUERY_THREADS), dim3(QUERY_THREADS), 0,
                               E->stream, NT, (const u64*)D.d_ids, na, D.d_accounts, D.d_found, (const u64*)D.d_pids, m, D.d_p,
                               D.d_found_p);
            HIPCK(hipGetLastError());
            HIPCK(hipMemcpyAsync(D.h_accounts, D.d_accounts, (u64)na * 128, hipMemcpyDeviceToHost, E->stream));
            HIPCK(hipMemcpyAsync(D.h_found, D.d_found, (u64)na * 4, hipMemcpyDeviceToHost, E->stream));
            HIPCK(hipMemcpyAsync(D.h_p, D.d_p, (u64)m * 16, hipMemcpyDeviceToHost, E->stream));
            HIPCK(hipMemcpyAsync(D.h_found_p, D.d_found_p, (u64)m * 4, hipMemcpyDeviceToHost, E->stream));
        }
        return TBGPU_STATUS_OK;
    });
    if (status) return status;
    bool complete = result->complete != 0;
    // end(a): into Es[0]'s bins in place, as u128s (a slot is 4 x {lo, hi}, little-endian).
    u128* bal = (u128*)C.h_bins;
    for (u32 d = 0; d < world; d++) complete &= Es[d]->qs->qc.h_bins[(u64)na * BALANCE_SLOT_WORDS + CHANGE_FLAG_ORPHAN] == 0;
    for (u32 a = 0; a < na; a++) {
        const u8* rec = C.h_accounts + (u64)a * 128;
        for (u32 c = 0; c < 4; c++) {
            u128 sum = bal[(u64)a * 4 + c];
            for (u32 d = 1; d < world; d++) sum += ((const u128*)Es[d]->qs->qc.h_bins)[(u64)a * 4 + c];
            const u128 cur = C.h_found[a] ? tb_u128(change_row_word(rec, 2 + 2 * c), change_row_word(rec, 3 + 2 * c)) : (u128)0;
            bal[(u64)a * 4 + c] = cur - sum;
        }
        complete &= C.h_found[a] != 0;
    }
    complete &= change_walk(rows, m, C.h_row_idx, C.h_accounts, C.h_found, C.h_p, C.h_found_p, bal, out);
    result->complete = complete ? 1 : 0;
    result->count = m;
    return TBGPU_STATUS_OK;
}

static bool change_filter_valid(const tbgpu_change_events_filter* f) {
    if (f->timestamp_min == ~0ULL || f->timestamp_max == ~0ULL) return false;
    if (f->timestamp_max != 0 && f->timestamp_max < f->timestamp_min) return false;
    if (f->limit == 0) return false;
    for (u8 b : f->reserved) if (b) return false;
    return true;
}

// The rows go to Es[0]'s pinned h_rows: one engine's answer as it is, a node's merged.
extern "C" int tbgpu_get_change_events(tbgpu_t* E, const tbgpu_change_events_filter* filter, void* out,
                                       uint32_t out_cap_events, tbgpu_query_result* result) {
    QueryCall c;
    if (const int st = query_begin(E, "get_change_events", filter, out, out_cap_events, CHANGE_EVENTS_MAX, true, result, &c)) return st;
    if (!change_filter_valid(filter)) return TBGPU_STATUS_OK;
    QueryFieldFilter F{};
    F.ts_min = filter->timestamp_min;
    F.ts_max = filter->timestamp_max ? filter->timestamp_max : ~0ULL;
    u8* rows = c.Es[0]->qs->qc.h_rows;
    int st = query_log_rows(c, F, false, rows, result);
    const u32 m = result->count;
    result->count = 0;
    if (st == TBGPU_STATUS_OK && m) st = change_events_finish(c.Es, c.world, rows, m, (u8*)out, result);
    return query_end(result, st);
}

// ---- the account-set scan (k_account_scan.h; k_asof.h, k_statement.h, k_integral.h, k_series.h) ----
// lookup_accounts_at, get_account_statements, get_account_balance_integrals and
// get_account_statement_series through one driver.  One engine: ids up, set and bins zeroed,
// tb_asof_gather -> the call's scan -> the call's emit on the engine stream, the result words back; one
// wait; then the answer's count rows.  The set has get_change_events' slots for as many accounts as
// the request has ids (tb_change_set_slots).  A node: every shard gathers (each builds the same set:
// an id's index is its smallest request position, whatever the order of the inserts; the records come
// from the owners' tables, as tb_change_gather reads them) and scans its own log on its own device
// and stream, side by side; the host adds the shards' bins (account_scan_host.h) and writes the rows
// with the call's row function.  An entry point describes its call in an AccountScan and owns
// nothing else but its validity test.

// What a call's launch callables get: one engine's part of the call.
struct ScanLaunch {
    tbgpu* E;
    const NodeTablesArgs& NT;
    u32 self;
    u64 records;  // the log's end
    unsigned nb;  // the scan's workgroups
    u32 slots, mask;
    AccountScanBufs& B;
    u64* d_bins;
    u32 cap;
};
struct ScanBins {
    u64 *d, *h;
};

struct AccountScan {
    const char* name;                   // in messages
    const char* unit;                   // what the call returns, in the panic message
    std::string asked;                  // what it was asked for, likewise
    AccountScanBufs QueryState::*bufs;  // the ids, set, records, flags, out and res
    ScanBins (*bins)(QueryState&);      // the bins and their pinned mirror
    u32 n;                              // request ids
    u64 T;                              // tb_asof_gather's T
    bool scan;           // false: the records as they are — no set, no scan, no bins, and a node asks its first shard only
    u64 bin_bytes;       // the request's bins and their flag word
    u64 flag_word;       // the orphan flag's word in the bins
    const ScanBinRun* layout;  // a bin's sums, for a node's adder
    u32 n_runs;
    u32 keys_per_id;     // consecutive bins of one id
    u32 row_bytes;
    u32 rows_per_id;     // `matched` is at most n * rows_per_id
    std::function<int(const ScanLaunch&)> launch_scan, launch_emit;
};

#define SCAN_ANSWERED (-1)  // account_scan_begin: nothing to ask, the result stands as it is

// What every entry point does before it describes its call (after API_ENTER): the checks, the zeroed
// result, the engine list, `valid()` — false: the zeroed result is the answer — every engine drained,
// the tables, the ids into every shard's pinned buffer.
template <typename VALID>
static int account_scan_begin(tbgpu* E, const char* name, AccountScanBufs QueryState::*bufs, u32 n, u32 n_max, const void* ids,
                              const void* out, tbgpu_query_result* result, QueryCall* c, NodeTablesArgs* NT, VALID valid) {
    if (n > n_max) return fail(TBGPU_STATUS_INVALID, "%s: %u ids (at most %u)", name, n, n_max);
    if (n == 0) return SCAN_ANSWERED;
    if (!ids || !out || !result) return fail(TBGPU_STATUS_INVALID, "%s: NULL ids, out or result", name);
    result->count = 0;
    result->matched = 0;
    result->complete = query_engines(E, true, c);
    if (!valid()) return SCAN_ANSWERED;
    *NT = NodeTablesArgs{};
    NT->world = c->world;
    for (u32 d = 0; d < c->world; d++) NT->T[d] = c->Es[d]->T;
    // Every engine is drained before any is asked: a gather reads the owners' tables and a scan its
    // posts' pending transfers on their homes.
    for (u32 d = 0; d < c->world; d++) {
        HIPCK(hipSetDevice(c->Es[d]->device));
        if (c->Es[d]->pending) {
            const int st = engine_sync(c->Es[d]);
            if (st) return query_end(result, st);
        }
    }
    for (u32 d = 0; d < c->world; d++) memcpy((c->Es[d]->qs->*bufs).h_ids, ids, (u64)n * 16);
    return TBGPU_STATUS_OK;
}

static int account_scan_enqueue(tbgpu* E, const AccountScan& s, const NodeTablesArgs& NT, u32 self, bool emit, u32 cap) {
    AccountScanBufs& B = E->qs->*s.bufs;
    const ScanBins bins = s.bins(*E->qs);
    HIPCK(hipSetDevice(E->device));
    const u32 n = s.n, slots = tb_change_set_slots(n), mask = slots - 1;
    const unsigned nb_ids = (n + QUERY_THREADS - 1) / QUERY_THREADS;
    HIPCK(hipMemcpyAsync(B.d_ids, B.h_ids, (u64)n * 16, hipMemcpyHostToDevice, E->stream));
    if (s.scan) {
        HIPCK(hipMemsetAsync(B.d_set, 0, (u64)slots * 4, E->stream));
        HIPCK(hipMemsetAsync(bins.d, 0, s.bin_bytes, E->stream));
    }
    const bool store = emit || self == 0;  // a node reads the first shard's records only
    hipLaunchKernelGGL(tb_asof_gather, dim3(nb_ids), dim3(QUERY_THREADS), 0, E->stream, NT, (const u64*)B.d_ids, n, s.T,
                       store ? B.d_accounts : nullptr, store ? B.d_found : nullptr, s.scan ? B.d_set : nullptr, mask);
    HIPCK(hipGetLastError());
    const u64 records = E->log_next, per = (u64)CHANGE_THREADS * CHANGE_TILES, nb = (records + per - 1) / per;
    const ScanLaunch L{E, NT, self, records, (unsigned)nb, slots, mask, B, bins.d, cap};
    if (s.scan && nb) {
        if (const int st = s.launch_scan(L)) return st;
        HIPCK(hipGetLastError());
    }
    if (emit) {
        if (const int st = s.launch_emit(L)) return st;
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(B.h_res, B.d_res, SCAN_RES_WORDS * 8, hipMemcpyDeviceToHost, E->stream));
        return TBGPU_STATUS_OK;
    }
    if (s.scan) HIPCK(hipMemcpyAsync(bins.h, bins.d, s.bin_bytes, hipMemcpyDeviceToHost, E->stream));
    if (self == 0) {
        HIPCK(hipMemcpyAsync(B.h_accounts, B.d_accounts, (u64)n * 128, hipMemcpyDeviceToHost, E->stream));
        HIPCK(hipMemcpyAsync(B.h_found, B.d_found, (u64)n * 4, hipMemcpyDeviceToHost, E->stream));
    }
    return TBGPU_STATUS_OK;
}

// A node's answer from its shards' pinned mirrors: the found positions in request order, each from
// its record and the sum of every shard's bins of its id (null without a scan).  `rows(account, bins,
// first, out)` writes the position's rows — `first` is the first of them, and below `cap` — under the
// caller's room and returns how many it wrote.
template <typename ROWS>
static void account_scan_node_rows(const QueryCall& c, const AccountScan& s, u32 cap, u8* out, tbgpu_query_result* result, ROWS rows) {
    const AccountScanBufs& B = c.Es[0]->qs->*s.bufs;
    const u64 id_words = (u64)s.keys_per_id * scan_bin_words(s.layout, s.n_runs);
    std::vector<u32> index;
    if (s.scan) index = scan_first_positions(B.h_ids, s.n);
    std::vector<u64> sum(s.scan ? id_words : 0);
    u64 m = 0;
    u32 written = 0;
    for (u32 i = 0; i < s.n; i++) {
        if (!B.h_found[i]) continue;
        const u64 first = m;
        m += s.rows_per_id;
        if (first >= cap) continue;
        std::fill(sum.begin(), sum.end(), 0);
        for (u32 d = 0; d < c.world && s.scan; d++) {
            scan_bins_add(sum.data(), s.bins(*c.Es[d]->qs).h + index[i] * id_words, s.layout, s.n_runs, s.keys_per_id);
        }
        written += rows((const u64*)(B.h_accounts + (u64)i * 128), s.scan ? sum.data() : nullptr, first, out);
    }
    for (u32 d = 0; d < c.world && s.scan; d++) {
        if (s.bins(*c.Es[d]->qs).h[s.flag_word]) result->complete = 0;
    }
    result->count = written;
    result->matched = m;
}

// One engine's answer: the result words are back, the rows follow.
static int account_scan_finish(tbgpu* E, const AccountScan& s, u32 cap, void* out, tbgpu_query_result* result) {
    const AccountScanBufs& B = E->qs->*s.bufs;
    const u64 matched = B.h_res[SCAN_RES_MATCHED];
    const u32 m = (u32)std::min<u64>(matched, cap);
    if (matched > (u64)s.n * s.rows_per_id) {
        return query_end(result, fail(TBGPU_STATUS_PANIC, "%s: %llu %s for %s", s.name, (unsigned long long)matched, s.unit, s.asked.c_str()));
    }
    if (m) {
        HIPCK(hipMemcpyAsync(out, B.d_out, (u64)m * s.row_bytes, hipMemcpyDeviceToHost, E->stream));
        HIPCK(hipStreamSynchronize(E->stream));
    }
    if (B.h_res[SCAN_RES_ORPHAN]) result->complete = 0;
    result->count = m;
    result->matched = matched;
    return TBGPU_STATUS_OK;
}

// The driver.  `node()` writes a node's answer from its shards' pinned mirrors, once every shard is back.
template <typename NODE>
static int account_scan_run_node(const QueryCall& c, const AccountScan& s, const NodeTablesArgs& NT, u32 cap, void* out,
                                 tbgpu_query_result* result, NODE node) {
    const bool one = c.world == 1;
    const u32 asked = s.scan ? c.world : 1;  // without a scan nothing is summed: a node's first shard gathers alone
    const int st = query_side_by_side(c.Es, asked, [&](u32 d) -> int { return account_scan_enqueue(c.Es[d], s, NT, d, one, cap); });
    if (st) return query_end(result, st);
    if (one) return account_scan_finish(c.Es[0], s, cap, out, result);
    node();
    return TBGPU_STATUS_OK;
}

// The driver of a call whose rows go by request position: a node's answer is account_scan_node_rows'.
template <typename ROWS>
static int account_scan_run(const QueryCall& c, const AccountScan& s, const NodeTablesArgs& NT, u32 cap, void* out,
                            tbgpu_query_result* result, ROWS rows) {
    return account_scan_run_node(c, s, NT, cap, out, result, [&] { account_scan_node_rows(c, s, cap, (u8*)out, result, rows); });
}

// lookup_accounts_at (k_asof.h).  Its own: T = 0 asks for the records as they are, without a scan; the
// scan is tb_change_effects with claimed bins, and a workgroup keeps the set in LDS as it is up to
// 4,096 ids (at most 8,192 slots) and narrowed to 16-bit entries above (16,384 slots), either way
// beside ASOF_LDS_BINS claimed bins.
static constexpr ScanBinRun ASOF_BIN_LAYOUT[] = {{2, 4}};
extern "C" int tbgpu_lookup_accounts_at(tbgpu_t* E, uint64_t timestamp, const void* ids, uint32_t n, void* out,
                                        uint32_t out_cap_records, tbgpu_query_result* result) {
    static_assert(ASOF_IDS_MAX == TBGPU_LOOKUP_AT_MAX && scan_bin_words(ASOF_BIN_LAYOUT, 1) == BALANCE_SLOT_WORDS,
                  "k_asof.h's constants are the header's");
    static_assert((size_t)CHANGE_SET_SLOTS_MAX * 2 + (size_t)ASOF_LDS_BINS * (BALANCE_SLOT_WORDS * 8 + 4) <= 65536 &&
                      (size_t)CHANGE_LDS_BINS_SLOTS_MAX * 4 + (size_t)ASOF_LDS_BINS * (BALANCE_SLOT_WORDS * 8 + 4) <= 65536,
                  "set, bins and tags stay within 64 KB a workgroup");
    API_ENTER(E, false);
    QueryCall c;
    NodeTablesArgs NT;
    if (const int st = account_scan_begin(E, "lookup_accounts_at", &QueryState::ql, n, TBGPU_LOOKUP_AT_MAX, ids, out, result, &c, &NT,
                                          [&] { return timestamp != ~0ULL; })) {
        return st == SCAN_ANSWERED ? TBGPU_STATUS_OK : st;
    }
    const bool scan = timestamp != 0;
    AccountScan s{};
    s.name = "lookup_accounts_at", s.unit = "records", s.asked = std::to_string(n) + " ids";
    s.bufs = &QueryState::ql, s.bins = [](QueryState& q) { return ScanBins{q.ql.d_bins, q.ql.h_bins}; };
    s.n = n, s.T = timestamp, s.scan = scan;
    s.bin_bytes = ASOF_BIN_BYTES(n), s.flag_word = (u64)n * BALANCE_SLOT_WORDS + CHANGE_FLAG_ORPHAN;
    s.layout = ASOF_BIN_LAYOUT, s.n_runs = 1, s.keys_per_id = 1, s.row_bytes = 128, s.rows_per_id = 1;
    s.launch_scan = [=](const ScanLaunch& L) -> int {
        const bool narrow = L.slots > CHANGE_LDS_BINS_SLOTS_MAX;  // 16-bit entries in LDS: the bins keep their room
        const size_t lds = (size_t)L.slots * (narrow ? 2 : 4) + (size_t)ASOF_LDS_BINS * (BALANCE_SLOT_WORDS * 8 + 4);
        hipLaunchKernelGGL((narrow ? tb_change_effects<u16, true> : tb_change_effects<u32, true>), dim3(L.nb), dim3(CHANGE_THREADS), lds,
                           L.E->stream, L.NT, L.self, L.records, timestamp, (const u32*)L.B.d_set, L.mask, (const u64*)L.B.d_ids, n,
                           L.d_bins, ASOF_LDS_BINS);
        return TBGPU_STATUS_OK;
    };
    s.launch_emit = [=](const ScanLaunch& L) -> int {
        hipLaunchKernelGGL(tb_asof_emit, dim3((n + QUERY_THREADS - 1) / QUERY_THREADS), dim3(QUERY_THREADS), 0, L.E->stream,
                           (const u64*)L.B.d_ids, n, (const u8*)L.B.d_accounts, (const u32*)L.B.d_found,
                           scan ? (const u32*)L.B.d_set : nullptr, L.mask, scan ? (const u64*)L.d_bins : nullptr, L.cap, L.B.d_out,
                           L.B.d_res);
        return TBGPU_STATUS_OK;
    };
    return account_scan_run(c, s, NT, out_cap_records, out, result, [&](const u64* account, const u64* bin, u64 first, u8* rows) -> u32 {
        u8* rec = rows + first * 128;  // the record, its balances less its id's bin
        memcpy(rec, account, 128);
        if (!bin) return 1;
        u128 bal[4];
        memcpy(bal, rec + 16, sizeof bal);
        for (u32 col = 0; col < 4; col++) bal[col] -= tb_u128(bin[2 * col], bin[2 * col + 1]);
        memcpy(rec + 16, bal, sizeof bal);
        return 1;
    });
}

// What the three calls that return 256-B rows from the statements call's buffers have in common.
static AccountScan account_scan_of_rows(const char* name, u32 n, u64 T) {
    AccountScan s{};
    s.name = name, s.unit = "rows", s.asked = std::to_string(n) + " ids";
    s.bufs = &QueryState::qt;
    s.n = n, s.T = T, s.scan = true;
    s.keys_per_id = 1, s.row_bytes = STATEMENT_ROW_BYTES, s.rows_per_id = 1;
    return s;
}

// get_account_statements (k_statement.h): T = t_close.  The scan always runs: t_close = 0 has nothing
// above it, but the period's sums are the log's.  The set has at most 8,192 slots and stays 32-bit in
// LDS beside STATEMENT_LDS_BINS claimed bins.
static constexpr ScanBinRun STATEMENT_BIN_LAYOUT[] = {{2, 4}, {2, 3}, {1, 1}, {2, 3}, {1, 1}};
extern "C" int tbgpu_get_account_statements(tbgpu_t* E, uint64_t t_open, uint64_t t_close, const void* ids, uint32_t n, void* out,
                                            uint32_t out_cap_rows, tbgpu_query_result* result) {
    static_assert(sizeof(tbgpu_account_statement) == STATEMENT_ROW_BYTES && STATEMENT_IDS_MAX == TBGPU_STATEMENTS_MAX &&
                      STATEMENT_ZONE1 + 2 * STATEMENT_SIDE_WORDS == STATEMENT_BIN_WORDS &&
                      scan_bin_words(STATEMENT_BIN_LAYOUT, 5) == STATEMENT_BIN_WORDS,
                  "k_statement.h's constants are the header's");
    static_assert((size_t)CHANGE_LDS_BINS_SLOTS_MAX * 4 + (size_t)STATEMENT_LDS_BINS * (STATEMENT_BIN_WORDS * 8 + 4) <= 65536,
                  "set, bins and tags stay within 64 KB a workgroup");
    API_ENTER(E, false);
    QueryCall c;
    NodeTablesArgs NT;
    if (const int st = account_scan_begin(E, "get_account_statements", &QueryState::qt, n, TBGPU_STATEMENTS_MAX, ids, out, result, &c, &NT,
                                          [&] { return t_open != ~0ULL && t_close != ~0ULL && (t_close == 0 || t_close >= t_open); })) {
        return st == SCAN_ANSWERED ? TBGPU_STATUS_OK : st;
    }
    AccountScan s = account_scan_of_rows("get_account_statements", n, t_close);
    s.bins = [](QueryState& q) { return ScanBins{q.qt.d_bins, q.qt.h_bins}; };
    s.bin_bytes = STATEMENT_BIN_BYTES(n), s.flag_word = (u64)n * STATEMENT_BIN_WORDS;
    s.layout = STATEMENT_BIN_LAYOUT, s.n_runs = 5;
    s.launch_scan = [=](const ScanLaunch& L) -> int {
        const size_t lds = (size_t)L.slots * 4 + (size_t)STATEMENT_LDS_BINS * (STATEMENT_BIN_WORDS * 8 + 4);
        hipLaunchKernelGGL(tb_statement_effects, dim3(L.nb), dim3(CHANGE_THREADS), lds, L.E->stream, L.NT, L.self, L.records, t_open,
                           t_close, (const u32*)L.B.d_set, L.mask, (const u64*)L.B.d_ids, n, L.d_bins);
        return TBGPU_STATUS_OK;
    };
    s.launch_emit = [=](const ScanLaunch& L) -> int {
        hipLaunchKernelGGL(tb_statement_emit, dim3((n + QUERY_THREADS - 1) / QUERY_THREADS), dim3(QUERY_THREADS), 0, L.E->stream,
                           (const u64*)L.B.d_ids, n, (const u8*)L.B.d_accounts, (const u32*)L.B.d_found, (const u32*)L.B.d_set, L.mask,
                           (const u64*)L.d_bins, L.cap, L.B.d_out, L.B.d_res);
        return TBGPU_STATUS_OK;
    };
    return account_scan_run(c, s, NT, out_cap_rows, out, result, [&](const u64* account, const u64* bin, u64 first, u8* rows) -> u32 {
        u64 row[STATEMENT_ROW_BYTES / 8];
        tb_statement_row(account, bin, row);
        memcpy(rows + first * STATEMENT_ROW_BYTES, row, sizeof row);
        return 1;
    });
}

// get_account_balance_integrals (k_integral.h): T = t_end, and bins of its own (IntegralBufs), wider
// and with 192-bit sums.
static constexpr ScanBinRun INTEGRAL_BIN_LAYOUT[] = {{2, 8}, {3, 4}};
extern "C" int tbgpu_get_account_balance_integrals(tbgpu_t* E, uint64_t t_open, uint64_t t_close, const void* ids, uint32_t n, void* out,
                                                   uint32_t out_cap_rows, tbgpu_query_result* result) {
    static_assert(sizeof(tbgpu_account_balance_integral) == INTEGRAL_ROW_BYTES && INTEGRAL_IDS_MAX == TBGPU_INTEGRALS_MAX &&
                      INTEGRAL_WEIGHTED + 4 * 3 == INTEGRAL_BIN_WORDS && INTEGRAL_IDS_MAX == STATEMENT_IDS_MAX &&
                      INTEGRAL_ROW_BYTES == STATEMENT_ROW_BYTES && scan_bin_words(INTEGRAL_BIN_LAYOUT, 2) == INTEGRAL_BIN_WORDS,
                  "k_integral.h's constants are the header's, and the statements call's buffers fit");
    static_assert((size_t)CHANGE_LDS_BINS_SLOTS_MAX * 4 + (size_t)INTEGRAL_LDS_BINS * (INTEGRAL_BIN_WORDS * 8 + 4) <= 65536,
                  "set, bins and tags stay within 64 KB a workgroup");
    API_ENTER(E, false);
    QueryCall c;
    NodeTablesArgs NT;
    if (const int st = account_scan_begin(E, "get_account_balance_integrals", &QueryState::qt, n, TBGPU_INTEGRALS_MAX, ids, out, result, &c,
                                          &NT, [&] { return t_open != ~0ULL && t_close != ~0ULL; })) {
        return st == SCAN_ANSWERED ? TBGPU_STATUS_OK : st;
    }
    // An integral needs a finite end: "now" is commit_timestamp, read once, after the drain.  No account
    // and no record has timestamp 0, so an end at 0 (nothing was ever committed) has no rows.
    const u64 t_end = t_close ? t_close : tbgpu_commit_timestamp(E);
    if (t_end < t_open || t_end == 0) return TBGPU_STATUS_OK;
    AccountScan s = account_scan_of_rows("get_account_balance_integrals", n, t_end);
    s.bins = [](QueryState& q) { return ScanBins{q.qi.d_bins, q.qi.h_bins}; };
    s.bin_bytes = INTEGRAL_BIN_BYTES(n), s.flag_word = (u64)n * INTEGRAL_BIN_WORDS;
    s.layout = INTEGRAL_BIN_LAYOUT, s.n_runs = 2;
    s.launch_scan = [=](const ScanLaunch& L) -> int {
        const size_t lds = (size_t)L.slots * 4 + (size_t)INTEGRAL_LDS_BINS * (INTEGRAL_BIN_WORDS * 8 + 4);
        hipLaunchKernelGGL(tb_integral_effects, dim3(L.nb), dim3(CHANGE_THREADS), lds, L.E->stream, L.NT, L.self, L.records, t_open,
                           t_end, (const u32*)L.B.d_set, L.mask, (const u64*)L.B.d_ids, n, L.d_bins);
        return TBGPU_STATUS_OK;
    };
    s.launch_emit = [=](const ScanLaunch& L) -> int {
        hipLaunchKernelGGL(tb_integral_emit, dim3((n + QUERY_THREADS - 1) / QUERY_THREADS), dim3(QUERY_THREADS), 0, L.E->stream,
                           (const u64*)L.B.d_ids, n, (const u8*)L.B.d_accounts, (const u32*)L.B.d_found, (const u32*)L.B.d_set, L.mask,
                           (const u64*)L.d_bins, t_open, t_end, L.cap, L.B.d_out, L.B.d_res);
        return TBGPU_STATUS_OK;
    };
    return account_scan_run(c, s, NT, out_cap_rows, out, result, [&](const u64* account, const u64* bin, u64 first, u8* rows) -> u32 {
        u64 row[INTEGRAL_ROW_BYTES / 8];
        tb_integral_row(account, bin, t_open, t_end, row);
        memcpy(rows + first * INTEGRAL_ROW_BYTES, row, sizeof row);
        return 1;
    });
}

// get_account_balance_extremes (k_extremes.h).  One engine: T = t_end, the statements call's buffers,
// and in place of bins the zone 0 sums and the element array, which the scan's launch cuts into slabs.
// The exact path below answers a node, an engine whose log turned out not to lie in timestamp order
// (the walk says so), and any engine under TBGPU_EXTREMES_EXACT=1.

// How the walk is cut: `tiles` tiles of CHANGE_THREADS positions into slabs of whole spans of
// CHANGE_TILES tiles, as many as the element array holds for n ids, at most EXTREME_SLABS_MAX and
// `cap` (0: none).  Returns the tiles a slab holds; *slabs: how many there are.
static u32 extreme_slabs(u64 tiles, u32 n, u64 elem_bytes, u32 cap, u32* slabs) {
    u64 most = std::min<u64>(elem_bytes / ((u64)n * EXTREME_ELEM_BYTES), EXTREME_SLABS_MAX);
    if (cap) most = std::min<u64>(most, cap);
    most = std::max<u64>(most, 1);
    const u64 spans = (tiles + CHANGE_TILES - 1) / CHANGE_TILES, spans_per = (spans + most - 1) / most;
    const u64 slab_tiles = std::max<u64>(spans_per, 1) * CHANGE_TILES;
    *slabs = (u32)((tiles + slab_tiles - 1) / slab_tiles);
    return (u32)slab_tiles;
}

// The exact path, from what the other calls answer: which ids yield a row and their closing records
// (lookup_accounts_at at t_end), the opening records (lookup_accounts_at at t_open; an account created
// inside the period has no record there, and none before its own timestamp, so it is asked at that),
// and per found account the balance history of (t_open, t_end] page by page (get_account_balances),
// folded with the walk's own operator.  A log scan or two per account per page.
static int extremes_exact(tbgpu* E, u64 t_open, u64 t_end, u64 measure, const void* ids, u32 n, void* out, u32 cap,
                          tbgpu_query_result* result) {
    std::vector<u8> closing((u64)n * 128), opening((u64)n * 128), page((u64)BATCH_EVENTS_MAX * 128);
    tbgpu_query_result rc{}, ro{}, rp{};
    if (const int st = tbgpu_lookup_accounts_at(E, t_end, ids, n, closing.data(), n, &rc)) return query_end(result, st);
    if (t_open) {  // (0 would ask for the records as they are now; no account was created at or before 0)
        if (const int st = tbgpu_lookup_accounts_at(E, t_open, ids, n, opening.data(), n, &ro)) return query_end(result, st);
    } else {
        ro.complete = 1;
    }
    u32 complete = rc.complete & ro.complete, k = 0, written = 0;
    for (u32 j = 0; j < rc.count; j++) {
        if (j >= cap) break;
        u64 account[16], first[16];
        memcpy(account, closing.data() + (u64)j * 128, 128);
        if (t_open && account[15] <= t_open) {
            if (k >= ro.count) return query_end(result, fail(TBGPU_STATUS_PANIC, "get_account_balance_extremes: an account of t_end is missing at t_open"));
            memcpy(first, opening.data() + (u64)k++ * 128, 128);
        } else {
            tbgpu_query_result r1{};
            if (const int st = tbgpu_lookup_accounts_at(E, account[15], account, 1, first, 1, &r1)) return query_end(result, st);
            if (r1.count != 1) return query_end(result, fail(TBGPU_STATUS_PANIC, "get_account_balance_extremes: an account is missing at its own timestamp"));
            complete &= r1.complete;
        }
        if (first[0] != account[0] || first[1] != account[1]) {
            return query_end(result, fail(TBGPU_STATUS_PANIC, "get_account_balance_extremes: the opening and closing records differ in order"));
        }
        const U192 v0 = tb_extreme_measure_of(measure, first + 2);
        U192 v = v0;
        ExtremeElem e = tb_extreme_empty();
        bool unordered = false;
        tbgpu_account_filter f{};
        f.account_id_lo = account[0], f.account_id_hi = account[1];
        f.timestamp_min = t_open + 1, f.timestamp_max = t_end;
        f.limit = BATCH_EVENTS_MAX, f.flags = TBGPU_FILTER_DEBITS | TBGPU_FILTER_CREDITS;
        while (f.timestamp_min <= t_end) {
            if (const int st = tbgpu_get_account_balances(E, &f, page.data(), BATCH_EVENTS_MAX, &rp)) return query_end(result, st);
            if (rp.count == 0) break;
            complete &= rp.complete;
            for (u32 i = 0; i < rp.count; i++) {
                u64 row[9];
                memcpy(row, page.data() + (u64)i * 128, sizeof row);
                const U192 next = tb_extreme_measure_of(measure, row);
                e = tb_extreme_compose(e, tb_extreme_leaf(tb_sub192(next, v), row[8]), &unordered);
                v = next;
            }
            if (rp.count == rp.matched) break;
            f.timestamp_min = e.last_ts + 1;
        }
        if (unordered) return query_end(result, fail(TBGPU_STATUS_PANIC, "get_account_balance_extremes: a balance history out of timestamp order"));
        u64 row[EXTREME_ROW_BYTES / 8];
        tb_extreme_row(account[0], account[1], v0, e, t_open, t_end, measure, row);
        memcpy((u8*)out + (u64)written++ * EXTREME_ROW_BYTES, row, sizeof row);
    }
    result->count = written;
    result->matched = rc.matched;
    result->complete = complete;
    return TBGPU_STATUS_OK;
}

extern "C" int tbgpu_get_account_balance_extremes(tbgpu_t* E, uint64_t t_open, uint64_t t_close, const tbgpu_balance_measure* measure,
                                                  const void* ids, uint32_t n, void* out, uint32_t out_cap_rows,
                                                  tbgpu_query_result* result) {
    static_assert(sizeof(tbgpu_account_balance_extreme) == EXTREME_ROW_BYTES && sizeof(tbgpu_balance_measure) == 8 &&
                      EXTREME_IDS_MAX == TBGPU_EXTREMES_MAX && EXTREME_IDS_MAX == STATEMENT_IDS_MAX &&
                      EXTREME_ROW_BYTES <= STATEMENT_ROW_BYTES && sizeof(ExtremeElem) == EXTREME_ELEM_BYTES &&
                      EXTREME_ZONE0 == EXTREME_ELEM_WORDS && EXTREME_ZONE0 + 3 == EXTREME_BIN_WORDS,
                  "k_extremes.h's constants are the header's, and the statements call's buffers fit");
    static_assert((size_t)CHANGE_LDS_BINS_SLOTS_MAX * 4 + (size_t)EXTREME_LDS_BINS * (EXTREME_BIN_WORDS * 8 + 4) + 2 * EXTREME_WAVES * 4 <= 65536,
                  "set, bins, tags and hit words stay within 64 KB a workgroup");
    static_assert(EXTREME_ARRAY_BYTES / (EXTREME_IDS_MAX * EXTREME_ELEM_BYTES) >= 256, "a slab per CU at the largest request");
    API_ENTER(E, false);
    if (n > TBGPU_EXTREMES_MAX) return fail(TBGPU_STATUS_INVALID, "get_account_balance_extremes: %u ids (at most %u)", n, TBGPU_EXTREMES_MAX);
    if (n == 0) return TBGPU_STATUS_OK;
    if (!measure || !ids || !out || !result) return fail(TBGPU_STATUS_INVALID, "get_account_balance_extremes: NULL measure, ids, out or result");
    const int8_t coefs[4] = {measure->debits_pending, measure->debits_posted, measure->credits_pending, measure->credits_posted};
    bool some = false;
    for (const int8_t c : coefs) {
        if (c < -1 || c > 1) return fail(TBGPU_STATUS_INVALID, "get_account_balance_extremes: a coefficient of %d (-1, 0 or +1)", (int)c);
        some |= c != 0;
    }
    if (!some) return fail(TBGPU_STATUS_INVALID, "get_account_balance_extremes: a measure of no column");
    for (const uint8_t b : measure->reserved) {
        if (b) return fail(TBGPU_STATUS_INVALID, "get_account_balance_extremes: a non-zero reserved byte in the measure");
    }
    u64 mword;
    memcpy(&mword, measure, 8);
    QueryCall c;
    NodeTablesArgs NT;
    if (const int st = account_scan_begin(E, "get_account_balance_extremes", &QueryState::qt, n, TBGPU_EXTREMES_MAX, ids, out, result, &c,
                                          &NT, [&] { return t_open != ~0ULL && t_close != ~0ULL; })) {
        return st == SCAN_ANSWERED ? TBGPU_STATUS_OK : st;
    }
    const u64 t_end = t_close ? t_close : tbgpu_commit_timestamp(E);  // read once, after the drain
    if (t_end < t_open || t_end == 0) return TBGPU_STATUS_OK;
    if (E->node || E->qs->qe.exact) return extremes_exact(E, t_open, t_end, mword, ids, n, out, out_cap_rows, result);
    AccountScan s = account_scan_of_rows("get_account_balance_extremes", n, t_end);
    s.row_bytes = EXTREME_ROW_BYTES;
    s.bins = [](QueryState& q) { return ScanBins{q.qe.d_zone0, nullptr}; };
    s.bin_bytes = EXTREME_ZONE0_BYTES(n), s.flag_word = (u64)n * 3 + EXTREME_FLAG_ORPHAN;
    u32 slabs = 0;  // what the scan's launch cut the walk into, for the emit; none without a record
    s.launch_scan = [&, n, mword](const ScanLaunch& L) -> int {
        ExtremeBufs& X = L.E->qs->qe;
        const u64 tiles = (L.records + CHANGE_THREADS - 1) / CHANGE_THREADS;
        const u32 slab_tiles = extreme_slabs(tiles, n, X.elem_bytes, X.slabs_cap, &slabs);
        HIPCK(hipMemsetAsync(X.d_elems, 0, (u64)slabs * n * EXTREME_ELEM_BYTES, L.E->stream));
        const size_t lds = (size_t)L.slots * 4 + (size_t)EXTREME_LDS_BINS * (EXTREME_BIN_WORDS * 8 + 4) + 2 * EXTREME_WAVES * 4;
        hipLaunchKernelGGL(tb_extreme_effects, dim3(slabs), dim3(CHANGE_THREADS), lds, L.E->stream, L.NT, L.self, L.records, t_open, t_end,
                           mword, (const u32*)L.B.d_set, L.mask, (const u64*)L.B.d_ids, n, slab_tiles, X.d_elems, L.d_bins);
        return TBGPU_STATUS_OK;
    };
    s.launch_emit = [&, n, mword](const ScanLaunch& L) -> int {
        ExtremeBufs& X = L.E->qs->qe;
        hipLaunchKernelGGL(tb_extreme_emit, dim3((n + QUERY_THREADS - 1) / QUERY_THREADS), dim3(QUERY_THREADS), 0, L.E->stream,
                           (const u64*)L.B.d_ids, n, (const u8*)L.B.d_accounts, (const u32*)L.B.d_found, (const u32*)L.B.d_set, L.mask,
                           (const u64*)X.d_elems, slabs, L.d_bins, t_open, t_end, mword, L.cap, L.B.d_out, L.B.d_res);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpyAsync(X.h_flags, L.d_bins + (u64)n * 3, EXTREME_FLAG_WORDS * 8, hipMemcpyDeviceToHost, L.E->stream));
        return TBGPU_STATUS_OK;
    };
    const int st = account_scan_run_node(c, s, NT, out_cap_rows, out, result, [] {});
    if (st == TBGPU_STATUS_OK && E->qs->qe.h_flags[EXTREME_FLAG_UNORDERED]) {
        return extremes_exact(E, t_open, t_end, mword, ids, n, out, out_cap_rows, result);
    }
    return st;
}

// get_account_statement_series (k_series.h): T = the last bound, B + 1 buckets for the statements
// call's two zones, bins by key and the bounds (SeriesBufs), which go up before the scan.  A node's
// host writes an account's buckets from the last to the first: the closing balances run from the tail
// down, a bucket's opening is the closing of the one before it.
static constexpr ScanBinRun SERIES_BIN_LAYOUT[] = {{2, 3}, {1, 1}, {2, 3}, {1, 1}};
extern "C" int tbgpu_get_account_statement_series(tbgpu_t* E, const uint64_t* bounds, uint32_t n_buckets, const void* ids, uint32_t n,
                                                  void* out, uint32_t out_cap_rows, tbgpu_query_result* result) {
    static_assert(SERIES_ROWS_MAX == TBGPU_SERIES_ROWS_MAX && SERIES_ROWS_MAX == STATEMENT_IDS_MAX &&
                      scan_bin_words(SERIES_BIN_LAYOUT, 4) == SERIES_BIN_WORDS,
                  "k_series.h's constants are the header's, and the statements call's buffers fit");
    // n * n_buckets <= 4,095: above 2,048 ids there is one bucket, and 256 slots hold at most 128 ids.
    static_assert((size_t)CHANGE_LDS_BINS_SLOTS_MAX * 4 + 2 * 8 <= SERIES_LDS_FIXED_MAX &&
                      (size_t)CHANGE_LDS_BINS_SLOTS_MAX / 2 * 4 + 3 * 8 <= SERIES_LDS_FIXED_MAX &&
                      (size_t)SERIES_LDS_FIXED_MAX + (size_t)SERIES_LDS_BINS * (SERIES_BIN_WORDS * 8 + 4) <= 65536,
                  "bounds, set, bins and tags stay within 64 KB a workgroup");
    API_ENTER(E, false);
    if (n_buckets == 0) return fail(TBGPU_STATUS_INVALID, "get_account_statement_series: no buckets");
    if ((u64)n * n_buckets > TBGPU_SERIES_ROWS_MAX) {
        return fail(TBGPU_STATUS_INVALID, "get_account_statement_series: %u ids x %u buckets (at most %u rows)", n, n_buckets,
                    TBGPU_SERIES_ROWS_MAX);
    }
    if (!bounds) return fail(TBGPU_STATUS_INVALID, "get_account_statement_series: NULL bounds");
    QueryCall c;
    NodeTablesArgs NT;
    if (const int st = account_scan_begin(E, "get_account_statement_series", &QueryState::qt, n, ~0u, ids, out, result, &c, &NT, [&] {
            for (u32 k = 0; k <= n_buckets; k++) {
                if (bounds[k] == ~0ULL) return false;
                if (k == 0) continue;
                const bool open_end = k == n_buckets && bounds[k] == 0;
                if (!open_end && (bounds[k] == 0 || bounds[k] < bounds[k - 1])) return false;
            }
            return true;
        })) {
        return st == SCAN_ANSWERED ? TBGPU_STATUS_OK : st;
    }
    for (u32 d = 0; d < c.world; d++) memcpy(c.Es[d]->qs->qr.h_bounds, bounds, ((u64)n_buckets + 1) * 8);
    const u32 stride = n_buckets + 1;
    AccountScan s = account_scan_of_rows("get_account_statement_series", n, bounds[n_buckets]);
    s.asked += " x " + std::to_string(n_buckets) + " buckets";
    s.bins = [](QueryState& q) { return ScanBins{q.qr.d_bins, q.qr.h_bins}; };
    s.bin_bytes = SERIES_BIN_BYTES((u64)n * stride), s.flag_word = (u64)n * stride * SERIES_BIN_WORDS;
    s.layout = SERIES_BIN_LAYOUT, s.n_runs = 4, s.keys_per_id = stride, s.rows_per_id = n_buckets;
    s.launch_scan = [=](const ScanLaunch& L) -> int {
        const SeriesBufs& R = L.E->qs->qr;
        const size_t lds = tb_series_lds_bytes(L.slots, n_buckets);
        if (lds > 65536) return fail(TBGPU_STATUS_PANIC, "get_account_statement_series: %zu bytes of LDS", lds);
        HIPCK(hipMemcpyAsync(R.d_bounds, R.h_bounds, ((u64)n_buckets + 1) * 8, hipMemcpyHostToDevice, L.E->stream));
        hipLaunchKernelGGL(tb_series_effects, dim3(L.nb), dim3(CHANGE_THREADS), lds, L.E->stream, L.NT, L.self, L.records,
                           (const u64*)R.d_bounds, n_buckets, (const u32*)L.B.d_set, L.mask, (const u64*)L.B.d_ids, n, L.d_bins);
        return TBGPU_STATUS_OK;
    };
    s.launch_emit = [=](const ScanLaunch& L) -> int {
        hipLaunchKernelGGL(tb_series_emit, dim3((n * n_buckets + QUERY_THREADS - 1) / QUERY_THREADS), dim3(QUERY_THREADS), 0, L.E->stream,
                           (const u64*)L.B.d_ids, n, n_buckets, (const u8*)L.B.d_accounts, (const u32*)L.B.d_found,
                           (const u32*)L.B.d_set, L.mask, (const u64*)L.d_bins, L.cap, L.B.d_out, L.B.d_res);
        return TBGPU_STATUS_OK;
    };
    return account_scan_run(c, s, NT, out_cap_rows, out, result, [&](const u64* account, const u64* bins, u64 first, u8* rows) -> u32 {
        u128 closing[4], net[4];
        tb_series_net(bins + (u64)n_buckets * SERIES_BIN_WORDS, net);  // the tail
        for (u32 col = 0; col < 4; col++) closing[col] = tb_u128(account[2 + 2 * col], account[3 + 2 * col]) - net[col];
        u32 written = 0;
        for (u32 k = n_buckets; k-- > 0;) {
            u64 row[STATEMENT_ROW_BYTES / 8];
            tb_flows_row(account, bins + (u64)k * SERIES_BIN_WORDS, closing, row);
            if (first + k < out_cap_rows) {
                memcpy(rows + (first + k) * STATEMENT_ROW_BYTES, row, sizeof row);
                written++;
            }
            for (u32 col = 0; col < 4; col++) closing[col] = tb_u128(row[2 + 2 * col], row[3 + 2 * col]);  // its opening
        }
        return written;
    });
}

// get_account_flow_matrix (k_matrix.h): the request is the two lists laid end to end, T = t_close, the
// key is the pair.  The host builds the maps from the ids and sends them up before the scan.  Rows
// are a product of two found lists, so a node's answer has a loop of its own: for every found pair
// under the cap, the sum of every shard's bin of key (row_of, col_of), written by the device's cell
// function.
static constexpr ScanBinRun MATRIX_BIN_LAYOUT[] = {{2, 3}, {1, 1}};
static void matrix_node_cells(const QueryCall& c, const AccountScan& s, u32 n_debit, u32 n_credit, const std::vector<u32>& first,
                              u32 cap, u8* out, tbgpu_query_result* result) {
    const AccountScanBufs& B = c.Es[0]->qs->*s.bufs;
    const u16 *row_of = c.Es[0]->qs->qxm.h_maps, *col_of = row_of + s.n;
    u64 found_debit = 0, found_credit = 0;
    for (u32 i = 0; i < n_debit; i++) found_debit += B.h_found[i] != 0;
    for (u32 i = n_debit; i < s.n; i++) found_credit += B.h_found[i] != 0;
    const u64 matched = found_debit * found_credit;
    u64 at = 0;
    for (u32 i = 0; i < n_debit && at < cap; i++) {
        if (!B.h_found[i]) continue;
        for (u32 j = n_debit; j < s.n && at < cap; j++) {
            if (!B.h_found[j]) continue;
            const u64 key = (u64)row_of[first[i]] * n_credit + col_of[first[j]];
            u64 sum[MATRIX_BIN_WORDS] = {}, cell[MATRIX_CELL_BYTES / 8];
            for (u32 d = 0; d < c.world; d++) scan_bins_add(sum, s.bins(*c.Es[d]->qs).h + key * MATRIX_BIN_WORDS, s.layout, s.n_runs, 1);
            tb_matrix_cell(B.h_ids + 2 * (u64)i, B.h_ids + 2 * (u64)j, sum, cell);
            memcpy(out + at * MATRIX_CELL_BYTES, cell, sizeof cell);
            at++;
        }
    }
    for (u32 d = 0; d < c.world; d++) {
        if (s.bins(*c.Es[d]->qs).h[s.flag_word]) result->complete = 0;
    }
    result->count = (u32)at;
    result->matched = matched;
}

extern "C" int tbgpu_get_account_flow_matrix(tbgpu_t* E, uint64_t t_open, uint64_t t_close, const void* debit_ids, uint32_t n_debit,
                                             const void* credit_ids, uint32_t n_credit, void* out, uint32_t out_cap_cells,
                                             tbgpu_query_result* result) {
    static_assert(sizeof(tbgpu_flow_cell) == MATRIX_CELL_BYTES && MATRIX_CELLS_MAX == TBGPU_FLOW_MATRIX_CELLS_MAX &&
                      MATRIX_IDS_MAX == MATRIX_CELLS_MAX + 1 && MATRIX_NONE == SCAN_PAIR_NONE && MATRIX_IDS_MAX <= MATRIX_NONE &&
                      MATRIX_IDS_MAX == MATRIX_EMIT_CHUNK * QUERY_THREADS && scan_bin_words(MATRIX_BIN_LAYOUT, 2) == MATRIX_BIN_WORDS &&
                      (MATRIX_BIN_WORDS + 5) * 8 == MATRIX_CELL_BYTES,
                  "k_matrix.h's constants are the header's and account_scan_host.h's");
    // 4,096 positions: 8,192 slots of 32 bits, as CHANGE_LDS_BINS_SLOTS_MAX, and an index + 1 fits an entry's 16 bits.
    static_assert((size_t)CHANGE_LDS_BINS_SLOTS_MAX * 4 + (size_t)MATRIX_IDS_MAX * 4 + (size_t)MATRIX_LDS_BINS * (MATRIX_BIN_WORDS * 8 + 4) <=
                      65536,
                  "set, maps, bins and tags stay within 64 KB a workgroup");
    API_ENTER(E, false);
    if (n_debit == 0 || n_credit == 0) return TBGPU_STATUS_OK;
    if ((u64)n_debit * n_credit > TBGPU_FLOW_MATRIX_CELLS_MAX) {
        return fail(TBGPU_STATUS_INVALID, "get_account_flow_matrix: %u x %u ids (at most %u cells)", n_debit, n_credit,
                    TBGPU_FLOW_MATRIX_CELLS_MAX);
    }
    if (!credit_ids) return fail(TBGPU_STATUS_INVALID, "get_account_flow_matrix: NULL ids, out or result");
    const u32 n = n_debit + n_credit;  // at most MATRIX_IDS_MAX: the product is at most 4,095
    QueryCall c;
    NodeTablesArgs NT;
    if (const int st = account_scan_begin(E, "get_account_flow_matrix", &QueryState::qx, n_debit, MATRIX_IDS_MAX, debit_ids, out, result, &c,
                                          &NT, [&] { return t_open != ~0ULL && t_close != ~0ULL && (t_close == 0 || t_close >= t_open); })) {
        return st == SCAN_ANSWERED ? TBGPU_STATUS_OK : st;
    }
    // The debit ids are in every shard's pinned buffer; the credit ids go behind them, and the maps beside.
    const std::vector<u32> first = [&] {
        u64* h_ids = c.Es[0]->qs->qx.h_ids;
        memcpy(h_ids + 2 * (u64)n_debit, credit_ids, (u64)n_credit * 16);
        return scan_first_positions(h_ids, n);
    }();
    scan_pair_maps(first, n_debit, n_credit, c.Es[0]->qs->qxm.h_maps, c.Es[0]->qs->qxm.h_maps + n);
    for (u32 d = 1; d < c.world; d++) {
        memcpy(c.Es[d]->qs->qx.h_ids + 2 * (u64)n_debit, credit_ids, (u64)n_credit * 16);
        memcpy(c.Es[d]->qs->qxm.h_maps, c.Es[0]->qs->qxm.h_maps, (u64)n * 4);
    }
    const u32 n_keys = n_debit * n_credit;
    AccountScan s{};
    s.name = "get_account_flow_matrix", s.unit = "cells", s.asked = std::to_string(n_debit) + " x " + std::to_string(n_credit) + " ids";
    s.bufs = &QueryState::qx, s.bins = [](QueryState& q) { return ScanBins{q.qx.d_bins, q.qx.h_bins}; };
    s.n = n, s.T = t_close, s.scan = true;
    s.bin_bytes = MATRIX_BIN_BYTES(n_keys), s.flag_word = (u64)n_keys * MATRIX_BIN_WORDS;
    s.layout = MATRIX_BIN_LAYOUT, s.n_runs = 2, s.keys_per_id = 1, s.row_bytes = MATRIX_CELL_BYTES;
    s.rows_per_id = std::max(n_debit, n_credit);  // matched = found_debit * found_credit <= n * the longer list
    const auto maps_up = [=](const ScanLaunch& L) -> int {
        const MatrixBufs& X = L.E->qs->qxm;
        HIPCK(hipMemcpyAsync(X.d_maps, X.h_maps, (u64)n * 4, hipMemcpyHostToDevice, L.E->stream));
        return TBGPU_STATUS_OK;
    };
    s.launch_scan = [=](const ScanLaunch& L) -> int {
        if (const int st = maps_up(L)) return st;
        hipLaunchKernelGGL(tb_matrix_effects, dim3(L.nb), dim3(CHANGE_THREADS), tb_matrix_lds_bytes(L.slots, n), L.E->stream, L.NT, L.self,
                           L.records, t_open, t_close, (const u32*)L.B.d_set, L.mask, (const u64*)L.B.d_ids, n,
                           (const u16*)L.E->qs->qxm.d_maps, n_credit, n_keys, L.d_bins);
        return TBGPU_STATUS_OK;
    };
    s.launch_emit = [=](const ScanLaunch& L) -> int {
        if (L.nb == 0) {  // an empty log: no scan took the maps up
            if (const int st = maps_up(L)) return st;
        }
        hipLaunchKernelGGL(tb_matrix_emit, dim3((n_keys + QUERY_THREADS - 1) / QUERY_THREADS), dim3(QUERY_THREADS), 0, L.E->stream,
                           (const u64*)L.B.d_ids, n_debit, n_credit, (const u32*)L.B.d_found, (const u32*)L.B.d_set, L.mask,
                           (const u16*)L.E->qs->qxm.d_maps, (const u64*)L.d_bins, L.cap, L.B.d_out, L.B.d_res);
        return TBGPU_STATUS_OK;
    };
    return account_scan_run_node(c, s, NT, out_cap_cells, out, result,
                                 [&] { matrix_node_cells(c, s, n_debit, n_credit, first, out_cap_cells, (u8*)out, result); });
}

// ---- get_account_counterparties (k_counterparties.h, include/tbgpu.h) ------------------------------
// The groups are discovered on the device, so the call has a driver of its own: every engine zeroes
// its group table and scans its own log, side by side; a node's first shard then folds its peers'
// tables into its own, one merge kernel a peer, once every stream is idle; the select's passes, the
// collect and the emit follow back to back on the first engine's stream, and only the state words and
// the answer's rows cross PCIe.  One engine enqueues all of it at once.
static bool counterparty_filter_valid(const tbgpu_counterparty_filter* f) {
    if (tb_id_reserved(f->account_id_lo, f->account_id_hi)) return false;
    if ((f->flags & (TBGPU_FILTER_DEBITS | TBGPU_FILTER_CREDITS)) == 0) return false;
    if (f->flags & ~(u32)(TBGPU_FILTER_DEBITS | TBGPU_FILTER_CREDITS | TBGPU_COUNTERPARTIES_BY_VOLUME)) return false;
    for (u32 i = 0; i < sizeof f->reserved; i++) {
        if (f->reserved[i]) return false;
    }
    if (f->t_open == ~0ULL || f->t_close == ~0ULL || (f->t_close != 0 && f->t_close < f->t_open)) return false;
    return f->limit != 0;
}

// launch(nb, records, K): the member's scan kernel over E's log, on E's stream.
template <typename LAUNCH>
static int counterparty_enqueue_scan(tbgpu* E, bool mirror, LAUNCH launch) {
    CounterpartyBufs& K = E->qs->qk;
    HIPCK(hipSetDevice(E->device));
    HIPCK(hipMemsetAsync(K.d_table, 0, K.slots * CP_SLOT_WORDS * 8, E->stream));
    HIPCK(hipMemsetAsync(K.d_state, 0, CP_STATE_BYTES, E->stream));
    const u64 records = E->log_next, per = (u64)CHANGE_THREADS * CHANGE_TILES, nb = (records + per - 1) / per;
    if (nb) {
        launch((unsigned)nb, records, K);
        HIPCK(hipGetLastError());
    }
    if (mirror) HIPCK(hipMemcpyAsync(K.h_state, K.d_state, (u64)CP_WORDS * 8, hipMemcpyDeviceToHost, E->stream));
    return TBGPU_STATUS_OK;
}

// On the first engine's stream: the peers' tables folded in (a node), then count -> begin -> the
// select's passes -> collect -> emit, and the state words on their way back.  order: a CP_ORDER_*.
static int counterparty_enqueue_select(const QueryCall& c, const NodeTablesArgs& NT, u32 order) {
    tbgpu* E = c.Es[0];
    CounterpartyBufs& K = E->qs->qk;
    HIPCK(hipSetDevice(E->device));
    const u32 mask = (u32)(K.slots - 1), k = c.k;
    const unsigned nb = (unsigned)((K.slots + QUERY_THREADS - 1) / QUERY_THREADS);
    for (u32 d = 1; d < c.world; d++) {
        hipLaunchKernelGGL(tb_cp_merge, dim3(nb), dim3(QUERY_THREADS), 0, E->stream, NT, (const u64*)c.Es[d]->qs->qk.d_table, K.d_table,
                           mask, K.d_state);
    }
    hipLaunchKernelGGL(tb_cp_count, dim3(nb), dim3(QUERY_THREADS), 0, E->stream, NT, (const u64*)K.d_table, mask, order, K.d_counts,
                       K.d_state);
    if (k) {
        hipLaunchKernelGGL(tb_cp_begin, dim3(1), dim3(64), 0, E->stream, k, K.d_state);
        select_enqueue(E->stream, CpSource{NT, K.d_table, mask, order}, nb, k, tb_cp_order_words(order) * SEL_WORD_PASSES, K.d_state,
                       (u32*)(K.d_state + CP_WORDS), K.d_counts, K.d_keys);
        hipLaunchKernelGGL(tb_cp_emit, dim3((k + SEL_EMIT_KEYS - 1) / SEL_EMIT_KEYS), dim3(QUERY_THREADS), 0, E->stream, NT,
                           (const u64*)K.d_table, mask, k, (const u64*)K.d_state, (const u64*)K.d_keys, K.d_out);
    }
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpyAsync(K.h_state, K.d_state, (u64)CP_WORDS * 8, hipMemcpyDeviceToHost, E->stream));
    return TBGPU_STATUS_OK;
}

// The driver after query_begin and the filter's checks, shared with get_active_accounts: every engine
// drained, the scans side by side (launch(d, nb, records, K): shard d's scan kernel), the select, the
// flags, the rows.  `name` is the call's, `what` what its groups are, for the capacity message.
template <typename LAUNCH>
static int counterparty_answer(QueryCall& c, NodeTablesArgs& NT, u32 order, const char* name, const char* what, void* out,
                               tbgpu_query_result* result, LAUNCH launch) {
    NT.world = c.world;
    for (u32 d = 0; d < c.world; d++) NT.T[d] = c.Es[d]->T;
    // Every engine is drained before any is asked: a scan reads its posts' pending transfers on their homes.
    for (u32 d = 0; d < c.world; d++) {
        HIPCK(hipSetDevice(c.Es[d]->device));
        if (c.Es[d]->pending) {
            const int st = engine_sync(c.Es[d]);
            if (st) return query_end(result, st);
        }
    }
    const bool one = c.world == 1;
    int st = query_side_by_side(c.Es, c.world, [&](u32 d) -> int {
        const int s = counterparty_enqueue_scan(c.Es[d], !one, [&](unsigned nb, u64 records, CounterpartyBufs& K) { launch(d, nb, records, K); });
        if (s) return s;
        return one ? counterparty_enqueue_select(c, NT, order) : TBGPU_STATUS_OK;
    });
    if (st) return query_end(result, st);
    u64 orphan = 0, overflow = 0;
    if (!one) {  // the peers' flags are back; the first shard's follow with the select's words
        for (u32 d = 1; d < c.world; d++) orphan |= c.Es[d]->qs->qk.h_state[CP_ORPHAN], overflow |= c.Es[d]->qs->qk.h_state[CP_OVERFLOW];
        st = counterparty_enqueue_select(c, NT, order);
        if (st == TBGPU_STATUS_OK) st = query_wait(c.Es[0]);
        if (st) return query_end(result, st);
    }
    tbgpu* E0 = c.Es[0];
    const CounterpartyBufs& K = E0->qs->qk;
    orphan |= K.h_state[CP_ORPHAN], overflow |= K.h_state[CP_OVERFLOW];
    if (overflow) {
        return query_end(result, fail(TBGPU_STATUS_INVALID,
                                      "%s: the matching records name more distinct %s than the "
                                      "group table holds (capacity: %llu groups, %llu slots)",
                                      name, what, (unsigned long long)K.groups, (unsigned long long)K.slots));
    }
    const u64 matched = K.h_state[SEL_TOTAL];
    const u32 m = (u32)std::min<u64>(c.k, matched);
    if (m) {
        if (const int s = select_check(name, "groups", K.h_state, c.k, m)) return query_end(result, s);
        HIPCK(hipSetDevice(E0->device));
        HIPCK(hipMemcpyAsync(out, K.d_out, (u64)m * CP_ROW_BYTES, hipMemcpyDeviceToHost, E0->stream));
        HIPCK(hipStreamSynchronize(E0->stream));
    }
    if (orphan) result->complete = 0;
    result->count = m;
    result->matched = matched;
    return TBGPU_STATUS_OK;
}

extern "C" int tbgpu_get_account_counterparties(tbgpu_t* E, const tbgpu_counterparty_filter* filter, void* out, uint32_t out_cap_rows,
                                                tbgpu_query_result* result) {
    static_assert(sizeof(tbgpu_counterparty_filter) == 64 && sizeof(tbgpu_counterparty_flow) == CP_FLOW_WORDS * 8 &&
                      sizeof(tbgpu_counterparty) == CP_ROW_BYTES && CP_ROWS_MAX == TBGPU_COUNTERPARTIES_ROWS_MAX &&
                      CP_FLOW_WORDS == MATRIX_BIN_WORDS && CP_TO + 2 * CP_FLOW_WORDS == CP_SLOT_WORDS &&
                      CP_SIDE_DEBITS == TBGPU_FILTER_DEBITS && CP_SIDE_CREDITS == TBGPU_FILTER_CREDITS && NODE_WORLD_MAX <= (1u << 22),
                  "k_counterparties.h's constants are the header's");
    QueryCall c;
    if (const int st = query_begin(E, "get_account_counterparties", filter, out, out_cap_rows, TBGPU_COUNTERPARTIES_ROWS_MAX, true, result,
                                   &c)) {
        return st;
    }
    if (!counterparty_filter_valid(filter)) return TBGPU_STATUS_OK;
    CpFilter F{};
    F.a_lo = filter->account_id_lo, F.a_hi = filter->account_id_hi;
    F.t_open = filter->t_open, F.t_close = filter->t_close;
    F.min_lo = filter->id_min_lo, F.min_hi = filter->id_min_hi;
    F.sides = filter->flags & (TBGPU_FILTER_DEBITS | TBGPU_FILTER_CREDITS);
    F.by_volume = (filter->flags & TBGPU_COUNTERPARTIES_BY_VOLUME) != 0;
    NodeTablesArgs NT{};
    return counterparty_answer(c, NT, F.by_volume ? CP_ORDER_VOLUME : CP_ORDER_ID, "get_account_counterparties", "counterparties", out, result,
                               [&](u32 d, unsigned nb, u64 records, CounterpartyBufs& K) {
                                   hipLaunchKernelGGL(tb_cp_scan, dim3(nb), dim3(CHANGE_THREADS), 0, c.Es[d]->stream, NT, d, records, F,
                                                      K.d_table, (u32)(K.slots - 1), K.d_state);
                               });
}

// ---- get_active_accounts (k_activity.h, include/tbgpu.h) -------------------------------------------
// get_account_counterparties' driver, buffers and select with another scan: nobody is the subject.
static bool activity_filter_valid(const tbgpu_activity_filter* f) {
    if ((f->flags & (TBGPU_FILTER_DEBITS | TBGPU_FILTER_CREDITS)) == 0) return false;
    if (f->flags & ~(u32)(TBGPU_FILTER_DEBITS | TBGPU_FILTER_CREDITS | TBGPU_ACTIVE_BY_VOLUME | TBGPU_ACTIVE_BY_TRANSFERS)) return false;
    if ((f->flags & TBGPU_ACTIVE_BY_VOLUME) && (f->flags & TBGPU_ACTIVE_BY_TRANSFERS)) return false;
    for (u32 i = 0; i < sizeof f->reserved0; i++) {
        if (f->reserved0[i]) return false;
    }
    for (u32 i = 0; i < sizeof f->reserved; i++) {
        if (f->reserved[i]) return false;
    }
    if (f->t_open == ~0ULL || f->t_close == ~0ULL || (f->t_close != 0 && f->t_close < f->t_open)) return false;
    return f->limit != 0;
}

extern "C" int tbgpu_get_active_accounts(tbgpu_t* E, const tbgpu_activity_filter* filter, void* out, uint32_t out_cap_rows,
                                         tbgpu_query_result* result) {
    static_assert(sizeof(tbgpu_activity_filter) == 64 && sizeof(tbgpu_account_activity) == ACT_ROW_BYTES &&
                      offsetof(tbgpu_account_activity, debits) == CP_TO * 8 &&
                      offsetof(tbgpu_account_activity, credits) == (CP_TO + CP_FLOW_WORDS) * 8 && ACT_ROWS_MAX == TBGPU_ACTIVE_ROWS_MAX &&
                      ACT_ROWS_MAX <= CP_ROWS_MAX && offsetof(tbgpu_activity_filter, ledger) == 32 &&
                      offsetof(tbgpu_activity_filter, limit) == 40,
                  "k_activity.h's constants are the header's");
    QueryCall c;
    if (const int st = query_begin(E, "get_active_accounts", filter, out, out_cap_rows, TBGPU_ACTIVE_ROWS_MAX, true, result, &c)) return st;
    if (!activity_filter_valid(filter)) return TBGPU_STATUS_OK;
    ActFilter F{};
    F.t_open = filter->t_open, F.t_close = filter->t_close;
    F.min_lo = filter->id_min_lo, F.min_hi = filter->id_min_hi;
    tb_activity_w14(filter->ledger, filter->code, F.w14_mask, F.w14);
    F.sides = filter->flags & (TBGPU_FILTER_DEBITS | TBGPU_FILTER_CREDITS);
    const u32 order = (filter->flags & TBGPU_ACTIVE_BY_VOLUME) ? CP_ORDER_VOLUME : (filter->flags & TBGPU_ACTIVE_BY_TRANSFERS) ? CP_ORDER_TRANSFERS : CP_ORDER_ID;
    NodeTablesArgs NT{};
    return counterparty_answer(c, NT, order, "get_active_accounts", "accounts", out, result,
                               [&](u32 d, unsigned nb, u64 records, CounterpartyBufs& K) {
                                   hipLaunchKernelGGL(tb_activity_scan, dim3(nb), dim3(CHANGE_THREADS), 0, c.Es[d]->stream, NT, d, records,
                                                      F, K.d_table, (u32)(K.slots - 1), K.d_state);
                               });
}

// ---- get_ledger_balances (k_ledgers.h, include/tbgpu.h) -------------------------------------------
// The host builds the set of the request's distinct non-zero ledgers in the first engine's pinned
// buffer; every engine takes it up, zeroes its bins and runs the table scan and, for T != 0, the log
// scan on its own stream, side by side; the bins come back pinned, the host adds the engines' and
// writes the rows.  A ledger's bin is its slot in the set; bin `slots` is every ledger together.
static int ledgers_enqueue(tbgpu* E, const NodeTablesArgs& NT, u32 self, u32 slots, u64 T, u32 all) {
    LedgerBufs& G = E->qs->qg;
    HIPCK(hipSetDevice(E->device));
    const u32 mask = slots - 1;
    const u64 bin_bytes = LEDGER_BINS(slots) * LEDGER_BIN_WORDS * 8;
    HIPCK(hipMemcpyAsync(G.d_set, G.h_set, (u64)slots * 4, hipMemcpyHostToDevice, E->stream));
    HIPCK(hipMemsetAsync(G.d_bins, 0, bin_bytes, E->stream));
    const u64 per_table = (u64)LEDGER_THREADS * LEDGER_TABLE_TILES, nb_table = (E->account_cap + per_table - 1) / per_table;
    hipLaunchKernelGGL(tb_ledger_accounts, dim3((unsigned)nb_table), dim3(LEDGER_THREADS), tb_ledger_lds_bytes(slots, LEDGER_TABLE_WORDS),
                       E->stream, E->T, E->account_cap, NT.world, self, T, (const u32*)G.d_set, mask, all, G.d_bins);
    HIPCK(hipGetLastError());
    const u64 records = E->log_next, per_log = (u64)LEDGER_THREADS * LEDGER_LOG_TILES, nb_log = (records + per_log - 1) / per_log;
    if (T != 0 && nb_log) {
        hipLaunchKernelGGL(tb_ledger_effects, dim3((unsigned)nb_log), dim3(LEDGER_THREADS), tb_ledger_lds_bytes(slots, LEDGER_LOG_WORDS),
                           E->stream, NT, self, records, T, (const u32*)G.d_set, mask, all, G.d_bins);
        HIPCK(hipGetLastError());
    }
    HIPCK(hipMemcpyAsync(G.h_bins, G.d_bins, bin_bytes, hipMemcpyDeviceToHost, E->stream));
    return TBGPU_STATUS_OK;
}

// The rows from the engines' pinned bins: request position i's row is its ledger's bin (ledger 0: bin
// `slots`) summed over the engines, the accounts' sums less the newer records' effects on either side.
static void ledgers_rows(const QueryCall& c, const u32* ledgers, u32 n, u32 slots, u32 cap, u8* out, tbgpu_query_result* result) {
    const u32* set = c.Es[0]->qs->qg.h_set;
    const u32 rows = std::min(n, cap);
    for (u32 i = 0; i < rows; i++) {
        const u32 bin = ledgers[i] ? tb_ledger_probe(set, slots - 1, ledgers[i]) : slots;
        u128 sums[4] = {0, 0, 0, 0}, effects[2] = {0, 0};
        u64 accounts = 0;
        for (u32 d = 0; d < c.world; d++) {
            const u64* b = c.Es[d]->qs->qg.h_bins + (u64)bin * LEDGER_BIN_WORDS;
            for (u32 col = 0; col < 4; col++) sums[col] += tb_u128(b[2 * col], b[2 * col + 1]);
            for (u32 e = 0; e < 2; e++) effects[e] += tb_u128(b[LEDGER_BIN_EFFECTS + 2 * e], b[LEDGER_BIN_EFFECTS + 2 * e + 1]);
            accounts += b[LEDGER_BIN_COUNT];
        }
        tbgpu_ledger_balance row{};
        u64* w = &row.debits_pending_lo;
        for (u32 col = 0; col < 4; col++) {
            const u128 v = sums[col] - effects[col & 1];
            w[2 * col] = tb_lo(v), w[2 * col + 1] = tb_hi(v);
        }
        row.accounts = accounts;
        row.ledger = ledgers[i];
        memcpy(out + (u64)i * sizeof row, &row, sizeof row);
    }
    for (u32 d = 0; d < c.world; d++) {
        if (c.Es[d]->qs->qg.h_bins[((u64)slots + 1) * LEDGER_BIN_WORDS + CHANGE_FLAG_ORPHAN]) result->complete = 0;
    }
    result->count = rows;
    result->matched = n;
}

extern "C" int tbgpu_get_ledger_balances(tbgpu_t* E, uint64_t timestamp, const uint32_t* ledgers, uint32_t n, void* out,
                                         uint32_t out_cap_rows, tbgpu_query_result* result) {
    static_assert(sizeof(tbgpu_ledger_balance) == 128, "a row is 128 bytes");
    API_ENTER(E, false);
    if (n > TBGPU_LEDGERS_MAX) return fail(TBGPU_STATUS_INVALID, "get_ledger_balances: %u ledgers (at most %u)", n, TBGPU_LEDGERS_MAX);
    if (n == 0) return TBGPU_STATUS_OK;
    if (!ledgers || !out || !result) return fail(TBGPU_STATUS_INVALID, "get_ledger_balances: NULL ledgers, out or result");
    QueryCall c;
    result->count = 0;
    result->matched = 0;
    result->complete = query_engines(E, true, &c);
    if (timestamp == ~0ULL) return TBGPU_STATUS_OK;
    NodeTablesArgs NT{};
    NT.world = c.world;
    for (u32 d = 0; d < c.world; d++) NT.T[d] = c.Es[d]->T;
    // Every engine is drained before any is asked: a scan reads its posts' pending transfers on their homes.
    for (u32 d = 0; d < c.world; d++) {
        HIPCK(hipSetDevice(c.Es[d]->device));
        if (c.Es[d]->pending) {
            const int st = engine_sync(c.Es[d]);
            if (st) return query_end(result, st);
        }
    }
    u32* set = c.Es[0]->qs->qg.h_set;
    u32 all = 0;
    const u32 slots = tb_ledger_set_slots(n);  // (sized by the positions: at most half full whatever repeats)
    memset(set, 0, (u64)slots * 4);
    for (u32 i = 0; i < n; i++) {
        if (ledgers[i]) tb_ledger_insert(set, slots - 1, ledgers[i]);
        else all = 1;
    }
    const int st = query_side_by_side(c.Es, c.world, [&](u32 d) -> int {
        if (d) memcpy(c.Es[d]->qs->qg.h_set, set, (u64)slots * 4);
        return ledgers_enqueue(c.Es[d], NT, d, slots, timestamp, all);
    });
    if (st) return query_end(result, st);
    ledgers_rows(c, ledgers, n, slots, out_cap_rows, (u8*)out, result);
    return TBGPU_STATUS_OK;
}

// ---- get_pending_transfers (k_pending.h, include/tbgpu.h) -----------------------------------------
// The selection is the log scan under QueryPendingFilter: every listed engine's kept records land in
// its own pinned h_rows and their states, written on the device beside them, in its h_states; the
// host places one engine's, or a node's merged by timestamp, into the caller's rows.  Then, only when
// a placed row is posted or voided, the join: the set of those rows' ids, built in the first engine's
// pinned buffer (change_set_insert; a node copies it into every shard's), every engine's
// tb_pending_resolutions over its own log on its own stream, side by side, and the slots into the rows.
static bool pending_filter_valid(const tbgpu_pending_filter* f) {
    const u32 sides = TBGPU_FILTER_DEBITS | TBGPU_FILTER_CREDITS;
    if ((f->account_id_lo & f->account_id_hi) == ~0ULL) return false;
    if ((f->account_id_lo | f->account_id_hi) != 0 && !(f->flags & sides)) return false;
    if (!(f->flags & PENDING_STATES)) return false;
    if (f->flags & ~(sides | TBGPU_FILTER_REVERSED | PENDING_STATES)) return false;
    if (f->timestamp_min == ~0ULL || f->timestamp_max == ~0ULL || f->now == ~0ULL) return false;
    if (f->timestamp_max != 0 && f->timestamp_max < f->timestamp_min) return false;
    if (f->limit == 0) return false;
    for (u8 b : f->reserved) if (b) return false;
    return true;
}

// The first k of the engines' kept records by timestamp (the last k, newest first, under `reversed`)
// into the rows' pending halves, their states beside them: query_merge with the state carried along.
static u32 pending_place_rows(const QueryCall& c, const u32* cnt, bool reversed, u8* rows, u8* states) {
    u32 at[NODE_WORLD_MAX] = {};
    u32 w = 0;
    for (; w < c.k; w++) {
        u32 pick = c.world;
        u64 best = 0;
        for (u32 d = 0; d < c.world; d++) {
            if (at[d] == cnt[d]) continue;
            const u64 ts = change_row_word(c.Es[d]->qs->qp.h_rows + (u64)at[d] * 128, 15);
            if (pick == c.world || (reversed ? ts > best : ts < best)) pick = d, best = ts;
        }
        if (pick == c.world) break;
        const PendingBufs& D = c.Es[pick]->qs->qp;
        memcpy(rows + (u64)w * 256, D.h_rows + (u64)at[pick] * 128, 128);
        states[w] = D.h_states[at[pick]];
        at[pick]++;
    }
    return w;
}

// rows: m placed rows with their states.  Fills every row's resolution half; returns through
// *complete whether every posted or voided row found its resolving record.
static int pending_resolutions(const QueryCall& c, u32 m, u8* rows, const u8* states, bool* complete) {
    PendingBufs& P = c.Es[0]->qs->qp;
    u32 resolved = 0;
    for (u32 i = 0; i < m; i++) resolved += (states[i] & (PENDING_POSTED | PENDING_VOIDED)) != 0;
    for (u32 i = 0; i < m; i++) memset(rows + (u64)i * 256 + 128, 0, 128);
    *complete = true;
    if (resolved == 0) return TBGPU_STATUS_OK;
    const u32 slots = tb_change_set_slots(resolved), mask = slots - 1;
    memset(P.h_set, 0, (u64)slots * 4);
    u32 nr = 0;
    u64 ts_floor = ~0ULL;  // the oldest resolved row: nothing at or below it resolves any of them
    for (u32 i = 0; i < m; i++) {
        if (!(states[i] & (PENDING_POSTED | PENDING_VOIDED))) continue;
        const u8* r = rows + (u64)i * 256;
        P.h_row_of[change_set_insert(P.h_set, mask, P.h_ids, &nr, change_row_word(r, 0), change_row_word(r, 1))] = i;
        ts_floor = std::min(ts_floor, change_row_word(r, 15));
    }
    const int status = query_side_by_side(c.Es, c.world, [&](u32 d) -> int {
        tbgpu* E = c.Es[d];
        PendingBufs& D = E->qs->qp;
        HIPCK(hipSetDevice(E->device));
        if (d) {
            memcpy(D.h_set, P.h_set, (u64)slots * 4);
            memcpy(D.h_ids, P.h_ids, (u64)nr * 16);
        }
        HIPCK(hipMemcpyAsync(D.d_set, D.h_set, (u64)slots * 4, hipMemcpyHostToDevice, E->stream));
        HIPCK(hipMemcpyAsync(D.d_ids, D.h_ids, (u64)nr * 16, hipMemcpyHostToDevice, E->stream));
        HIPCK(hipMemsetAsync(D.d_slots, 0, (u64)nr * 128, E->stream));
        const u64 n = E->log_next, per = (u64)PENDING_THREADS * PENDING_TILES, nb = (n + per - 1) / per;
        if (nb) {
            hipLaunchKernelGGL(tb_pending_resolutions, dim3((unsigned)nb), dim3(PENDING_THREADS), (size_t)slots * 4, E->stream, E->T, n,
                               ts_floor, (const u32*)D.d_set, mask, (const u64*)D.d_ids, D.d_slots);
            HIPCK(hipGetLastError());
        }
        HIPCK(hipMemcpyAsync(D.h_slots, D.d_slots, (u64)nr * 128, hipMemcpyDeviceToHost, E->stream));
        return TBGPU_STATUS_OK;
    });
    if (status) return status;
    // A slot is filled by at most one shard: the home of the resolving record's own id.
    for (u32 s = 0; s < nr; s++) {
        bool found = false;
        for (u32 d = 0; d < c.world && !found; d++) {
            const u8* rec = c.Es[d]->qs->qp.h_slots + (u64)s * 128;
            if (change_row_word(rec, 15) == 0) continue;
            memcpy(rows + (u64)P.h_row_of[s] * 256 + 128, rec, 128);
            found = true;
        }
        if (!found) *complete = false;
    }
    return TBGPU_STATUS_OK;
}

extern "C" int tbgpu_get_pending_transfers(tbgpu_t* E, const tbgpu_pending_filter* filter, void* out_rows, uint8_t* out_states,
                                           uint32_t out_cap_rows, tbgpu_query_result* result) {
    static_assert(sizeof(tbgpu_pending_filter) == 64 && sizeof(tbgpu_pending_row) == 256, "the filter is 64 bytes, a row 256");
    static_assert(PENDING_OPEN == TBGPU_PENDING_OPEN && PENDING_EXPIRED == TBGPU_PENDING_EXPIRED &&
                  PENDING_POSTED == TBGPU_PENDING_POSTED && PENDING_VOIDED == TBGPU_PENDING_VOIDED &&
                  PENDING_ROWS_MAX == TBGPU_PENDING_ROWS_MAX, "k_query.h's and k_pending.h's constants are the header's");
    API_ENTER(E, false);
    if (!filter || !out_rows || !out_states || !result) {
        return fail(TBGPU_STATUS_INVALID, "get_pending_transfers: a NULL filter, out_rows, out_states or result");
    }
    QueryCall c;
    result->count = 0;
    result->matched = 0;
    result->complete = query_engines(E, true, &c);
    c.k = std::min<u32>(std::min<u32>(filter->limit, out_cap_rows), PENDING_ROWS_MAX);
    if (!pending_filter_valid(filter)) return TBGPU_STATUS_OK;
    const bool reversed = (filter->flags & TBGPU_FILTER_REVERSED) != 0;
    QueryPendingFilter F{};
    F.id_lo = filter->account_id_lo;
    F.id_hi = filter->account_id_hi;
    F.ts_min = filter->timestamp_min;
    F.ts_max = filter->timestamp_max ? filter->timestamp_max : ~0ULL;
    F.now = filter->now ? filter->now : tbgpu_commit_timestamp(E);
    F.debits = (filter->flags & TBGPU_FILTER_DEBITS) != 0;
    F.credits = (filter->flags & TBGPU_FILTER_CREDITS) != 0;
    F.want = filter->flags & PENDING_STATES;
    for (u32 d = 0; d < c.world; d++) {
        F.states = c.Es[d]->qs->qp.d_states;
        const int st = query_enqueue(c.Es[d], F, c.k, reversed);
        if (st) return query_end(result, st);
    }
    // Every engine is waited for, whatever an earlier one returned.
    u32 cnt[NODE_WORLD_MAX] = {};
    u64 matched = 0;
    int status = TBGPU_STATUS_OK;
    for (u32 d = 0; d < c.world; d++) {
        u64 m = 0;
        const int st = query_collect(c.Es[d], c.Es[d]->qs->qp.h_rows, &cnt[d], &m);
        if (st && status == TBGPU_STATUS_OK) status = st;
        matched += m;
    }
    if (status) return query_end(result, status);
    const u32 m = pending_place_rows(c, cnt, reversed, (u8*)out_rows, out_states);
    bool resolved = true;
    if (m) status = pending_resolutions(c, m, (u8*)out_rows, out_states, &resolved);
    if (status) return query_end(result, status);
    if (!resolved) result->complete = 0;
    result->count = m;
    result->matched = matched;
    return TBGPU_STATUS_OK;
}
