/*
 * tbgpu.h — C ABI of the MI355X batch-commit engine for TigerBeetle's create_accounts /
 * create_transfers state-machine path.
 *
 * Drop-in boundary: these entry points are what a Zig `StateMachineType` wrapper binds through
 * `@cImport` to replace the reference's synchronous commit:
 *
 *   reference interface                                   replaced by
 *   ----------------------------------------------------  ----------------------------------------
 *   StateMachine.init(allocator, grid, options)            tbgpu_init
 *     (src/state_machine.zig:264-278)
 *   StateMachine.deinit / reset (:280-299)                 tbgpu_deinit / tbgpu_reset
 *   StateMachine.prefetch (:345-506)                       tbgpu_prefetch (stages a pageable body)
 *   StateMachine.commit(client, op, timestamp, operation,  tbgpu_commit (one prepare) and
 *     input, output) -> usize (:508-540)                     tbgpu_commit_many (N prepares, one
 *                                                             device pass; same bytes as N commits)
 *   execute_lookup_accounts / _transfers (:700-736)        tbgpu_commit with operation 130 / 131
 *   the transfers groove's account-id index trees          tbgpu_get_account_transfers (no reference
 *     (:140-178; no reference operation reads them)          operation: specified below)
 *   both grooves' user_data / ledger / code / timestamp     tbgpu_query_transfers, tbgpu_query_accounts
 *     index trees (:103-169; likewise unread)                (likewise)
 *   (later references: the account_balances groove)        tbgpu_get_account_balances (likewise;
 *                                                             derived from the log, nothing stored)
 *   (later references: get_change_events)                  tbgpu_get_change_events (likewise)
 *   (no reference: accounts as of a timestamp)             tbgpu_lookup_accounts_at (likewise)
 *   (no reference: a trial balance per ledger)             tbgpu_get_ledger_balances (likewise)
 *   (no reference: pending transfers with their state)     tbgpu_get_pending_transfers (likewise)
 *   (no reference: account statements over a period)       tbgpu_get_account_statements (likewise)
 *   (no reference: time-weighted balances over a period)   tbgpu_get_account_balance_integrals (likewise)
 *   (no reference: statements per bucket of a period)      tbgpu_get_account_statement_series (likewise)
 *   (no reference: who paid whom over a period)            tbgpu_get_account_flow_matrix (likewise)
 *   (no reference: who an account dealt with)              tbgpu_get_account_counterparties (likewise)
 *   (no reference: the accounts a period's records name)   tbgpu_get_active_accounts (likewise)
 *   (no reference: a balance's low and high over a period) tbgpu_get_account_balance_extremes (likewise)
 *   `setup` action of the table tests (:1398-1407)         tbgpu_test_set_balances (test only)
 *   StateMachine.commit_timestamp field (:251)             tbgpu_commit_timestamp
 *
 * Layouts are the reference's extern structs (src/tigerbeetle.zig:7-249), identical to the C
 * client header (src/clients/c/tb_client.h:25-64,150-158): Account and Transfer are 128-byte
 * little-endian records, results are {uint32 index, uint32 result} pairs, only non-ok events,
 * ascending index.  Operation numbers: 128 create_accounts, 129 create_transfers,
 * 130 lookup_accounts, 131 lookup_transfers (src/state_machine.zig:208-214).
 *
 * Conventions (src/state_machine.zig:508-540):
 *   - Every call is synchronous unless its name ends in _async; calls never overlap.
 *   - Invalid input is reported through result codes, never through the status.
 *   - A non-zero status is TBGPU_STATUS_INVALID (bad arguments: the reference could not have
 *     been called that way), TBGPU_STATUS_PANIC (the reference would have trapped: an overflow
 *     assert, a failed invariant, `timestamp <= commit_timestamp`), or TBGPU_STATUS_DEVICE
 *     (a HIP error).  The Zig wrapper turns PANIC/DEVICE into @panic.
 *   - No allocation after tbgpu_init: every device buffer, pinned host buffer and HIP event is
 *     made there (tbgpu_debug_allocations, tbgpu_bench.h, counts them; tests/test_gpu_alloc.py
 *     holds the commit, prefetch and write-back entry points to zero).  tbgpu_deinit, and a
 *     tbgpu_init that fails, release every one of them (tbgpu_debug_live).
 *   - A device panic (the reference would have trapped mid-commit) leaves state the reference
 *     never reaches, so the engine stops: every later call that changes state returns
 *     TBGPU_STATUS_PANIC until tbgpu_reset (or tbgpu_deinit).  Reads (exports, stats) still work.
 *   - Device exclusivity: the ordered fallback kernel (tb_flow) synchronises its workgroups with a
 *     software grid barrier among the workgroups it ADMITS at its start — those resident within
 *     ~50 us of the first one (at most a quarter of the CUs, shared among this process's engines on
 *     the device); a workgroup that starts later exits, and the admitted ones cover the pass.  So a
 *     co-tenant that holds CUs makes a pass slower, never a stall (tests/test_gpu_liveness.py
 *     launches tb_flow 8x over what the device holds).  tbgpu_init still checks once that a grid
 *     of that shape can be co-resident (within 200 ms) and fails with TBGPU_STATUS_DEVICE on a
 *     device other work holds; one engine process per device is the supported deployment.  Every
 *     wait stays bounded (PANIC_FLOW_STALL: an engine bug, never a hang).
 */
#ifndef TBGPU_H
#define TBGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TBGPU_STATUS_OK 0
#define TBGPU_STATUS_INVALID 1
#define TBGPU_STATUS_PANIC 2
#define TBGPU_STATUS_DEVICE 3

#define TBGPU_OPERATION_CREATE_ACCOUNTS 128
#define TBGPU_OPERATION_CREATE_TRANSFERS 129
#define TBGPU_OPERATION_LOOKUP_ACCOUNTS 130
#define TBGPU_OPERATION_LOOKUP_TRANSFERS 131

/* batch_max.create_transfers for the production config (src/state_machine.zig:46-65). */
#define TBGPU_BATCH_EVENTS_MAX 8191u

/* Config flags. */
#define TBGPU_CONFIG_PROFILE (1u << 0) /* time every kernel with HIP events (tbgpu_get_stats) */
/* Ordered fallback on one lane in batch order (tb_replay) instead of the parallel flow path
 * (tb_flow); identical results, for cross-checking the two. */
#define TBGPU_CONFIG_SEQUENTIAL_FALLBACK (1u << 1)
/* Limit checks (tb_flow bounds): sweep whatever the first scan round leaves undecided in event
 * order (TBGPU_CONFIG_SWEEP_EARLY), or never sweep (TBGPU_CONFIG_SWEEP_OFF: rounds until they
 * converge, else the ordered run).  Identical results; for cross-checking the paths. */
#define TBGPU_CONFIG_SWEEP_EARLY (1u << 2)
#define TBGPU_CONFIG_SWEEP_OFF (1u << 3)
/* The sweep as one wave walking the undecided checks in event order, 64 a window (round 2's form),
 * instead of one walker per limit account.  Identical results; for cross-checking the two. */
#define TBGPU_CONFIG_SWEEP_WINDOW (1u << 4)

#define TBGPU_DEVICES_MAX 16u

typedef struct tbgpu_config {
    uint64_t accounts_max;      /* HBM account table capacity (the groove's object count) */
    uint64_t transfers_max;     /* HBM transfer store capacity (the whole ledger, over every device);
                                   137 bytes per position: record, posted byte, timestamp plane */
    uint32_t pass_events_max;   /* max events in one device pass (tbgpu_commit_many); on a node: per
                                   source device and pass */
    uint32_t pass_batches_max;  /* max prepares in one device pass; on a node: per source device */
    int32_t device;             /* HIP device ordinal (device_count <= 1) */
    uint32_t flags;             /* TBGPU_CONFIG_* */
    /* SURVEY.md §8b device_mask.  device_count >= 2: a NODE engine over devices[0 .. device_count),
     * one shard per entry (an ordinal may repeat: logical shards sharing a GPU).  Every entry point
     * of this header works on a node engine with the same semantics: accounts hash-partitioned
     * (record and balances on their owner shard only), transfers on their home shard, each
     * create_transfers pass routed across the shards by kernels reading their peers' HBM over xGMI
     * (tigerbeetle_amd/csrc/node.h).  Not on a node: tbgpu_commit_device_async and the
     * tbgpu_shard.h primitives (they take one device's engine). */
    uint32_t device_count;
    int32_t devices[TBGPU_DEVICES_MAX];
} tbgpu_config;

typedef struct tbgpu tbgpu_t;

/* StateMachine.init: allocates every HBM table up front (static allocation). */
int tbgpu_init(const tbgpu_config* config, tbgpu_t** out);
void tbgpu_deinit(tbgpu_t* engine);
/* StateMachine.reset: empties every table, commit_timestamp = 0. */
int tbgpu_reset(tbgpu_t* engine);

/* StateMachine.commit for one prepare.  `input` holds `input_len` bytes (a multiple of 128 for
 * creates, of 16 for lookups); `output` receives the reply body and `*out_len` its size.
 * Byte-identical to the reference for every operation. */
int tbgpu_commit(tbgpu_t* engine, uint8_t operation, uint64_t timestamp, const void* input,
                 uint32_t input_len, void* output, uint32_t output_cap, uint32_t* out_len);

/* StateMachine.prefetch (src/state_machine.zig:345-506) for the prepare about to be committed.  The
 * objects are HBM-resident; what is staged is the body: a pageable create body starts its copy to
 * HBM at once, and the following tbgpu_commit of the same body (same pointer and length) only waits
 * for it.  A body in registered host memory (tbgpu_register_host: the message pool) is not staged:
 * the commit's first kernel reads it through, which measured faster than a DMA the replica's serial
 * prefetch -> commit leaves nothing to overlap with — except while the copy-out of an
 * asynchronous write-back written every few commits is in flight: then it is staged, so the commit
 * reads HBM and the copy-out need not wait for the commit's PCIe reads.  Completes
 * immediately (the reference allows the callback inside the call, src/lsm/groove.zig:723-742).
 * The staged copy belongs to the very next call only, if that call is tbgpu_commit of this body
 * (the replica's prefetch(op) -> commit(op)); any other call drops it.  The body must not change
 * between the two (a prepare message is immutable while its op commits, as in the reference). */
int tbgpu_prefetch(tbgpu_t* engine, uint8_t operation, const void* input, uint32_t input_len);

/* N consecutive prepares of the same create operation, pass_batches_max prepares per device pass
 * (tbgpu_commit_pipelined with chunk_batches = 0); identical results to N sequential tbgpu_commit
 * calls (timestamps strictly increasing). */
int tbgpu_commit_many(tbgpu_t* engine, uint8_t operation, uint32_t n, const uint64_t* timestamps,
                      const void* const* inputs, const uint32_t* input_lens, void* const* outputs,
                      uint32_t* out_lens);

/* Pipelined commit of N prepares from host memory: the replica's prefetch -> commit overlap
 * (src/state_machine.zig:345-506, src/vsr/replica.zig:3324-3665) with the objects HBM-resident.
 * Prepares are grouped into chunks of up to `chunk_batches` prepares (0: pass_batches_max); chunk
 * c+1's bodies cross PCIe while chunk c commits, and chunk c's replies come back as soon as it is
 * committed.  Bodies in memory registered with tbgpu_register_host (or otherwise pinned) move by
 * DMA; runs of address-contiguous prepares move as one copy.  Results are identical to N sequential
 * tbgpu_commit calls.  latency_ms (optional, N entries): per-prepare submit-to-reply time, from the
 * start of its chunk's PCIe copy to its reply landing in host memory (device clock).
 * On a node engine the bodies may also be in device memory (UVA pointers): a source shard's block of a
 * pass whose prepares sit back to back in that shard's own HBM is read in place (the node's
 * device-resident commit: prepares received or generated on each GPU), anything else is copied to it
 * (from another GPU over xGMI).  Replies still land in the host `outputs`. */
int tbgpu_commit_pipelined(tbgpu_t* engine, uint8_t operation, uint32_t n, const uint64_t* timestamps,
                           const void* const* inputs, const uint32_t* input_lens, void* const* outputs,
                           uint32_t* out_lens, uint32_t chunk_batches, double* latency_ms);

/* Device-resident throughput entry point: `events_dev` holds sum(batch_lens) events back to back
 * in HBM; batch k's reply is written to results_dev + 8*offset_k (offset_k = sum of earlier
 * batch lengths) and its byte count to reply_bytes_dev[k].  Enqueued on the engine's stream;
 * call tbgpu_sync() to wait and collect the status. */
int tbgpu_commit_device_async(tbgpu_t* engine, uint8_t operation, uint32_t n_batches,
                              const uint64_t* timestamps, const uint32_t* batch_lens,
                              const void* events_dev, void* results_dev, uint32_t* reply_bytes_dev);
int tbgpu_sync(tbgpu_t* engine);

/* Zero-copy create_transfers: the device address where the next `events` transfer records will be
 * stored (the transfer log from the engine's next position; the groove's insert,
 * src/lsm/groove.zig:950-1014, lands here).  Prepares placed there — by DMA from the message
 * buffers, by a peer, by a generator — and committed with tbgpu_commit_device_async(operation 129,
 * events_dev = *window) are committed IN PLACE: a committed create's record is its event where it
 * lies, and the pass stores its 8-byte timestamp into a dense plane beside the log (one u64 per log
 * position, 8 bytes of HBM per transfers_max) instead of copying 128 bytes (results identical to a
 * copy commit).  After the commit the window's bytes are the events as placed — a committed
 * create's timestamp field may still read 0 — so records are read through the API (lookups,
 * queries, exports, the write-back), which all return them with their timestamps, never from the
 * window.  The window is valid until the next call that stores transfers; INVALID when the log
 * cannot hold `events` more, or on a node engine. */
int tbgpu_log_window(tbgpu_t* engine, uint64_t events, void** window);

/* Host-memory registration for the replica's message pool (allocated once at init, like every
 * reference buffer): prepare bodies inside registered memory reach HBM by direct DMA. */
int tbgpu_register_host(tbgpu_t* engine, void* ptr, uint64_t bytes);
int tbgpu_unregister_host(tbgpu_t* engine, void* ptr);

/* StateMachine.commit_timestamp (src/state_machine.zig:251). */
uint64_t tbgpu_commit_timestamp(tbgpu_t* engine);

/* Test-only: the table harness `setup` action (src/state_machine.zig:1398-1407).
 * balances = {dp_lo, dp_hi, dpost_lo, dpost_hi, cp_lo, cp_hi, cpost_lo, cpost_hi}. */
int tbgpu_test_set_balances(tbgpu_t* engine, uint64_t id_lo, uint64_t id_hi,
                            const uint64_t balances[8]);

/* Parity read-back: every live record, sorted by id ascending; *count = records written. */
int tbgpu_export_accounts(tbgpu_t* engine, void* out, uint64_t cap, uint64_t* count);
int tbgpu_export_transfers(tbgpu_t* engine, void* out, uint64_t cap, uint64_t* count);
/* Posted groove (src/state_machine.zig:185-198): {pending_timestamp, fulfillment} pairs, sorted. */
int tbgpu_export_posted(tbgpu_t* engine, uint64_t* out_pairs, uint64_t cap, uint64_t* count);

/* Groove write-back for a durable replica (StateMachine.checkpoint / compact,
 * src/state_machine.zig:542-582; groove insert / upsert, src/lsm/groove.zig:902-963): the objects
 * changed since the previous call (or since init / reset) — accounts created or re-balanced (full
 * records, in no particular order: the groove sorts its mutable table itself), transfers created
 * (by timestamp), posted-groove entries created or changed ({pending timestamp, fulfillment} pairs,
 * by timestamp).  The cost follows the changes, not the tables.  If a buffer is too small the call
 * returns TBGPU_STATUS_INVALID with the sizes needed in *counts and nothing advances.  Buffers in
 * registered host memory (tbgpu_register_host) are filled by DMA. */
typedef struct tbgpu_delta_counts {
    uint64_t accounts;
    uint64_t transfers;
    uint64_t posted;
    uint64_t created_after;  /* accounts with a timestamp above this were created since the previous
                                write-back (groove insert); the others changed (groove upsert) */
} tbgpu_delta_counts;
int tbgpu_checkpoint_delta(tbgpu_t* engine, void* accounts_out, void* accounts_before_out, uint64_t accounts_cap,
                           void* transfers_out, uint64_t transfers_cap, uint64_t* posted_out, uint64_t posted_cap,
                           tbgpu_delta_counts* counts);
/* accounts_before_out (nullable, 64 B per account): {dp, dpost, cp, cpost} as of the previous
 * write-back (zero for accounts created since) — the old object a groove upsert diffs the balance
 * index trees against (src/lsm/groove.zig:925-963).
 * The buffers are checked before anything runs against what the write-back can emit at most
 * (transfers and posted entries: the transfer-log positions written since; accounts: two per such
 * position plus the listed creates, or every live account after creates the engine could not list):
 * a refused call returns those sizes in *counts and changes nothing. */

/* The same write-back without the wait (StateMachine.compact is asynchronous,
 * src/state_machine.zig:542-567; the replica's compact stage, src/vsr/replica.zig:3088-3091): the
 * state it describes is captured in stream order with the commits (the accounts the bar's transfers
 * name, with their balances; the next commits follow the capture), the rest is gathered on a
 * low-priority stream beside them, and the objects cross PCIe into the caller's buffers by DMA,
 * one slice after each one-prepare tbgpu_commit's body read (all at once after a commit whose body
 * tbgpu_prefetch staged; the rest at the wait).  A write-back every few commits whose objects
 * filled those bounds is sent at the bounds from the first commit after it (the bytes past the
 * counts land in the caller's buffers, unread; tbgpu_stats.write_backs_bound).
 * tbgpu_checkpoint_delta_wait returns the counts once the
 * objects have landed (transfers and posted entries sorted as above); until then the buffers belong
 * to the engine, and no other write-back may start.  Needs buffers registered with
 * tbgpu_register_host and large enough for the bounds above; otherwise (or past one slice of the
 * engine's write-back buffers) the call runs the synchronous write-back and the wait returns at
 * once.  A node engine (device_count >= 2) merges its shards' objects at the call (owners'
 * balances, homes' records, on the host) and its wait returns at once: the same contract, without the
 * single device's overlap with the next commits. */
int tbgpu_checkpoint_delta_async(tbgpu_t* engine, void* accounts_out, void* accounts_before_out, uint64_t accounts_cap,
                                 void* transfers_out, uint64_t transfers_cap, uint64_t* posted_out, uint64_t posted_cap);
int tbgpu_checkpoint_delta_wait(tbgpu_t* engine, tbgpu_delta_counts* counts);

/* Replica restart (StateMachine.open, src/state_machine.zig:322-334, then WAL replay from the
 * checkpoint): the HBM tables start empty while the forest holds the checkpointed objects.  The
 * wrapper's prefetch (src/state_machine.zig:345-506) reads the objects a prepare needs from the
 * forest and loads the ones the engine lacks: objects the engine already holds are newer and are
 * left as they are.  posted_state per transfer: 0 = no posted entry, 1 = posted, 2 = voided. */
int tbgpu_load_accounts(tbgpu_t* engine, const void* accounts, uint32_t n);
int tbgpu_load_transfers(tbgpu_t* engine, const void* transfers, const uint8_t* posted_state, uint32_t n);

/* Bounded residency.  The transfer log holds tbgpu_config.transfers_max records; a replica that
 * outlives it evicts what its forest already holds and loads it back when a prepare names it — the
 * reference's groove keeps every transfer reachable through its cache and LSM levels
 * (src/lsm/groove.zig:602-898), loaded by prefetch before commit (src/state_machine.zig:419-467).
 *   tbgpu_evict_transfers: drops the transfers the last write-back (tbgpu_checkpoint_delta) covered,
 *     except the newest `keep` log positions; the rest of the log is compacted and re-indexed.
 *     *evicted = transfers dropped.  Synchronous.  Only right after a write-back: with an
 *     asynchronous write-back in flight, or any log position written since the last one (a commit,
 *     a load), it returns TBGPU_STATUS_INVALID and changes nothing (an unwritten post / void may name
 *     a pending transfer the cut would drop, and the next write-back needs that record).
 *   tbgpu_transfers_maybe_cold: for n ids ({lo, hi} pairs), cold[i] = 1 when the engine does not
 *     hold id i and may have evicted it (a Bloom filter of evicted ids: false positives only).  The
 *     wrapper's prefetch loads the cold ids its forest holds (tbgpu_load_transfers, with their posted
 *     state) before the commit of a prepare that names them (its ids and post / void pending ids);
 *     an id it does not load is taken as absent, as the reference's groove would report it.
 * A node engine evicts per home shard (each shard's log keeps its share of `keep`; log_used in
 * tbgpu_stats is the fullest shard's fill in units of the node's capacity) and answers each id's
 * cold query on its home shard. */
int tbgpu_evict_transfers(tbgpu_t* engine, uint64_t keep, uint64_t* evicted);
int tbgpu_transfers_maybe_cold(tbgpu_t* engine, const uint64_t* ids, uint32_t n, uint8_t* cold);

/* get_account_transfers: which transfers touched one account.  The reference maintains the
 * debit_account_id / credit_account_id index trees of the transfers groove for this query
 * (src/state_machine.zig:140-178) but has no operation that reads them, and its Operation enum has no
 * number for it — so it is an entry point of its own (tbgpu_commit keeps refusing operations outside
 * 128-131), and this comment is its specification.
 *   What matches: a committed, resident transfer (its record is live: the id index holds its id at
 *     that log position) whose debit account id equals account_id under DEBITS, or whose credit
 *     account id equals it under CREDITS (a record matching on both sides is returned once), with its
 *     timestamp in [timestamp_min, timestamp_max] (0 leaves that end open).  Post / void records carry
 *     their pending transfer's account ids (src/state_machine.zig:971-985) and match under those.
 *     Failed events, withdrawn speculative records and rolled-back chain members never match.
 *   What is returned: the first min(limit, out_cap_records, TBGPU_BATCH_EVENTS_MAX) matches (one reply
 *     is one message body) by timestamp ascending, or descending from the newest under REVERSED —
 *     whole 128-byte records, the bytes lookup_transfers returns for the same ids — whatever order the
 *     log holds them in (loads and upserts append out of timestamp order).  `matched` counts all.
 *   Invalid filters are never a status: account_id 0 or 2^128-1, timestamp_min or timestamp_max
 *     2^64-1, a non-zero timestamp_max below timestamp_min, limit 0, neither DEBITS nor CREDITS, an
 *     unknown flag bit, a non-zero reserved byte — each returns TBGPU_STATUS_OK with count = matched
 *     = 0.  A NULL filter, out or result is TBGPU_STATUS_INVALID.
 *   Synchronous; drains a pending tbgpu_commit_device_async first, as tbgpu_commit does.  A read: it
 *     changes nothing (commit_timestamp, balances, log, index, stats, the write-back snapshot), works
 *     on an engine a device panic stopped, allocates nothing, and is legal while an asynchronous
 *     write-back is in flight.
 *   A node engine has the same contract: every home shard scans its own log on its own device and the
 *     host merges the shards' answers by timestamp under the limit. */
#define TBGPU_FILTER_DEBITS   (1u << 0)  /* match debit_account_id  == account_id */
#define TBGPU_FILTER_CREDITS  (1u << 1)  /* match credit_account_id == account_id */
#define TBGPU_FILTER_REVERSED (1u << 2)  /* newest first */

typedef struct tbgpu_account_filter {    /* 64 bytes, little-endian, no padding */
    uint64_t account_id_lo, account_id_hi;
    uint64_t timestamp_min;              /* inclusive; 0 = no lower bound */
    uint64_t timestamp_max;              /* inclusive; 0 = no upper bound */
    uint32_t limit;
    uint32_t flags;
    uint8_t  reserved[24];               /* must be zero */
} tbgpu_account_filter;

typedef struct tbgpu_query_result {
    uint32_t count;     /* records written to out */
    uint32_t complete;  /* 1: no transfer was ever evicted from this engine (any shard of a node), so
                           `out` is the ledger's answer; 0: only the resident transfers were searched,
                           and the caller merges with its forest */
    uint64_t matched;   /* resident transfers matching the filter, before the limit */
} tbgpu_query_result;

int tbgpu_get_account_transfers(tbgpu_t* engine, const tbgpu_account_filter* filter,
                                void* out, uint32_t out_cap_records, tbgpu_query_result* result);

/* get_account_transfers_many: up to TBGPU_QUERY_FILTERS_MAX account filters answered by one read of the
 * transfer log instead of one read each (a replica serving several get_account_transfers requests
 * between two writes hands them over together).  This sentence is its specification:
 *   Answer i is exactly what tbgpu_get_account_transfers(engine, &filters[i],
 *     (uint8_t*)out + i * out_cap_records * 128, out_cap_records, &results[i]) would have produced at the
 *     same point: the records, their order, count, matched and complete are all the same.
 *   So out has room for n_filters * out_cap_records records, answer i starts at record i *
 *     out_cap_records and holds min(limit_i, out_cap_records, TBGPU_BATCH_EVENTS_MAX) records at most;
 *     bytes of a slot past its count are not written.  REVERSED, DEBITS / CREDITS and the window apply
 *     per filter; filters may name the same account, be identical, or mix directions.  An invalid
 *     filter (the rules above) yields count = matched = 0 for its entry only, never a status; the other
 *     filters are answered.  complete is the same for every entry.
 *   n_filters == 0 returns TBGPU_STATUS_OK and writes nothing.  n_filters > TBGPU_QUERY_FILTERS_MAX is
 *     TBGPU_STATUS_INVALID and writes nothing; so is a NULL filters, out or results with n_filters > 0.
 *     After any failing status no result names a record.
 *   The call contract of tbgpu_get_account_transfers: synchronous, drains a pending
 *     tbgpu_commit_device_async first, a read that changes nothing, works on a stopped engine,
 *     allocates nothing after tbgpu_init, and is legal beside an asynchronous write-back.
 *   A node engine: every home shard scans its own log once for the whole batch, side by side, and the
 *     host merges per filter.
 *   Cost: one scan of the log for the batch, plus one more read of the chunks that hold a wanted
 *     record.  A log out of timestamp order (loads, upserts) is answered filter by filter, as
 *     n_filters single calls would. */
#define TBGPU_QUERY_FILTERS_MAX 64u
int tbgpu_get_account_transfers_many(tbgpu_t* engine, const tbgpu_account_filter* filters, uint32_t n_filters,
                                     void* out, uint32_t out_cap_records /* per filter */,
                                     tbgpu_query_result* results /* [n_filters] */);

/* get_account_balances: an account's four balances as they stood right after each of its transfers.
 * Later references answer it from balance rows they store at every commit for accounts that opted in
 * with a `history` flag.  This engine stores nothing and asks for no flag: the transfer log is in HBM
 * and the account table holds the current balances, so the history is derived when asked, and the
 * commit path is not touched.  An entry point of its own, as above; this comment is its specification.
 *   Which rows: exactly the transfers tbgpu_get_account_transfers returns for the same filter and
 *     out_cap_records, in the same order, one 128-byte row per transfer.  count, matched and every
 *     invalid-filter rule are that call's: an invalid filter returns TBGPU_STATUS_OK with count =
 *     matched = 0; a NULL filter, out or result is TBGPU_STATUS_INVALID.
 *   What a row holds: the transfer's timestamp and the account's four balances right after that
 *     transfer committed.  Let R be every live resident record that names the account on either side
 *     (the DEBITS / CREDITS flags and the timestamp window choose rows, not what is summed).  A
 *     record's effect on the account's side — debits_* where it is the debit account, credits_* where
 *     it is the credit account — follows src/state_machine.zig:872-878 and :997-1007:
 *       a pending record   *_pending += amount
 *       a post             *_pending -= P, *_posted += amount
 *       a void             *_pending -= P
 *       any other          *_posted  += amount
 *     where P is the amount of the resident record whose id is the record's pending_id (for a void, P
 *     equals the void record's own amount).  Then
 *       balance_after(r) = current balances - the sum of the effects of the records in R with a
 *                          timestamp strictly above r's,
 *     per column modulo 2^128; the true values are in range, so the modular result is exact.  The
 *     anchor is the current balance, not zero, so the rows stay exact after the oldest transfers were
 *     evicted, after a restart from checkpointed balances (tbgpu_load_accounts) and after
 *     tbgpu_test_set_balances.
 *   complete: 1 when no transfer was ever evicted (tbgpu_get_account_transfers' rule) and every post
 *     record that entered a sum found its pending transfer resident; otherwise 0.  A post whose pending
 *     transfer is not resident is summed with P = its own amount.  Rows of a complete = 0 answer are
 *     still exact whenever every transfer of the account newer than the oldest returned row is
 *     resident and none of them is such an orphan post — the common case, eviction of an old prefix.
 *   The call contract of tbgpu_get_account_transfers: synchronous, drains a pending
 *     tbgpu_commit_device_async first, changes nothing, works on an engine a device panic stopped,
 *     allocates nothing (every buffer is made in tbgpu_init), legal beside an asynchronous write-back.
 *     It scans the log once more than tbgpu_get_account_transfers does.
 *   A node engine has the same contract: the rows are the merged answer; every home shard sums the
 *     effects of its own log on its own device, reading a post's pending transfer on the home shard of
 *     its pending_id; the host adds the shards' sums and takes the current balances from the account's
 *     owner shard. */
typedef struct tbgpu_account_balance {   /* 128 bytes, little-endian, no padding: the later
                                            reference's AccountBalance */
    uint64_t debits_pending_lo,  debits_pending_hi;
    uint64_t debits_posted_lo,   debits_posted_hi;
    uint64_t credits_pending_lo, credits_pending_hi;
    uint64_t credits_posted_lo,  credits_posted_hi;
    uint64_t timestamp;
    uint8_t  reserved[56];               /* zero */
} tbgpu_account_balance;

int tbgpu_get_account_balances(tbgpu_t* engine, const tbgpu_account_filter* filter,
                               void* out, uint32_t out_cap_records, tbgpu_query_result* result);

/* query_transfers / query_accounts: which transfers, or accounts, carry these field values.  The
 * reference maintains the user_data_128 / user_data_64 / user_data_32 / ledger / code / timestamp
 * index trees of both grooves (src/state_machine.zig:103-169) and no operation reads them; later
 * references read them through a QueryFilter.  Entry points of their own, as above,
 * and this comment is their specification.
 *   What matches: every non-zero field of the filter equals the object's stored field (AND; a 128-bit
 *     field compares both words), and the object's timestamp lies in [timestamp_min, timestamp_max]
 *     (0 leaves that end open).  A filter with every field zero is valid and matches every object in
 *     the window.
 *     Transfers: liveness as for tbgpu_get_account_transfers — failed events, withdrawn speculative
 *     records and rolled-back chain members never match; post / void records match on the bytes they
 *     store (src/state_machine.zig:971-985).
 *     Accounts: a live slot of the account table (a non-zero timestamp, an id that is not reserved).
 *   What is returned: the first min(limit, out_cap_records, TBGPU_BATCH_EVENTS_MAX) matches by timestamp
 *     ascending, or descending from the newest under REVERSED — whole 128-byte records, the bytes
 *     lookup_transfers / lookup_accounts return for the same ids; for accounts that is the current
 *     balances.  `matched` counts every match before the limit.
 *   complete: transfers, the rule above (no transfer was ever evicted, on any shard); accounts, always
 *     1 (accounts are never evicted).  An engine that was loaded lazily holds only what was loaded:
 *     INTEGRATION.md.
 *   Invalid filters are never a status: timestamp_min or timestamp_max 2^64-1, a non-zero
 *     timestamp_max below timestamp_min, limit 0, an unknown flag bit, a non-zero reserved byte — each
 *     returns TBGPU_STATUS_OK with count = matched = 0.  A NULL filter, out or result is
 *     TBGPU_STATUS_INVALID.
 *   The call contract of tbgpu_get_account_transfers: synchronous, drains a pending
 *     tbgpu_commit_device_async first, changes nothing, works on a stopped engine, allocates nothing,
 *     legal beside an asynchronous write-back.
 *   A node engine: transfers as above.  An account is answered by its owner shard only (a home's
 *     imported copies of foreign accounts and the sequencer's loaded copies never match), so it
 *     appears once, with the owner's balances; the host merges the shards' answers by timestamp. */
#define TBGPU_QUERY_REVERSED (1u << 0)   /* newest first */

typedef struct tbgpu_query_filter {      /* 64 bytes, little-endian, no padding */
    uint64_t user_data_128_lo, user_data_128_hi;   /* 0 (both words) = not filtered */
    uint64_t user_data_64;                         /* 0 = not filtered */
    uint32_t user_data_32;                         /* 0 = not filtered */
    uint32_t ledger;                               /* 0 = not filtered */
    uint16_t code;                                 /* 0 = not filtered */
    uint8_t  reserved[6];                          /* must be zero */
    uint64_t timestamp_min;                        /* inclusive; 0 = open */
    uint64_t timestamp_max;                        /* inclusive; 0 = open */
    uint32_t limit;
    uint32_t flags;
} tbgpu_query_filter;

int tbgpu_query_transfers(tbgpu_t* engine, const tbgpu_query_filter* filter, void* out, uint32_t out_cap_records,
                          tbgpu_query_result* result);
int tbgpu_query_accounts(tbgpu_t* engine, const tbgpu_query_filter* filter, void* out, uint32_t out_cap_records,
                         tbgpu_query_result* result);

/* get_change_events: the ledger's change stream — every committed transfer in a timestamp window, in
 * timestamp order, with both of its accounts as they stood right after it.  Later references keep a
 * groove for it; this engine stores nothing at commit and derives the account blocks from the log in
 * HBM and the current balances, as tbgpu_get_account_balances does for one account.  An entry point
 * of its own, as above; this comment is its specification.
 *   Which events: exactly the transfers tbgpu_query_transfers returns for a filter whose fields are
 *     all zero, with the same window, ascending by timestamp (there is no REVERSED), under
 *     k = min(limit, out_cap_events, TBGPU_CHANGE_EVENTS_MAX).  `matched` and the liveness rules are
 *     that call's.  Post and void records carry their pending transfer's account ids (the log stores
 *     them so).  The event's kind is read from the transfer's flags; there is no expired kind, as this
 *     reference never expires a pending transfer ("Timeouts").  A consumer pages with
 *     timestamp_min = the last event's timestamp + 1.
 *   The account blocks: an account's fields other than its four balances never change after it was
 *     created, so a block is the account's current record with the four balances replaced by the
 *     balances right after the event.  For event r and account a, per column modulo 2^128,
 *       balance_after(r, a) = current(a) - the sum of the effects on a of every live resident record
 *                             that names a and has a timestamp strictly above r's,
 *     with the effect table and the P rule of tbgpu_get_account_balances (a post whose pending transfer
 *     is not resident is summed with P = its own amount).  The anchor is the current balance: the
 *     blocks stay exact after eviction of an old prefix, after tbgpu_load_accounts and after
 *     tbgpu_test_set_balances; events older than such a step follow this definition, not the ledger's
 *     past.  An account the table does not hold (transfers loaded without their accounts) yields an
 *     all-zero block.
 *   complete: 1 only when no transfer was ever evicted, every post that entered a sum found its
 *     pending transfer resident, and every account named by a returned event was found.
 *   Invalid filters are never a status: timestamp_min or timestamp_max 2^64-1, a non-zero
 *     timestamp_max below timestamp_min, limit 0, a non-zero reserved byte — each returns
 *     TBGPU_STATUS_OK with count = matched = 0.  A NULL filter, out or result is TBGPU_STATUS_INVALID.
 *   The call contract of tbgpu_get_account_transfers: synchronous, drains a pending
 *     tbgpu_commit_device_async first, changes nothing, works on an engine a device panic stopped,
 *     allocates nothing (every buffer is made in tbgpu_init), legal beside an asynchronous write-back.
 *     It scans the log once more than tbgpu_query_transfers does.
 *   A node engine has the same contract: the events are the merged answer; every home shard sums the
 *     effects of its own log on its own device and stream, reading a post's pending transfer on the
 *     home shard of its pending_id; the host adds the shards' sums; each account's record comes from
 *     its owner shard. */
#define TBGPU_CHANGE_EVENTS_MAX 2730u   /* 384 B events in one message body: 2730*384 <= 8191*128 */

typedef struct tbgpu_change_events_filter {   /* 64 bytes, little-endian, no padding */
    uint64_t timestamp_min;   /* inclusive; 0 = open */
    uint64_t timestamp_max;   /* inclusive; 0 = open */
    uint32_t limit;
    uint8_t  reserved[44];    /* must be zero */
} tbgpu_change_events_filter;

typedef struct tbgpu_change_event {           /* 384 bytes, no padding */
    uint8_t transfer[128];        /* the bytes lookup_transfers returns for this id */
    uint8_t debit_account[128];   /* the bytes lookup_accounts would have returned for the record's
                                     debit account right after this transfer committed */
    uint8_t credit_account[128];  /* likewise, its credit account */
} tbgpu_change_event;

int tbgpu_get_change_events(tbgpu_t* engine, const tbgpu_change_events_filter* filter, void* out,
                            uint32_t out_cap_events, tbgpu_query_result* result);

/* lookup_accounts_at: the records of the accounts the caller names, as they stood at a timestamp the
 * caller names — what a statement run, an end-of-day close or a reconciliation starts from.  No
 * reference has an operation for it; this engine stores nothing at commit and derives the balances
 * from the log in HBM and the current balances, as tbgpu_get_change_events does for the accounts of a
 * page.  One scan of the log answers the call, whatever the number of ids.  An entry point of its own,
 * as above; this comment is its specification.
 *   Which records: lookup_accounts' — one 128-byte record per requested id that the account table
 *     holds, in request order.  Absent ids and the reserved ids (0, 2^128-1) are skipped; a repeated
 *     id is answered once per occurrence.  An account whose own timestamp is above `timestamp` did
 *     not exist then and is skipped like an absent one.  `matched` is the number of ids that yield a
 *     record; count = min(matched, out_cap_records), the first ones in request order; bytes past
 *     count records are not written.
 *   What a record holds: the account's current record with its four balances replaced by
 *       balance_at(a, T) = current(a) - the sum of the effects on a of every live resident record
 *                          that names a and has a timestamp strictly above T,
 *     per column modulo 2^128, with the effect table, the P rule and the liveness rule of
 *     tbgpu_get_account_balances (a post whose pending transfer is not resident is summed with P =
 *     its own amount).  The anchor is the current balance: the answers stay exact after eviction of
 *     an old prefix, after tbgpu_load_accounts and after tbgpu_test_set_balances; timestamps older
 *     than such a step follow this definition, not the ledger's past.
 *   timestamp == 0 means now: the answer is byte-identical to tbgpu_commit(operation 130) for the
 *     same ids, and no log is scanned.  A timestamp at or above every resident record's gives the same
 *     bytes, except for accounts loaded with a later timestamp, which the rule above skips; its scan
 *     reads the records' timestamps and nothing else.
 *   complete: 1 only when no transfer was ever evicted (any shard) and every post that entered a sum
 *     found its pending transfer resident; otherwise 0.
 *   timestamp == 2^64-1 returns TBGPU_STATUS_OK with count = matched = 0.  n == 0 returns
 *     TBGPU_STATUS_OK and writes nothing.  n > TBGPU_LOOKUP_AT_MAX, or a NULL ids, out or result with
 *     n > 0, is TBGPU_STATUS_INVALID and writes nothing.  After any failing status the result names
 *     no record.
 *   The call contract of tbgpu_get_account_transfers: synchronous, drains a pending
 *     tbgpu_commit_device_async first, a read that changes nothing (commit_timestamp, balances, log,
 *     index, stats, the write-back snapshot), works on an engine a device panic stopped, allocates
 *     nothing after tbgpu_init, legal beside an asynchronous write-back.
 *   A node engine has the same contract: every home shard scans its own log on its own device and
 *     stream, side by side, reading a post's pending transfer on the home shard of its pending_id;
 *     each account's record, and whether it existed at T, come from its owner shard only; the host
 *     adds the shards' sums. */
#define TBGPU_LOOKUP_AT_MAX 8191u   /* one lookup_accounts body */
int tbgpu_lookup_accounts_at(tbgpu_t* engine, uint64_t timestamp,
                             const void* ids /* n x {lo, hi} */, uint32_t n,
                             void* out, uint32_t out_cap_records,
                             tbgpu_query_result* result);

/* get_ledger_balances: a trial balance per ledger as of a timestamp the caller names — what a close
 * or a reconciliation asks first: does each ledger balance, and what were its totals at T.  No
 * reference has an operation for it; nothing is stored at commit, and the answer is one scan of the
 * account table (every account carries its ledger) plus, for T != 0, one scan of the log's records
 * newer than T (every record carries its own ledger).  An entry point of its own, as above; this
 * comment is its specification.
 *   Rows: one row per requested position, in request order, always.  A ledger no account carries
 *     yields a zero row (accounts = 0, ledger set); a repeated ledger is answered once per
 *     occurrence.  matched = n and count = min(n, out_cap_rows); bytes past count rows are not
 *     written.
 *   Sums, for a requested ledger L != 0 and T = timestamp, per column modulo 2^128:
 *       column(L, T) = the sum of current(a).column over every live account a with a.ledger == L
 *                      (those created after T included)
 *                      - the summed effects of every live resident record r with r.ledger == L and
 *                        r.timestamp strictly above T,
 *     with the effect table, the P rule and the liveness rule of tbgpu_get_account_balances (a post
 *     whose pending transfer is not resident is summed with P = its own amount).  A record's effect is
 *     subtracted from the debit columns once and from the credit columns once.  It is the record's own
 *     ledger field that assigns it to a row; no account is looked up from the log (a committed record's
 *     two accounts always share its ledger, and a post or void stores its pending transfer's).
 *   Anchor: the current balances.  After eviction of an old prefix, tbgpu_load_accounts or
 *     tbgpu_test_set_balances the answer follows this definition, not the ledger's past.  On an engine
 *     that saw none of those, a row equals the per-ledger sum of tbgpu_lookup_accounts_at over every
 *     account at T (accounts younger than T contribute zero), and debits_* == credits_* in every row
 *     at every T.
 *   Ledger 0: no account can carry it, so a requested 0 means every ledger together: that row sums
 *     every live account and every live resident record newer than T.  At T = 0 it is
 *     tbgpu_bench_ledger_summary's four sums and its account count.
 *   accounts: the live accounts of L whose creation timestamp is <= T; all of them when T = 0; over
 *     every ledger for L = 0.
 *   timestamp == 0 means now: no log is scanned.  A T at or above every resident record's timestamp
 *     gives the same sums, and its scan reads the records' timestamps and nothing else.
 *     timestamp == 2^64-1 returns TBGPU_STATUS_OK with count = matched = 0.
 *   n == 0 returns TBGPU_STATUS_OK and writes nothing.  n > TBGPU_LEDGERS_MAX, or a NULL ledgers, out
 *     or result with n > 0, is TBGPU_STATUS_INVALID and writes nothing.  After any failing status the
 *     result names no row.
 *   complete: tbgpu_lookup_accounts_at's rule — 1 only when no transfer was ever evicted (any shard)
 *     and no post without its resident pending transfer entered a sum.  An orphan post of a ledger
 *     nobody asked for, with 0 not asked either, enters no sum.
 *   The call contract of tbgpu_get_account_transfers: synchronous, drains a pending
 *     tbgpu_commit_device_async first, a read that changes nothing, works on an engine a device panic
 *     stopped, allocates nothing after tbgpu_init, legal beside an asynchronous write-back.
 *   A node engine has the same contract: each shard sums the accounts it owns (a home's imported
 *     copies and the sequencer's loaded copies never count) and scans its own log on its own device
 *     and stream, side by side, reading a post's pending amount on the home of its pending_id; the
 *     host adds the shards' sums.
 *   TBGPU_LEDGERS_MAX is 1,024 so that a workgroup's LDS — the requested ledgers as a set with twice
 *     as many slots, and a few hundred claimed bins — stays well within 64 KB, with room for a second
 *     workgroup on the compute unit. */
#define TBGPU_LEDGERS_MAX 1024u
typedef struct tbgpu_ledger_balance {      /* 128 bytes, little-endian, no padding */
    uint64_t debits_pending_lo,  debits_pending_hi;    /* the first 64 bytes: tbgpu_account_balance's */
    uint64_t debits_posted_lo,   debits_posted_hi;
    uint64_t credits_pending_lo, credits_pending_hi;
    uint64_t credits_posted_lo,  credits_posted_hi;
    uint64_t accounts;                     /* accounts of the ledger that existed at T */
    uint32_t ledger;
    uint8_t  reserved[52];                 /* zero */
} tbgpu_ledger_balance;
int tbgpu_get_ledger_balances(tbgpu_t* engine, uint64_t timestamp,
                              const uint32_t* ledgers, uint32_t n,
                              void* out, uint32_t out_cap_rows, tbgpu_query_result* result);

/* get_pending_transfers: the two-phase transfers of a window with their state — which holds are
 * outstanding, and what became of the others.  lookup_transfers returns a pending record unchanged
 * whether it is open, was posted, was voided or has timed out; this call says which, and hands back
 * the post or void record with it.  No reference has an operation for it; nothing is stored at commit,
 * the answer is a scan of the log under a third predicate and, when a returned row is resolved, one
 * more scan that joins the resolving records.  An entry point of its own, as above; this comment is
 * its specification.
 *   What matches: a live resident record (tbgpu_get_account_transfers' liveness rule: the id index
 *     holds its id at that log position) whose flags carry `pending`, whose timestamp lies in
 *     [timestamp_min, timestamp_max] (0 leaves that end open), whose account — if account_id != 0 —
 *     sits on a wanted side (DEBITS / CREDITS, as in tbgpu_get_account_transfers), and whose state is
 *     among the requested TBGPU_PENDING_* bits.  With account_id 0 the side bits are ignored.
 *   State of a pending record p, as the commit path decides it for a post or void that arrives at
 *     timestamp `now`: the posted groove says posted -> POSTED; it says voided -> VOIDED; otherwise, if
 *     p.timeout != 0 and p.timestamp + p.timeout * 10^9 <= now -> EXPIRED (the sum is taken in u64 and
 *     saturates at 2^64-1: a wrapped sum never expires); otherwise -> OPEN.  `now` is only the clock
 *     for expiry: posted and voided are always the engine's current state.  now == 0 means
 *     tbgpu_commit_timestamp (a node: the node's own).  The engine never expires a pending transfer by
 *     itself, so an EXPIRED row's amount still stands in its accounts' *_pending balances.
 *   What is returned: the first k = min(limit, out_cap_rows, TBGPU_PENDING_ROWS_MAX) matches by the
 *     pending record's timestamp, ascending, or newest first under REVERSED, whatever order the log
 *     holds them in.  Row i is 256 bytes: the pending record (the bytes lookup_transfers returns) and
 *     its resolution; out_states[i] holds the single TBGPU_PENDING_* bit of row i.  `matched` counts
 *     every match.  Bytes past `count` rows and states are not written.
 *   Resolution: for a returned POSTED or VOIDED row, the live resident record with the post or void
 *     flag (and not `pending`) whose pending_id equals the row's id; commits produce at most one.  It
 *     may sit anywhere later in the log, and on a node on another shard (a post lives on the home of
 *     its own id).  All zero for OPEN and EXPIRED rows, and for a resolved row whose resolving record
 *     is not resident (it was evicted, or the pending transfer was loaded by tbgpu_load_transfers with
 *     a posted state and nothing else).
 *   complete: 1 only when no transfer was ever evicted (any shard) and every returned POSTED / VOIDED
 *     row found its resolution.
 *   Invalid filters are never a status: account_id 2^128-1, a non-zero account_id with neither DEBITS
 *     nor CREDITS, no TBGPU_PENDING_* bit, an unknown flag bit, a non-zero reserved byte,
 *     timestamp_min, timestamp_max or now equal to 2^64-1, a non-zero timestamp_max below
 *     timestamp_min, limit 0 — each returns TBGPU_STATUS_OK with count = matched = 0.  A NULL filter,
 *     out_rows, out_states or result is TBGPU_STATUS_INVALID.  After a failing status the result names
 *     no row.
 *   The call contract of tbgpu_get_account_transfers: synchronous, drains a pending
 *     tbgpu_commit_device_async first, a read that changes nothing (commit_timestamp, balances, log,
 *     index, the posted groove, stats, the write-back snapshot), works on an engine a device panic
 *     stopped, allocates nothing after tbgpu_init, legal beside an asynchronous write-back.
 *   A node engine has the same contract: every home shard selects from its own log (a pending
 *     transfer's posted state lives on its home), the host merges the shards' rows by timestamp under
 *     the limit, and every shard then scans its own log for the merged rows' resolutions, side by side. */
#define TBGPU_PENDING_OPEN     (1u << 4)  /* unresolved, not expired at `now` */
#define TBGPU_PENDING_EXPIRED  (1u << 5)  /* unresolved, expired at `now` */
#define TBGPU_PENDING_POSTED   (1u << 6)
#define TBGPU_PENDING_VOIDED   (1u << 7)
#define TBGPU_PENDING_ROWS_MAX 4095u      /* 256 B rows in one message body: 4095*256 <= 8191*128 */

typedef struct tbgpu_pending_filter {   /* 64 bytes, little-endian, no padding */
    uint64_t account_id_lo, account_id_hi; /* 0 (both words): any account */
    uint64_t timestamp_min, timestamp_max; /* window on the PENDING record's timestamp; 0 = open */
    uint64_t now;                          /* the clock for expiry; 0 = commit_timestamp */
    uint32_t limit;
    uint32_t flags;   /* TBGPU_FILTER_DEBITS | _CREDITS | _REVERSED (same bit values) | TBGPU_PENDING_* */
    uint8_t  reserved[16];                 /* must be zero */
} tbgpu_pending_filter;

typedef struct tbgpu_pending_row {      /* 256 bytes */
    uint8_t pending[128];     /* the bytes lookup_transfers returns for the pending transfer */
    uint8_t resolution[128];  /* the post or void record that resolved it; all zero if none is resident */
} tbgpu_pending_row;

int tbgpu_get_pending_transfers(tbgpu_t* engine, const tbgpu_pending_filter* filter,
                                void* out_rows, uint8_t* out_states, uint32_t out_cap_rows,
                                tbgpu_query_result* result);

/* get_account_statements: a statement header for each account the caller names, over a period the
 * caller names — the balances at the period's start, the balances at its end, what moved in between
 * (gross debits and credits, holds placed and released) and how many transfers there were.  No
 * reference has an operation for it.  Two tbgpu_lookup_accounts_at calls give the two balances in two
 * scans and their difference only the net; this call derives all of it in one scan of the log in HBM,
 * whatever the number of ids, and stores nothing at commit.  An entry point of its own, as above;
 * this comment is its specification.
 *   The period is (t_open, t_close], so consecutive statements tile: the next t_open is this
 *     t_close.  0 leaves that end open: t_open == 0 means from before every record (read literally,
 *     not as "now"), t_close == 0 means up to now.
 *   Which rows: tbgpu_lookup_accounts_at's rules with T = t_close — one 256-byte row per requested
 *     id that its owner's account table holds, in request order.  Absent ids and the reserved ids (0,
 *     2^128-1) are skipped; a repeated id is answered once per occurrence; an account whose own
 *     timestamp is above a non-zero t_close is skipped.  `matched` is the number of ids that yield a
 *     row; count = min(matched, out_cap_rows), the first ones in request order; bytes past count rows
 *     are not written.
 *   The sums are taken over every live resident record r that names the account (liveness:
 *     tbgpu_get_account_transfers' rule), on the debit side where the account is r's debit account,
 *     on the credit side where it is r's credit account; a loaded record that names it on both counts
 *     on both.  P and the orphan rule are tbgpu_get_account_balances': a void's P is its own amount,
 *     and a post whose pending transfer is not resident uses P = its own amount and drops `complete`.
 *     A record in the period (t_open < r.timestamp, and r.timestamp <= t_close when t_close != 0)
 *     adds one to its side's debit_transfers or credit_transfers, and by kind
 *         pending      *_pending_in  += amount
 *         post         *_pending_out += P,  *_posted_in += amount
 *         void         *_pending_out += P
 *         any other    *_posted_in   += amount
 *     closing = current(a) - the effects of the records above t_close (tbgpu_lookup_accounts_at's
 *     sum; for t_close == 0 nothing is above it), and
 *         opening.x_pending = closing.x_pending - x_pending_in + x_pending_out
 *         opening.x_posted  = closing.x_posted  - x_posted_in
 *     all of it per column modulo 2^128.  So `closing` is tbgpu_lookup_accounts_at's balances at
 *     t_close, `opening` is that call's formula at t_open, and the identities hold exactly.  The
 *     anchor is the current balance: the answers stay exact after eviction of an old prefix, after
 *     tbgpu_load_accounts and after tbgpu_test_set_balances; periods that reach behind such a step
 *     follow this definition, not the ledger's past.  An account created inside the period gets its
 *     `opening` by the definition too: zero on an engine that saw none of those steps.
 *   complete: tbgpu_lookup_accounts_at's rule — 1 only when no transfer was ever evicted (any shard)
 *     and every post that entered a sum found its pending transfer resident; otherwise 0.
 *   t_open or t_close equal to 2^64-1, or a non-zero t_close below t_open, returns TBGPU_STATUS_OK
 *     with count = matched = 0.  n == 0 returns TBGPU_STATUS_OK and writes nothing.
 *     n > TBGPU_STATEMENTS_MAX, or a NULL ids, out or result with n > 0, is TBGPU_STATUS_INVALID and
 *     writes nothing.  After any failing status the result names no row.
 *   The call contract of tbgpu_get_account_transfers: synchronous, drains a pending
 *     tbgpu_commit_device_async first, a read that changes nothing (commit_timestamp, balances, log,
 *     index, posted groove, stats, the write-back snapshot), works on an engine a device panic
 *     stopped, allocates nothing after tbgpu_init, legal beside an asynchronous write-back.
 *   A node engine has the same contract: every home shard scans its own log on its own device and
 *     stream, side by side, reading a post's pending transfer on the home shard of its pending_id;
 *     each account's record, and whether it existed at t_close, come from its owner shard only; the
 *     host adds the shards' sums. */
#define TBGPU_STATEMENTS_MAX 4095u   /* 256 B rows in one message body: 4095*256 <= 8191*128 */
typedef struct tbgpu_account_statement {   /* 256 bytes, little-endian, no padding */
    uint64_t id_lo, id_hi;
    uint64_t opening[8];   /* debits_pending, debits_posted, credits_pending, credits_posted: lo, hi each */
    uint64_t closing[8];   /* likewise */
    uint64_t debits_pending_in[2],  debits_pending_out[2],  debits_posted_in[2];
    uint64_t credits_pending_in[2], credits_pending_out[2], credits_posted_in[2];
    uint64_t debit_transfers, credit_transfers;
} tbgpu_account_statement;
int tbgpu_get_account_statements(tbgpu_t* engine, uint64_t t_open, uint64_t t_close,
                                 const void* ids /* n x {lo, hi} */, uint32_t n,
                                 void* out, uint32_t out_cap_rows, tbgpu_query_result* result);

/* get_account_balance_integrals: for each account the caller names, over a period the caller names,
 * how much was held for how long — the time integral of each of the four balances over the period,
 * balance x nanoseconds, the "average daily balance" once divided by the period's length: what every
 * interest, fee and overdraft calculation starts from.  No reference has an operation for it, and
 * paging tbgpu_get_account_balances per account to integrate on the host is a log scan per account
 * per page; this call derives it in one scan of the log in HBM, whatever the number of ids, and stores
 * nothing at commit.  An entry point of its own, as above; this comment is its specification.
 *   The period is (t_open, t_end], as tbgpu_get_account_statements' is.  t_open == 0 is read
 *     literally.  t_close == 0 means t_end = tbgpu_commit_timestamp (a node: the node's own), read once
 *     at the call — an integral needs a finite end; otherwise t_end = t_close.  L = t_end - t_open.
 *     The row carries the period as used (t_open, t_end).
 *   Which rows: tbgpu_lookup_accounts_at's rules with T = t_end — one 256-byte row per requested id
 *     that its owner's account table holds, in request order.  Absent ids and the reserved ids (0,
 *     2^128-1) are skipped; a repeated id is answered once per occurrence; an account whose own
 *     timestamp is above t_end is skipped.  `matched` is the number of ids that yield a row; count =
 *     min(matched, out_cap_rows), the first ones in request order; bytes past count rows are not
 *     written.
 *   opening, closing: tbgpu_lookup_accounts_at's formula at t_open and at t_end, byte for byte
 *     tbgpu_get_account_statements' fields for the same (t_open, t_end).
 *   integral[c], for each column c of {debits_pending, debits_posted, credits_pending,
 *     credits_posted}, three words, low word first, modulo 2^192:
 *         integral[c] = the sum over t = t_open .. t_end - 1 of balance_at(a, t).c
 *     where balance_at is tbgpu_lookup_accounts_at's formula: its anchor at the current balance, its
 *     effect table, the P rule, the orphan rule and the liveness rule.  The balance is below 2^128 and
 *     L below 2^64, so the value fits and the modular result is exact.  It is computed without any
 *     order of the log, as
 *         integral[c] = opening.c * L + the sum of effect(r).c * (t_end - r.timestamp)
 *     over the live resident records r that name the account with t_open < r.timestamp <= t_end (a
 *     record at t_end weighs 0); a released hold's effect on a *_pending column is negative and enters
 *     as its two's complement modulo 2^192.  The two forms are equal wherever no balance_at in the
 *     period falls below zero; one that does — only behind a tbgpu_test_set_balances or
 *     tbgpu_load_accounts step that set a balance below what the later records move — counts as that
 *     negative number, not as its wrap modulo 2^128, while `opening` itself is the wrapped value the
 *     other calls give.  L == 0 gives zero integrals and opening == closing.  Timestamps before the
 *     account's creation follow the definition: zero on an engine that never had its balances set or
 *     loaded.  The integrals are additive: over (t0, t1] and (t1, t2] they add to (t0, t2]'s.
 *   complete: tbgpu_lookup_accounts_at's rule.
 *   t_open or t_close equal to 2^64-1, or t_end below t_open (this includes t_close == 0 with
 *     commit_timestamp < t_open), returns TBGPU_STATUS_OK with count = matched = 0.  n == 0 returns
 *     TBGPU_STATUS_OK and writes nothing.  n > TBGPU_INTEGRALS_MAX, or a NULL ids, out or result with
 *     n > 0, is TBGPU_STATUS_INVALID and writes nothing.  After any failing status the result names
 *     no row.
 *   The call contract of tbgpu_get_account_statements: synchronous, drains a pending
 *     tbgpu_commit_device_async first, a read that changes nothing, works on an engine a device panic
 *     stopped, allocates nothing after tbgpu_init, legal beside an asynchronous write-back.
 *   A node engine has the same contract: every home shard scans its own log on its own device and
 *     stream, side by side, reading a post's pending transfer on the home shard of its pending_id;
 *     each account's record, and whether it existed at t_end, come from its owner shard only; the
 *     host adds the shards' sums modulo 2^192. */
#define TBGPU_INTEGRALS_MAX 4095u            /* 256 B rows in one message body */
typedef struct tbgpu_account_balance_integral {   /* 256 bytes, little-endian, no padding */
    uint64_t id_lo, id_hi;
    uint64_t opening[8];      /* debits_pending, debits_posted, credits_pending, credits_posted: lo, hi each */
    uint64_t closing[8];      /* likewise */
    uint64_t integral[12];    /* the same four columns, three words each, low word first: balance x ns, mod 2^192 */
    uint64_t t_open, t_end;   /* the period as used: t_end is t_close, or commit_timestamp where t_close was 0 */
} tbgpu_account_balance_integral;
int tbgpu_get_account_balance_integrals(tbgpu_t* engine, uint64_t t_open, uint64_t t_close,
                                        const void* ids /* n x {lo, hi} */, uint32_t n,
                                        void* out, uint32_t out_cap_rows, tbgpu_query_result* result);

/* get_account_balance_extremes: for each account the caller names, over a period the caller names,
 * the lowest and the highest value a balance reached, and when — what overdraft detection, a
 * minimum-balance fee, the peak exposure on holds and margin or limit monitoring start from.  Every
 * other query here is a sum over the log in any order; a running balance's extremes depend on the order
 * of the records.  No reference has an operation for it, and paging tbgpu_get_account_balances per
 * account to take the minimum on the host is one or two log scans per account per page of 8,190 rows;
 * this call answers every id in one walk of the log in HBM and stores nothing at commit.  An entry
 * point of its own, as above; this comment is its specification.
 *   The value.  `measure` picks what is watched, a coefficient of -1, 0 or +1 per balance column:
 *         v(a, t) = the sum over the four columns k of measure.k * balance_at(a, t).k
 *     taken as a signed integer, where balance_at is tbgpu_lookup_accounts_at's formula word for word —
 *     its anchor at the current balance, its effect table, the P rule, the orphan rule and the liveness
 *     rule — and each column is an unsigned 128-bit value.  The TBGPU_MEASURE_* macros name the usual
 *     ones: the net posted balance of a credit-normal account {0, -1, 0, +1}, its available balance
 *     {-1, -1, 0, +1}, the same two for a debit-normal account, and each single column.
 *   The period is (t_open, t_end], as tbgpu_get_account_balance_integrals' is: t_open == 0 is read
 *     literally; t_close == 0 means t_end = tbgpu_commit_timestamp (a node: the node's own), read once
 *     at the call; otherwise t_end = t_close.  The row carries the period as used.
 *   Which rows, request order, repeated, absent and reserved ids, an account created after t_end,
 *     matched, count and complete: tbgpu_get_account_balance_integrals' rules, with 192-byte rows.
 *   opening = v(a, t_open), closing = v(a, t_end).
 *   low, high.  Let r_1 .. r_m be the live resident records that name the account with t_open <
 *     timestamp <= t_end, by timestamp, v_0 = opening and v_i = v(a, timestamp(r_i)).  low is the least
 *     v_i and t_low the timestamp of the first i that reaches it, t_open for i = 0; high and t_high
 *     likewise with the greatest.  records = m.  With m = 0, low = high = opening = closing and t_low =
 *     t_high = t_open.  A post is one step: the release of its hold and its posting land together, so
 *     a measure that adds a pending and a posted column does not dip between them.
 *   The values are exact signed integers in 192 bits, two's complement, low word first.  One record's
 *     step is below 2^130 in magnitude and a log holds fewer than 2^32 records, so no value the
 *     definition walks through can wrap 192 bits.  They are computed from the records' steps: equal to
 *     the definition wherever no balance_at column in the period falls below zero — which only a
 *     tbgpu_test_set_balances or tbgpu_load_accounts step that set a balance below what the later
 *     records release can cause; such a column counts as that negative number, as the integrals do.
 *   A coefficient outside {-1, 0, +1}, a measure that is all zero, a non-zero reserved byte, a NULL
 *     measure, ids, out or result with n > 0, or n > TBGPU_EXTREMES_MAX is TBGPU_STATUS_INVALID and
 *     writes nothing.  t_open or t_close equal to 2^64-1, or t_end below t_open, returns
 *     TBGPU_STATUS_OK with count = matched = 0.  n == 0 returns TBGPU_STATUS_OK and writes nothing.
 *     After any failing status the result names no row.
 *   The call contract of tbgpu_get_account_statements: synchronous, drains a pending
 *     tbgpu_commit_device_async first, a read that changes nothing, works on an engine a device panic
 *     stopped, allocates nothing on the device after tbgpu_init, legal beside an asynchronous write-back.
 *   Cost.  One engine whose log lies in timestamp order (every log that commits built) is answered by
 *     one ordered walk of the log, a few times the cost of tbgpu_get_account_statements.  A node
 *     engine, whose shards interleave in time, and an engine whose log tbgpu_load_transfers filled out
 *     of timestamp order are answered exactly, with the same bytes, but slowly: per found account the
 *     balance history of the period is paged internally (tbgpu_get_account_balances' scans, 8,190 rows
 *     a page) and reduced on the host — a log scan or two per account per page.  Keep n small there. */
#define TBGPU_EXTREMES_MAX 4095u
typedef struct tbgpu_balance_measure {   /* 8 bytes */
    int8_t  debits_pending, debits_posted, credits_pending, credits_posted;  /* each -1, 0 or +1 */
    uint8_t reserved[4];                                                     /* zero */
} tbgpu_balance_measure;
/* {debits_pending, debits_posted, credits_pending, credits_posted} */
#define TBGPU_MEASURE_CREDIT_NET_POSTED   { 0, -1,  0, +1, {0, 0, 0, 0}}  /* credits_posted - debits_posted */
#define TBGPU_MEASURE_CREDIT_AVAILABLE    {-1, -1,  0, +1, {0, 0, 0, 0}}  /* ... less the held debits */
#define TBGPU_MEASURE_DEBIT_NET_POSTED    { 0, +1,  0, -1, {0, 0, 0, 0}}  /* debits_posted - credits_posted */
#define TBGPU_MEASURE_DEBIT_AVAILABLE     { 0, +1, -1, -1, {0, 0, 0, 0}}  /* ... less the held credits */
#define TBGPU_MEASURE_DEBITS_PENDING      {+1,  0,  0,  0, {0, 0, 0, 0}}
#define TBGPU_MEASURE_DEBITS_POSTED       { 0, +1,  0,  0, {0, 0, 0, 0}}
#define TBGPU_MEASURE_CREDITS_PENDING     { 0,  0, +1,  0, {0, 0, 0, 0}}
#define TBGPU_MEASURE_CREDITS_POSTED      { 0,  0,  0, +1, {0, 0, 0, 0}}
typedef struct tbgpu_account_balance_extreme {   /* 192 bytes, little-endian, no padding */
    uint64_t id_lo, id_hi;
    uint64_t opening[3], closing[3];   /* the measure at t_open and at t_end: signed, two's complement, 192 bits, low word first */
    uint64_t low[3], high[3];          /* its minimum and maximum over [t_open, t_end] */
    uint64_t t_low, t_high;            /* when each was first reached */
    uint64_t records;                  /* live resident records of the period that name the account */
    uint64_t t_open, t_end;            /* the period as used */
    uint64_t measure;                  /* the request's 8 bytes, echoed */
    uint64_t reserved[4];              /* zero */
} tbgpu_account_balance_extreme;
int tbgpu_get_account_balance_extremes(tbgpu_t* engine, uint64_t t_open, uint64_t t_close,
                                       const tbgpu_balance_measure* measure,
                                       const void* ids /* n x {lo, hi} */, uint32_t n,
                                       void* out, uint32_t out_cap_rows, tbgpu_query_result* result);

/* get_account_statement_series: tbgpu_get_account_statements cut into consecutive periods — for each
 * account the caller names, one statement row per bucket: daily closing balances for a month, monthly
 * turnover for a year, the day-by-day ledger an interest run walks.  One scan of the log in HBM
 * answers every bucket of every account, where the single call would scan once per bucket.  Each row
 * is the row the single call would have written.  An entry point of its own, as above; this comment
 * is its specification.
 *   Buckets: bounds holds n_buckets + 1 timestamps, and bucket k is the period
 *     (bounds[k], bounds[k+1]], so buckets tile exactly as consecutive statements do.  bounds[0] == 0
 *     is read literally (from before every record); bounds[n_buckets] == 0 leaves the last bucket
 *     open-ended, as t_close == 0 does; bounds[1 .. n_buckets-1] must be non-zero.  Bounds are
 *     non-decreasing; equal neighbours make an empty bucket, which is legal, as t_open == t_close is
 *     for the single call.  A record with timestamp ts belongs to the smallest k with
 *     ts <= bounds[k+1]; a record at or below bounds[0] belongs to none; a record above a non-zero
 *     last bound belongs to the tail, the effects "above t_close".
 *   Which accounts: tbgpu_lookup_accounts_at's rules with T = the last bound, or no limit when the
 *     last bound is 0 — an account counts when its owner's table holds it and its own timestamp is
 *     not above T.  Answers are in request order; absent ids and the reserved ids are skipped; a
 *     repeated id is answered once per occurrence.
 *   Rows: tbgpu_account_statement, unchanged.  Each such account yields exactly n_buckets rows,
 *     contiguous, bucket ascending: found account r's bucket k is row r * n_buckets + k.  `matched` is
 *     found accounts x n_buckets; count = min(matched, out_cap_rows): the cap cuts in that row order
 *     and may cut inside an account.  Bytes past count rows are not written.
 *   What a row holds: row (a, k) is byte for byte the row
 *     tbgpu_get_account_statements(bounds[k], bounds[k+1], {a}) writes, wherever that call yields a
 *     row.  Where the single call would skip `a` because its creation timestamp is above bounds[k+1]
 *     (it is still at or below the last bound), the row is present and holds the same formula's
 *     values: zeros on an engine that never had balances set or loaded — it follows the definition,
 *     not the ledger's past.  By construction the closing of bucket k is the opening of bucket k+1,
 *     the last bucket's closing is tbgpu_lookup_accounts_at at the last bound, and the sums and
 *     counts over all buckets equal the single call's over (bounds[0], bounds[n_buckets]].
 *   complete: tbgpu_lookup_accounts_at's rule over everything above bounds[0] — one value for the
 *     whole answer.  It may be 0 where a single narrow call would say 1: an orphan post in another
 *     bucket, or in the tail, drops it for every row.
 *   Any bound equal to 2^64-1, a zero among bounds[1 .. n_buckets-1], or a bound below its
 *     predecessor (except an open last bound of 0) returns TBGPU_STATUS_OK with count = matched = 0
 *     and writes nothing.  n == 0 returns TBGPU_STATUS_OK and writes nothing.  n_buckets == 0,
 *     n * n_buckets > TBGPU_SERIES_ROWS_MAX, NULL bounds, or a NULL ids, out or result with n > 0, is
 *     TBGPU_STATUS_INVALID and writes nothing.  After any failing status the result names no row.
 *   With n_buckets == 1 the answer is byte-identical to
 *     tbgpu_get_account_statements(bounds[0], bounds[1], ids, ...), `matched` and `complete` included.
 *   The call contract of tbgpu_get_account_statements: synchronous, drains a pending
 *     tbgpu_commit_device_async first, a read that changes nothing, works on an engine a device panic
 *     stopped, allocates nothing after tbgpu_init, legal beside an asynchronous write-back.
 *   A node engine has the same contract: every home shard scans its own log on its own device and
 *     stream, side by side, reading a post's pending transfer on the home shard of its pending_id;
 *     each account's record, and whether it existed at the last bound, come from its owner shard
 *     only; the host adds the shards' sums and builds the rows by the device's row function. */
#define TBGPU_SERIES_ROWS_MAX 4095u   /* 256 B rows in one message body */
int tbgpu_get_account_statement_series(tbgpu_t* engine,
        const uint64_t* bounds /* n_buckets + 1 */, uint32_t n_buckets,
        const void* ids /* n x {lo, hi} */, uint32_t n,
        void* out, uint32_t out_cap_rows, tbgpu_query_result* result);

/* get_account_flow_matrix: who paid whom — for a list of debit accounts and a list of credit accounts
 * the caller names, over a period the caller names, what each debit account d paid each credit
 * account c: one cell per pair.  It is what bilateral and multilateral netting, "this merchant's
 * payers" and "what this bank owes each correspondent" start from.  Every other read call here answers
 * for an account on its own; paging tbgpu_get_account_transfers per account and grouping on the host is
 * a log scan per account per page, and tbgpu_query_transfers has no account-pair filter.  This call
 * derives the whole matrix in one scan of the log in HBM, whatever the number of pairs, and stores
 * nothing at commit.  No reference has an operation for it.  An entry point of its own, as above; this
 * comment is its specification.
 *   The period is (t_open, t_close], exactly tbgpu_get_account_statements': t_open == 0 is read
 *     literally (from before every record), t_close == 0 means up to now.
 *   Which accounts: tbgpu_lookup_accounts_at's rules with T = t_close, applied to each list on its
 *     own — a position counts (is "found") when its owner's account table holds the id and the
 *     account's own timestamp is not above a non-zero t_close.  Absent ids and the reserved ids (0,
 *     2^128-1) are skipped; a repeated id is answered once per occurrence; an id may stand in both
 *     lists (for netting the two lists are the same).
 *   Rows: dense and row-major.  The found debit position of rank r (among the found debit positions,
 *     in request order) and the found credit position of rank q give cell r * found_credit + q.
 *     matched = found_debit * found_credit; count = min(matched, out_cap_cells): the cap cuts in that
 *     order and may cut inside a debit row.  Bytes past count cells are not written.  A cell with no
 *     record is present, and zero apart from its two ids.
 *   A cell (d, c) sums over every live resident record r (liveness: tbgpu_get_account_transfers'
 *     rule) whose debit account is d and whose credit account is c, with t_open < r.timestamp, and
 *     r.timestamp <= t_close when t_close != 0.  Post and void records count too: the log holds them
 *     with their accounts filled in.  Each adds one to `transfers`, and by kind
 *         pending      pending_in  += amount
 *         post         pending_out += P,  posted += amount
 *         void         pending_out += P
 *         any other    posted      += amount
 *     modulo 2^128.  P and the orphan rule are tbgpu_get_account_balances': a void's P is its own
 *     amount, and a post whose pending transfer is not resident uses P = its own amount.  The
 *     direction matters: a record from c to d belongs to cell (c, d), and only where c is a found
 *     debit position and d a found credit position.  A loaded record with d == c belongs to cell
 *     (d, d), once.  With both lists the same, a debit row's sums are that account's debits_* fields
 *     of tbgpu_get_account_statements less what it paid accounts outside the lists, and a credit
 *     column's its credits_* fields likewise.
 *   complete: 0 when any transfer was ever evicted (any shard), or when an orphan post entered a cell
 *     of the matrix, whether or not that cell lies under the cap; 1 otherwise.  An orphan post outside
 *     the period, or with a side that was not asked for, does not drop it: narrower than
 *     tbgpu_get_account_statements' rule, which also sums what lies above t_close and every record
 *     that names one requested account.
 *   t_open or t_close equal to 2^64-1, or a non-zero t_close below t_open, returns TBGPU_STATUS_OK
 *     with count = matched = 0.  n_debit == 0 or n_credit == 0 returns TBGPU_STATUS_OK and writes
 *     nothing.  n_debit * n_credit > TBGPU_FLOW_MATRIX_CELLS_MAX (computed in 64 bits), or a NULL
 *     debit_ids, credit_ids, out or result while both counts are non-zero, is TBGPU_STATUS_INVALID and
 *     writes nothing.  After any failing status the result names no cell.
 *   The call contract of tbgpu_get_account_statements: synchronous, drains a pending
 *     tbgpu_commit_device_async first, a read that changes nothing, works on an engine a device panic
 *     stopped, allocates nothing after tbgpu_init, legal beside an asynchronous write-back.
 *   A node engine has the same contract: every home shard scans its own log on its own device and
 *     stream, side by side, reading a post's pending transfer on the home shard of its pending_id;
 *     whether an account existed at t_close comes from its owner shard only; the host adds the shards'
 *     sums and builds the cells by the device's cell function. */
#define TBGPU_FLOW_MATRIX_CELLS_MAX 4095u   /* n_debit * n_credit; 96 B cells in one message body */
typedef struct tbgpu_flow_cell {            /* 96 bytes, little-endian, no padding */
    uint64_t debit_id_lo, debit_id_hi;
    uint64_t credit_id_lo, credit_id_hi;
    uint64_t posted[2];                     /* amounts posted d -> c: single-phase transfers and posts */
    uint64_t pending_in[2];                 /* holds placed d -> c */
    uint64_t pending_out[2];                /* holds released d -> c: P of posts and voids */
    uint64_t transfers;                     /* records of the period that name d as debit and c as credit */
    uint64_t reserved;                      /* zero */
} tbgpu_flow_cell;
int tbgpu_get_account_flow_matrix(tbgpu_t* engine, uint64_t t_open, uint64_t t_close,
        const void* debit_ids /* n_debit x {lo, hi} */, uint32_t n_debit,
        const void* credit_ids /* n_credit x {lo, hi} */, uint32_t n_credit,
        void* out, uint32_t out_cap_cells, tbgpu_query_result* result);

/* get_account_counterparties: who an account dealt with — for one subject account a and a period, one
 * row per distinct account x that a paid or was paid by, with what went each way.  Every other read
 * call here answers for accounts the caller already names (the flow matrix fills cells only for the
 * payers it is given); this one discovers them: "who pays this merchant, and how much", "whom did this
 * account pay last month", "the ten largest counterparties of this bank".  Paging
 * tbgpu_get_account_transfers for the account and grouping on the host is one log scan per page; this
 * call groups by the 128-bit counterparty id in one scan of the log in HBM and stores nothing at
 * commit.  No reference has an operation for it.  An entry point of its own, as above; this comment is
 * its specification.
 *   The period is (t_open, t_close], exactly tbgpu_get_account_statements': t_open == 0 is read
 *     literally (from before every record), t_close == 0 means up to now.
 *   What matches: a live resident record r (liveness: tbgpu_get_account_transfers' rule) with
 *     t_open < r.timestamp, and r.timestamp <= t_close when t_close != 0, that names a on a wanted
 *     side.  TBGPU_FILTER_DEBITS wants the records whose debit account is a: each feeds `to` of the
 *     row of its credit account.  TBGPU_FILTER_CREDITS wants the records whose credit account is a:
 *     each feeds `from` of the row of its debit account.  Post and void records count too, as in the
 *     flow matrix.  A record adds one to `transfers`, and by kind
 *         pending      pending_in  += amount
 *         post         pending_out += P,  posted += amount
 *         void         pending_out += P
 *         any other    posted      += amount
 *     modulo 2^128, exactly as a tbgpu_flow_cell; P and the orphan rule are
 *     tbgpu_get_account_balances' (a void's P is its own amount; a post whose pending transfer is not
 *     resident uses P = its own amount).  A loaded record with debit == credit == a belongs to row a:
 *     it enters `to` when DEBITS is wanted and `from` when CREDITS is wanted.  The half of a side that
 *     is not wanted is all zero.
 *   No account table is read: the subject and the counterparties are ids as the records carry them.
 *     A subject no record names gives no rows; a counterparty need not be in the account table; on a
 *     node engine nothing depends on account owners.
 *   A group is a distinct counterparty id x >= id_min (as 128-bit numbers; id_min 0: all) with at
 *     least one matching record.  matched is the number of groups.
 *   Order: by default by x ascending as a 128-bit number; a consumer pages with id_min = the last
 *     id + 1.  Under TBGPU_COUNTERPARTIES_BY_VOLUME by volume = (to.posted + from.posted) mod 2^128,
 *     descending, equal volumes by x ascending; that order has no cursor, id_min still narrows the
 *     groups.
 *   Rows: count = min(limit, out_cap_rows, TBGPU_COUNTERPARTIES_ROWS_MAX, matched) rows, the first in
 *     that order.  Bytes past count rows are not written.
 *   complete: 0 when any transfer was ever evicted (any shard), or when an orphan post matched —
 *     whether or not its group is returned, and whether or not its counterparty is at or above
 *     id_min; 1 otherwise.  An orphan post outside the period or on a side that is not wanted does
 *     not drop it.
 *   Identities.  For a returned x that the account table holds with a timestamp at or below a
 *     non-zero t_close, `to` is byte for byte the seven sum words {posted, pending_in, pending_out,
 *     transfers} of tbgpu_get_account_flow_matrix's cell (a, x) for the same period, and `from` those
 *     of cell (x, a).  With id_min 0 and DEBITS, the sums of `to` over every group are a's
 *     debits_pending_in, debits_pending_out, debits_posted_in and debit_transfers of
 *     tbgpu_get_account_statements; `from` and CREDITS give the credits_* fields likewise.
 *   An invalid filter is never a status: an account_id of 0 or 2^128-1, neither side bit, an unknown
 *     flag bit (TBGPU_FILTER_REVERSED included), a non-zero reserved byte, t_open or t_close equal to
 *     2^64-1, a non-zero t_close below t_open, or limit 0 return TBGPU_STATUS_OK with
 *     count = matched = 0 and write nothing.  A NULL filter, out or result is TBGPU_STATUS_INVALID.
 *     After any failing status the result names no row.
 *   Capacity: an engine has room for at least accounts_max groups (a node engine: the node's
 *     accounts_max).  Committed records name only accounts the table holds, so a committed log never
 *     exceeds it.  A log built with tbgpu_load_transfers whose matching records name more distinct
 *     counterparties than the engine has room for returns TBGPU_STATUS_INVALID, tbgpu_last_error
 *     names the capacity, and nothing is written: never a partial answer.
 *   The call contract of tbgpu_get_account_statements: synchronous, drains a pending
 *     tbgpu_commit_device_async first, a read that changes nothing, works on an engine a device panic
 *     stopped, allocates nothing after tbgpu_init, legal beside an asynchronous write-back.
 *   A node engine returns the same bytes: every home shard scans its own log on its own device and
 *     stream, side by side; a group's sums are the shards' sums added before the order is applied (a
 *     counterparty's volume rank is a property of its total, not of any shard's part). */
#define TBGPU_COUNTERPARTIES_BY_VOLUME (1u << 8)   /* order by volume descending; default: by id ascending */
#define TBGPU_COUNTERPARTIES_ROWS_MAX 8191u        /* 128 B rows in one message body */
typedef struct tbgpu_counterparty_filter {  /* 64 bytes, little-endian, no padding */
    uint64_t account_id_lo, account_id_hi;  /* the subject account a */
    uint64_t t_open, t_close;               /* the period (t_open, t_close] */
    uint64_t id_min_lo, id_min_hi;          /* only counterparties with id >= id_min; 0: all */
    uint32_t limit;
    uint32_t flags;  /* TBGPU_FILTER_DEBITS | TBGPU_FILTER_CREDITS | TBGPU_COUNTERPARTIES_BY_VOLUME */
    uint8_t  reserved[8];                   /* must be zero */
} tbgpu_counterparty_filter;
typedef struct tbgpu_counterparty_flow {    /* 56 bytes: a tbgpu_flow_cell without its ids and reserved word */
    uint64_t posted[2], pending_in[2], pending_out[2];
    uint64_t transfers;
} tbgpu_counterparty_flow;
typedef struct tbgpu_counterparty {         /* 128 bytes */
    uint64_t id_lo, id_hi;                  /* the counterparty x */
    tbgpu_counterparty_flow to;             /* a -> x: records whose debit account is a and credit account is x */
    tbgpu_counterparty_flow from;           /* x -> a */
} tbgpu_counterparty;
int tbgpu_get_account_counterparties(tbgpu_t* engine, const tbgpu_counterparty_filter* filter,
                                     void* out, uint32_t out_cap_rows, tbgpu_query_result* result);

/* get_active_accounts: the accounts a period's records name, ranked — one row per distinct account x
 * that a record of the period (t_open, t_close] names, with what x paid (`debits`) and what it was
 * paid (`credits`).  Every other read call answers for accounts the caller names, and
 * tbgpu_get_account_counterparties discovers accounts only around one subject; this one answers
 * "which accounts moved money in the last hour", "which ten moved the most", "which accounts on ledger
 * 7 had the most transfers under code 12 yesterday".  Paging the whole log out with
 * tbgpu_query_transfers and grouping on the host is one log scan per 8,190 records; this call groups by
 * the 128-bit account id in one scan of the log in HBM and stores nothing at commit.  No reference has
 * an operation for it.  An entry point of its own, as above; this comment is its specification.
 *   The period is (t_open, t_close], exactly tbgpu_get_account_statements': t_open == 0 is read
 *     literally (from before every record), t_close == 0 means up to now.
 *   What matches: a live resident record r (liveness: tbgpu_get_account_transfers' rule) with
 *     t_open < r.timestamp, and r.timestamp <= t_close when t_close != 0, and r.ledger == ledger when
 *     ledger != 0, and r.code == code when code != 0.  Ledger and code are read as the record carries
 *     them.  Post and void records count too, as in the flow matrix.
 *   Sides and sums: under TBGPU_FILTER_DEBITS a matching record feeds `debits` of the row of its debit
 *     account; under TBGPU_FILTER_CREDITS it feeds `credits` of the row of its credit account.  A
 *     loaded record with debit == credit feeds both halves of one row.  The half of a side that is not
 *     wanted is all zero.  A record adds one to `transfers`, and by kind
 *         pending      pending_in  += amount
 *         post         pending_out += P,  posted += amount
 *         void         pending_out += P
 *         any other    posted      += amount
 *     modulo 2^128, exactly as a tbgpu_flow_cell; P and the orphan rule are
 *     tbgpu_get_account_balances' (a void's P is its own amount; a post whose pending transfer is not
 *     resident uses P = its own amount).
 *   No account table is read: accounts are ids as the records carry them, an account need not be in
 *     the account table, and on a node engine nothing depends on account owners.
 *   A group is a distinct id x >= id_min (as 128-bit numbers; id_min 0: all) with at least one
 *     matching record on a wanted side.  matched is the number of groups.
 *   Order: by default by x ascending as a 128-bit number; a consumer pages with id_min = the last
 *     id + 1.  Under TBGPU_ACTIVE_BY_VOLUME by volume = (debits.posted + credits.posted) mod 2^128,
 *     descending, equal volumes by x ascending.  Under TBGPU_ACTIVE_BY_TRANSFERS by
 *     debits.transfers + credits.transfers descending, equal counts by x ascending.  The last two have
 *     no cursor; id_min still narrows the groups.
 *   Rows: count = min(limit, out_cap_rows, TBGPU_ACTIVE_ROWS_MAX, matched) rows, the first in that
 *     order.  Bytes past count rows are not written.
 *   complete: 0 when any transfer was ever evicted (any shard), or when an orphan post matched —
 *     whether or not its groups are returned, and whether or not they are at or above id_min; 1
 *     otherwise.  A post outside the period, or failing the ledger or code test, does not drop it.
 *   Identities, with ledger == code == 0 and both sides wanted.  Statement identity: for a returned x
 *     that the account table holds with a timestamp at or below a non-zero t_close, `debits` is
 *     {debits_posted_in, debits_pending_in, debits_pending_out, debit_transfers} of
 *     tbgpu_get_account_statements for x and the same period, and `credits` the credits_* fields.
 *     Counterparty identity: the same `debits` is the sum of `to` over
 *     tbgpu_get_account_counterparties(x, TBGPU_FILTER_DEBITS).  Double entry: with every group
 *     returned, the four sums of `debits` over all rows equal those of `credits`, modulo 2^128 and
 *     2^64.  Ledger identity: on a committed log a transfer carries its accounts' ledger, so the rows
 *     under ledger = L are exactly the unfiltered rows of the accounts whose ledger is L.
 *   An invalid filter is never a status: neither side bit, both BY_* bits, an unknown flag bit
 *     (TBGPU_FILTER_REVERSED included), a non-zero reserved byte, t_open or t_close equal to 2^64-1, a
 *     non-zero t_close below t_open, or limit 0 return TBGPU_STATUS_OK with count = matched = 0 and
 *     write nothing.  A NULL filter, out or result is TBGPU_STATUS_INVALID.  After any failing status
 *     the result names no row.
 *   Capacity: an engine has room for at least accounts_max groups (a node engine: the node's
 *     accounts_max).  Committed records name only accounts the table holds, so a committed log never
 *     exceeds it.  A log built with tbgpu_load_transfers whose matching records name more distinct
 *     accounts than the engine has room for returns TBGPU_STATUS_INVALID, tbgpu_last_error names the
 *     capacity, and nothing is written: never a partial answer.
 *   The call contract of tbgpu_get_account_statements: synchronous, drains a pending
 *     tbgpu_commit_device_async first, a read that changes nothing, works on an engine a device panic
 *     stopped, allocates nothing after tbgpu_init, legal beside an asynchronous write-back.
 *   A node engine returns the same bytes: every home shard scans its own log on its own device and
 *     stream, side by side; a group's sums are the shards' sums added before any order is applied. */
#define TBGPU_ACTIVE_BY_VOLUME    (1u << 8)   /* order by volume descending */
#define TBGPU_ACTIVE_BY_TRANSFERS (1u << 9)   /* order by record count descending */
#define TBGPU_ACTIVE_ROWS_MAX 8191u           /* 128 B rows in one message body */
typedef struct tbgpu_activity_filter {   /* 64 bytes, little-endian, no padding */
    uint64_t t_open, t_close;            /* the period (t_open, t_close] */
    uint64_t id_min_lo, id_min_hi;       /* only accounts with id >= id_min; 0: all */
    uint32_t ledger;                     /* 0: any */
    uint16_t code;                       /* 0: any */
    uint8_t  reserved0[2];               /* must be zero */
    uint32_t limit;
    uint32_t flags;   /* TBGPU_FILTER_DEBITS | TBGPU_FILTER_CREDITS | one TBGPU_ACTIVE_BY_* at most */
    uint8_t  reserved[16];               /* must be zero */
} tbgpu_activity_filter;
typedef struct tbgpu_account_activity {  /* 128 bytes */
    uint64_t id_lo, id_hi;               /* the account x */
    tbgpu_counterparty_flow debits;      /* records whose debit account is x */
    tbgpu_counterparty_flow credits;     /* records whose credit account is x */
} tbgpu_account_activity;
int tbgpu_get_active_accounts(tbgpu_t* engine, const tbgpu_activity_filter* filter,
                              void* out, uint32_t out_cap_rows, tbgpu_query_result* result);

/* The replica writes StateMachine.commit_timestamp itself: the header timestamp after every commit
 * (src/vsr/replica.zig:3664-3665) and the checkpoint's value on open / state sync.  The wrapper
 * pushes a changed value here before the next commit, so the engine asserts what the reference
 * asserts (timestamp > commit_timestamp, src/state_machine.zig:519). */
int tbgpu_set_commit_timestamp(tbgpu_t* engine, uint64_t timestamp);

typedef struct tbgpu_stats {
    uint64_t passes;
    uint64_t events;
    uint64_t dependent_events;   /* events replayed by the ordered fallback kernel */
    uint64_t accounts;           /* live accounts */
    uint64_t transfers;          /* live transfers */
    /* With TBGPU_CONFIG_PROFILE: total device ms and launch count per kernel. */
    double ms_validate;          /* tb_transfers_validate / tb_accounts_validate */
    double ms_resolve;           /* tb_*_resolve (classify + chains + apply + replies) */
    double ms_replay;            /* tb_replay (ordered fallback) */
    double ms_clear;             /* dedup table clears */
    uint64_t launches_validate, launches_resolve, launches_replay, launches_clear;
    double ms_apply;             /* tb_apply_legs (per-account sums of the balance legs) */
    uint64_t launches_apply;
    uint64_t flow_passes;        /* passes whose dependent events ran on the parallel flow path */
    uint64_t flow_units;         /* chains / single dependent events the flow path executed */
    uint64_t flow_runs;          /* runs: single-resource sequences walked with the balance in registers */
    uint64_t flow_run_units;     /* units covered by runs */
    double flow_plan_ms;         /* tb_flow wall time planning the dependent events (workgroup 0) */
    double flow_run_ms;          /* tb_flow wall time executing them in order (workgroup 0) */
    uint64_t bounds_passes;      /* passes whose limit checks were all decided by bounds scans (no ordered run) */
    uint64_t bounds_units;       /* dependent events they decided */
    uint64_t bounds_rounds;      /* scan rounds they took (and those of abandoned attempts) */
    uint64_t bounds_skipped;     /* dependent passes with an event the bounds do not cover */
    uint64_t bounds_abandoned;   /* passes whose bounds did not converge (ordered run instead) */
    uint64_t bounds_swept;       /* units decided by the in-order sweep after the rounds */
    double sweep_ms;             /* tb_flow wall time of the sweeps (one wave) */
    double sweep_loop_ms;        /* ... of it resolving windows in order */
    double sweep_wait_ms;        /* ... of it waiting for memory between windows */
    uint64_t sweep_u64_passes;   /* sweeps in the u64 X/Y form (bound + S >= 2^63: no signed slack) */
    double flow_exec_ms;         /* tb_flow run: time lanes spent executing units, summed over lanes */
    double flow_phase_ms[8];     /* tb_flow wall time by phase: plan, sort, link, bounds setup, bounds
                                    rounds, sweep, run (or applying the bounds), replies */
    /* The sweep's per-account walkers (k_flow.h fl_walk): segments walked, heavy segments (a wave
     * each); over the heavy walkers: positions, windows, stops at a partner's open unit, blocked
     * returns, blocked ms (summed over walkers), and the longest segment (positions). */
    uint64_t walk_segments, walk_heavy, walk_heavy_positions, walk_heavy_windows, walk_heavy_stops,
        walk_heavy_blocks;
    double walk_heavy_blocked_ms;
    uint64_t walk_longest;
    /* The critical walker (the longest segment's, a wave each): windows, waits at a partner's open
     * unit, ms spent waiting, ms in all (summed over passes). */
    uint64_t walk_crit_windows, walk_crit_blocks;
    double walk_crit_wait_ms, walk_crit_ms;
    uint64_t walk_dbg[4]; /* diagnostics: a stalled walker's kind | segment, unit, status, verdict bits */
    /* With TBGPU_CONFIG_PROFILE, the device clock of the launch itself (s_memrealtime): from the
     * first workgroup's start to the last workgroup's end, summed over launches, for validate,
     * resolve and apply (the HIP-event times above also hold the dispatch of each launch). */
    double span_ms[3];
    uint64_t span_launches[3];
    /* Node engines: create_transfers passes routed whole (clean), split (the dependent subsequence
     * committed by the sequencer, the rest routed), or sequenced whole (no overflow certificate);
     * events the sequencer committed. */
    uint64_t node_passes_clean, node_passes_split, node_passes_whole, node_sequenced_events;
    /* HBM bytes of the account table (hot records, balances, cold fields, marks): this engine's; on a
     * node engine the largest shard's, and each shard's in node_shard_account_bytes — the accounts it
     * owns (1/N of the ledger) plus an import room for foreign accounts' hot records (the ledger's
     * accounts, or two per event of a routed sub-pass when that is fewer). */
    uint64_t account_table_bytes;
    uint64_t node_shard_account_bytes[16];
    /* Bounded residency (tbgpu_evict_transfers): transfers evicted so far, transfer-log positions in
     * use and in all (a wrapper evicts when the log fills; a node: the sums over its shards, log_used
     * the fullest shard's fill times the node's capacity). */
    uint64_t transfers_evicted, log_used, log_capacity;
    /* Asynchronous write-backs started (tbgpu_checkpoint_delta_async), and of them those whose
     * copy-out was sent at its bounds from the first commit after it (a write-back every few ops;
     * the bytes past the counts land in the caller's buffers unread); since tbgpu_init. */
    uint64_t write_backs_async, write_backs_bound;
} tbgpu_stats;

int tbgpu_get_stats(tbgpu_t* engine, tbgpu_stats* stats);
void tbgpu_reset_stats(tbgpu_t* engine);

/* vsr.checksum (src/vsr/checksum.zig:50-74): Aegis-128L MAC, zero key and nonce, 16 tag bytes
 * (the u128 in little-endian order).  Host-only (touches no device): the AOF reader verifies
 * header and body checksums with it (src/aof.zig:214-218, src/vsr.zig:405-437). */
void tbgpu_checksum(const void* data, uint64_t len, uint8_t out[16]);

/* Last error message (thread-local, static storage). */
const char* tbgpu_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
