// k_ledgers.h — get_ledger_balances (include/tbgpu.h tbgpu_get_ledger_balances): a trial balance per
// ledger, as of a timestamp T the caller names.
//
// Nothing is stored at commit: the account table holds every account's ledger and current balances and
// every log record carries its own ledger (the low half of the word that also holds its flags), so
//   column(L, T) = the sum of current(a).column over the live accounts a of ledger L
//                  - the effects of every live resident record of ledger L with a timestamp above T,
// per column modulo 2^128 (k_balances.h's effect rule and P rule, k_query.h's liveness probe).  A
// committed record's two accounts share the record's ledger, so the log scan looks up no account: the
// record's effect {pend, post} is the same on the debit and the credit side and is summed once.
//   tb_ledger_accounts  a pass over the account table: a live slot this engine owns probes the ledger
//                       set and adds its four balances, and 1 to `accounts` when it existed at T;
//   tb_ledger_effects   a pass over the log, only when T != 0: the timestamp alone first (a wave with
//                       nothing newer than T reads nothing else), then the ledger against the set, the
//                       liveness probe, a post's pending amount, the effect.
// The host (query.h) subtracts the second from the first and writes the rows, one engine's or the sum
// of a node's shards'.
// The set is an open-addressing table of the requested ledgers themselves (0: empty — no account and
// no record carries ledger 0), built on the host, at least twice as many slots as requested positions;
// a ledger's bin is its slot, so the set holds nothing else.  A requested 0 asks for every ledger together: one
// more bin, behind the set's, that takes every live owned account and every live newer record.
// Both scans combine before any atomic.  The common table has one ledger, so all 64 lanes of a wave
// hit one bin: the lanes that share a bin are chained and summed by pointer jumping
// (k_account_scan.h's tb_scan_combine), the every-ledger share by a butterfly (tb_wave_sum128) carried in registers
// across the workgroup's tiles; the chains' first lanes add into LDS bins claimed at first use
// (tb_change_bin_claim), and the workgroup hands each LDS bin it touched to HBM once, at its end
// (tb_atomic_add128).  Sizes: 512 threads; 16 tiles (8,192 records) a workgroup of the log scan, as
// tb_change_effects; 4 tiles (2,048 slots) a workgroup of the table scan, so that a million-account
// table still gives every CU several workgroups.  LDS at 1,024 ledgers: 8 KB of set, 256 claimed bins of
// 80 B (table scan) or 32 B (log scan) and their tags, under 30 KB — two workgroups a CU within 64 KB.
// Plain launches: no grid barrier, no spin, no wait on another workgroup; every loop is bounded by
// the workgroup's tiles, the set's slots or the 64 lanes of a wave.
#pragma once

#include "k_change_events.h"

#define LEDGERS_MAX 1024u  // TBGPU_LEDGERS_MAX
#define LEDGER_SET_SLOTS_MIN 64u
#define LEDGER_SET_SLOTS_MAX (2 * LEDGERS_MAX)
#define LEDGER_THREADS 512
#define LEDGER_LOG_TILES 16
#define LEDGER_TABLE_TILES 4
#define LEDGER_LDS_BINS 256u
// A bin in HBM, 16 words: [0, 8) the accounts' four sums {debits_pending, debits_posted,
// credits_pending, credits_posted}, low word first; [8] the accounts that existed at T; [10, 14) the
// newer records' {pend, post}.  Bins [0, slots) are the set's, bin `slots` is every ledger together,
// and the slot behind it holds the flag words (CHANGE_FLAG_ORPHAN).
#define LEDGER_BIN_WORDS 16
#define LEDGER_BIN_COUNT 8
#define LEDGER_BIN_EFFECTS 10
#define LEDGER_BINS(slots) ((u64)(slots) + 2)
// A workgroup's LDS bin: the table scan's four sums and count, the log scan's two sums.
#define LEDGER_TABLE_WORDS 10
#define LEDGER_LOG_WORDS 4

__host__ static inline u32 tb_ledger_set_slots(u32 ledgers) {
    u32 s = LEDGER_SET_SLOTS_MIN;
    while (s < 2 * ledgers) s <<= 1;
    return s;
}
__host__ __device__ static inline u32 tb_ledger_hash(u32 ledger) { return (u32)(tb_mix64(ledger) >> 32); }

// The slot of `ledger` in the set, or CHANGE_NONE.  At most half the slots are taken: an empty one ends
// the probe.
__host__ __device__ static inline u32 tb_ledger_probe(const u32* set, u32 mask, u32 ledger) {
    u32 s = tb_ledger_hash(ledger) & mask;
    for (u32 i = 0; i <= mask; i++) {
        const u32 e = set[s];
        if (e == ledger) return s;
        if (e == 0) return CHANGE_NONE;
        s = (s + 1) & mask;
    }
    return CHANGE_NONE;
}

// The host's insert: the slot that holds `ledger` afterwards (a ledger already there keeps its slot).
__host__ static inline u32 tb_ledger_insert(u32* set, u32 mask, u32 ledger) {
    u32 s = tb_ledger_hash(ledger) & mask;
    while (set[s] != 0 && set[s] != ledger) s = (s + 1) & mask;
    set[s] = ledger;
    return s;
}

// A chain's first lane adds its sums: into the workgroup's LDS bin of `my` where it has or gets one,
// else straight into the bin in HBM (`dst`: its first word of this scan's part; the count, if any,
// NV * 2 words on in LDS and at `dst_count` in HBM).
template <u32 NV, u32 WORDS>
__device__ static inline void tb_ledger_add(u32* s_tags, u64* s_bins, u32 my, const u128 (&v)[NV], u32 count, u64* dst,
                                            u64* dst_count) {
    const u32 at = tb_change_bin_claim(s_tags, LEDGER_LDS_BINS, my);
    if (at != CHANGE_NONE) {
        dst = s_bins + at * WORDS;
        dst_count = dst + 2 * NV;
    }
#pragma unroll
    for (u32 c = 0; c < NV; c++) tb_atomic_add128(dst + 2 * c, v[c]);
    if (count) atomicAdd((unsigned long long*)dst_count, (unsigned long long)count);
}

// Dynamic LDS of both scans: the set's mask + 1 entries, LEDGER_LDS_BINS + 1 bins of WORDS words (the
// last one the every-ledger bin), the claimed bins' tags.
__host__ static inline size_t tb_ledger_lds_bytes(u32 slots, u32 words) {
    return (size_t)slots * 4 + (size_t)(LEDGER_LDS_BINS + 1) * words * 8 + (size_t)LEDGER_LDS_BINS * 4;
}

// T: the scanned engine's tables, cap slots; it answers for the accounts it owns under `world`
// (tb_ledger_summary's test; a single engine: world = 1, every id's home is 0).  set: mask + 1 entries;
// all: 1 when ledger 0 was asked; bins: LEDGER_BINS(mask + 1) bins, zeroed on the stream before the
// launch.  Workgroup b scans tiles [b, b + 1) * LEDGER_TABLE_TILES of LEDGER_THREADS slots.
__global__ __launch_bounds__(LEDGER_THREADS) void tb_ledger_accounts(Tables T, u64 cap, u32 world, u32 self, u64 t_at,
                                                                      const u32* set, u32 mask, u32 all, u64* bins) {
    extern __shared__ __attribute__((aligned(16))) u8 s_lds[];
    u32* s_set = (u32*)s_lds;
    u64* s_bins = (u64*)(s_set + mask + 1);
    u64* s_all = s_bins + LEDGER_LDS_BINS * LEDGER_TABLE_WORDS;
    u32* s_tags = (u32*)(s_all + LEDGER_TABLE_WORDS);
    const u32 lane = threadIdx.x & 63;
    for (u32 i = threadIdx.x; i <= mask; i += LEDGER_THREADS) s_set[i] = set[i];
    for (u32 i = threadIdx.x; i < (LEDGER_LDS_BINS + 1) * LEDGER_TABLE_WORDS; i += LEDGER_THREADS) s_bins[i] = 0;
    for (u32 i = threadIdx.x; i < LEDGER_LDS_BINS; i += LEDGER_THREADS) s_tags[i] = CHANGE_NONE;
    __syncthreads();
    u128 held[4] = {0, 0, 0, 0};  // the wave's every-ledger share: the same in every lane
    u32 held_count = 0;
    for (u32 t = 0; t < LEDGER_TABLE_TILES; t++) {
        const u64 tile0 = ((u64)blockIdx.x * LEDGER_TABLE_TILES + t) * LEDGER_THREADS, slot = tile0 + threadIdx.x;
        if (tile0 >= cap) break;  // the whole workgroup alike
        bool live = false;
        u32 ledger = 0;
        u64 ts = 0;
        if (slot < cap) {
            const ulonglong2* e = (const ulonglong2*)&T.acct_hot[slot];
            const ulonglong2 id = e[0], r = e[1];
            ledger = (u32)r.x, ts = r.y;
            live = ts != 0 && !tb_id_reserved(id.x, id.y) && tb_home(id.x, id.y, world) == self;
        }
        if (__ballot(live) == 0) continue;  // the whole wave alike
        const u32 my = live ? tb_ledger_probe(s_set, mask, ledger) : CHANGE_NONE;
        bool adds = my != CHANGE_NONE;
        u128 v[4] = {0, 0, 0, 0};
        u32 count = 0;
        if (live && (adds || all)) {  // the balance planes: live slots only
            const AccountBal b = tb_bal_load(T.bal, slot);
            v[0] = b.debits_pending, v[1] = b.debits_posted, v[2] = b.credits_pending, v[3] = b.credits_posted;
            count = t_at == 0 || ts <= t_at;
        }
        if (all) {
#pragma unroll
            for (u32 c = 0; c < 4; c++) held[c] += tb_wave_sum128(v[c]);
            held_count += (u32)__popcll(__ballot(count != 0));
        }
        if (__ballot(adds) == 0) continue;
        tb_scan_combine<4>(lane, my, adds, v, count);
        if (adds) {
            u64* dst = bins + (u64)my * LEDGER_BIN_WORDS;
            tb_ledger_add<4, LEDGER_TABLE_WORDS>(s_tags, s_bins, my, v, count, dst, dst + LEDGER_BIN_COUNT);
        }
    }
    if (all && lane == 0) {
#pragma unroll
        for (u32 c = 0; c < 4; c++) tb_atomic_add128(s_all + 2 * c, held[c]);
        if (held_count) atomicAdd((unsigned long long*)(s_all + 8), (unsigned long long)held_count);
    }
    // The workgroup's LDS bins go to HBM: a thread per 128-bit word, the unclaimed ones skipped.
    __syncthreads();
    for (u32 i = threadIdx.x; i < (LEDGER_LDS_BINS + 1) * 5; i += LEDGER_THREADS) {
        const u32 b = i / 5, c = i % 5;
        const u32 index = b == LEDGER_LDS_BINS ? mask + 1 : s_tags[b];
        if (index == CHANGE_NONE) continue;
        const u64* src = s_bins + b * LEDGER_TABLE_WORDS + 2 * c;
        u64* dst = bins + (u64)index * LEDGER_BIN_WORDS + 2 * c;
        if (c < 4) tb_atomic_add128(dst, tb_u128(src[0], src[1]));
        else if (src[0]) atomicAdd((unsigned long long*)dst, (unsigned long long)src[0]);
    }
}

// N.T[self] is the scanned engine, n its log's end; a post's pending transfer is read on the home of
// its pending_id.  set, all, bins: as above.  Workgroup b scans tiles [b, b + 1) * LEDGER_LOG_TILES of
// LEDGER_THREADS positions.
__global__ __launch_bounds__(LEDGER_THREADS) void tb_ledger_effects(NodeTablesArgs N, u32 self, u64 n, u64 t_at, const u32* set,
                                                                     u32 mask, u32 all, u64* bins) {
    extern __shared__ __attribute__((aligned(16))) u8 s_lds[];
    u32* s_set = (u32*)s_lds;
    u64* s_bins = (u64*)(s_set + mask + 1);
    u64* s_all = s_bins + LEDGER_LDS_BINS * LEDGER_LOG_WORDS;
    u32* s_tags = (u32*)(s_all + LEDGER_LOG_WORDS);
    const Tables& T = N.T[self];
    const u32 lane = threadIdx.x & 63;
    u64* flags = bins + ((u64)mask + 2) * LEDGER_BIN_WORDS;
    for (u32 i = threadIdx.x; i <= mask; i += LEDGER_THREADS) s_set[i] = set[i];
    for (u32 i = threadIdx.x; i < (LEDGER_LDS_BINS + 1) * LEDGER_LOG_WORDS; i += LEDGER_THREADS) s_bins[i] = 0;
    for (u32 i = threadIdx.x; i < LEDGER_LDS_BINS; i += LEDGER_THREADS) s_tags[i] = CHANGE_NONE;
    __syncthreads();
    u128 held[2] = {0, 0};  // the wave's every-ledger share: the same in every lane
    for (u32 t = 0; t < LEDGER_LOG_TILES; t++) {
        const u64 tile0 = ((u64)blockIdx.x * LEDGER_LOG_TILES + t) * LEDGER_THREADS, pos = tile0 + threadIdx.x;
        if (tile0 >= n) break;  // the whole workgroup alike
        // The timestamp alone first: at or below T (every tile of an ordered log's prefix) nothing else
        // is read.
        const u64* w = (const u64*)&T.xlog[pos < n ? pos : 0];
        const u64 ts = pos < n ? tb_log_ts(T, pos, w[15]) : 0;  // the plane: coalesced, beside chunk 7
        const bool newer = ts > t_at;
        if (__ballot(newer) == 0) continue;  // the whole wave alike
        u32 my = CHANGE_NONE;
        u64 tail = 0;
        if (newer) {
            tail = w[14];  // {ledger, code, flags}
            my = tb_ledger_probe(s_set, mask, (u32)tail);
        }
        bool adds = my != CHANGE_NONE;
        u128 v[2] = {0, 0};  // the record's effect on *_pending and *_posted of either side
        bool sums = false;
        if (newer && (adds || all)) {
            // Live: the id index holds this record's id at this position (tb_query_hit's test).
            const u64 lo = w[0], hi = w[1];
            if (!tb_id_reserved(lo, hi) && tb_transfer_find(T, lo, hi) == (u32)pos) {
                const u128 amount = tb_u128(w[6], w[7]);
                const u32 tf = (u32)(tail >> 48);
                u128 p = amount;
                if (tb_effect_is_post(tf) && !tb_pending_amount(N, w[8], w[9], &p)) {
                    atomicOr((unsigned long long*)(flags + CHANGE_FLAG_ORPHAN), 1ULL);
                }
                const BalanceEffect e = tb_balance_effect(tf, amount, p);
                v[0] = e.pend, v[1] = e.post;
                sums = true;
            }
        }
        adds = adds && sums;
        if (all) held[0] += tb_wave_sum128(v[0]), held[1] += tb_wave_sum128(v[1]);
        if (__ballot(adds) == 0) continue;
        u32 none = 0;
        tb_scan_combine<2>(lane, my, adds, v, none);
        if (adds) {
            u64* dst = bins + (u64)my * LEDGER_BIN_WORDS + LEDGER_BIN_EFFECTS;
            tb_ledger_add<2, LEDGER_LOG_WORDS>(s_tags, s_bins, my, v, 0, dst, dst);
        }
    }
    if (all && lane == 0) tb_atomic_add128(s_all, held[0]), tb_atomic_add128(s_all + 2, held[1]);
    // The workgroup's LDS bins go to HBM: a thread per 128-bit word, the unclaimed ones skipped.
    __syncthreads();
    for (u32 i = threadIdx.x; i < (LEDGER_LDS_BINS + 1) * 2; i += LEDGER_THREADS) {
        const u32 b = i >> 1, c = i & 1;
        const u32 index = b == LEDGER_LDS_BINS ? mask + 1 : s_tags[b];
        if (index == CHANGE_NONE) continue;
        const u64* src = s_bins + b * LEDGER_LOG_WORDS + 2 * c;
        tb_atomic_add128(bins + (u64)index * LEDGER_BIN_WORDS + LEDGER_BIN_EFFECTS + 2 * c, tb_u128(src[0], src[1]));
    }
}
