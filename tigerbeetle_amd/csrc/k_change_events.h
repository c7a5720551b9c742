// k_change_events.h — get_change_events (include/tbgpu.h tbgpu_get_change_events): every transfer of a
// timestamp window in timestamp order, each with both of its accounts as they stood right after it.
//
// Later references keep the change stream in a groove of its own.  Here nothing is stored: the rows
// are query_transfers' answer for an all-zero field filter (k_query.h), and an account's balances
// after a row are its current balances minus the effects of every newer resident record that names it
// (k_balances.h's definition, per column modulo 2^128).  The filter has no field predicate, so the
// page is *every* live record between its first and its last timestamp: the host walks the k rows
// themselves backward (query.h change_walk), and the device only sums what is newer than the last
// row, t_last — one bin per distinct account of the page (at most 2k), whatever the record's distance
// from the page:
//   tb_change_gather   a lane per distinct account: its 128-B record from its owner's table, or a
//                      not-found mark; a lane per post row: its pending transfer's amount from
//                      home(pending_id), or the orphan flag and the row's own amount;
//   tb_change_effects  a scan of the log: a record with timestamp > t_last probes the page's account
//                      set with its debit and its credit id; a hit that is live (k_query.h's probe)
//                      adds its effect into bins[account index].
// The scan is a member of k_account_scan.h's family: its set, record step and combine are that
// header's.  Its own: the set is built on the host, a key is an account index and a bin its four
// columns, and the accounts that come first in the page (index < CHANGE_LDS_BINS) have their bins in
// LDS by position, not by claim.
#pragma once

#include "k_account_scan.h"

#define CHANGE_EVENTS_MAX 2730u                     // TBGPU_CHANGE_EVENTS_MAX
#define CHANGE_ACCOUNTS_MAX (2 * CHANGE_EVENTS_MAX)  // distinct accounts of one page
// Slots of the set: a power of two, at least twice the accounts (load 1/4 .. 1/2; 5,460 accounts take
// 16,384 slots, 64 KB of LDS).  A miss, the common case, ends at the first empty slot it meets.
#define CHANGE_SET_SLOTS_MAX 16384u
#define CHANGE_SET_SLOTS_MIN 256u
// Bins kept in LDS, 64 B each, 32 KB: only beside a set of at most 8,192 slots (4,096 accounts), so
// that set and bins together stay within 64 KB a workgroup.  A page with more distinct accounts
// names none of them in more than a quarter of its events, and measured faster with the sparser set
// than with the bins.
#define CHANGE_LDS_BINS 512u
#define CHANGE_LDS_BINS_SLOTS_MAX 8192u
// Flag words behind the bins, in a slot of their own: {0: a post's pending transfer was not resident}.
#define CHANGE_FLAG_ORPHAN 0

__host__ static inline u32 tb_change_lds_bins(u32 slots) { return slots <= CHANGE_LDS_BINS_SLOTS_MAX ? CHANGE_LDS_BINS : 0; }
__host__ static inline u32 tb_change_set_slots(u32 accounts) {
    u32 s = CHANGE_SET_SLOTS_MIN;
    while (s < 2 * accounts) s <<= 1;
    return s;
}

// ids: n_accounts ids (lo, hi); accounts: their 128-B records; found: 1 per account its owner holds.
// pids: n_rows pending ids (lo, hi) of the post rows, zero for every other row; P: per row {lo, hi} of
// the pending transfer's amount, zero where it is not resident (found_p = 0: the host uses the row's
// own amount and drops `complete`).  A single engine: world = 1, every id's home is 0.
__global__ __launch_bounds__(QUERY_THREADS) void tb_change_gather(NodeTablesArgs N, const u64* ids, u32 n_accounts, u8* accounts,
                                                                  u32* found, const u64* pids, u32 n_rows, u64* P, u32* found_p) {
    const u32 i = blockIdx.x * QUERY_THREADS + threadIdx.x;
    if (i < n_accounts) {
        const u64 lo = ids[2 * (u64)i], hi = ids[2 * (u64)i + 1];
        const Tables& O = N.T[tb_home(lo, hi, N.world)];
        const u32 slot = tb_account_find(O, lo, hi);
        found[i] = slot != TB_NOT_FOUND;
        if (slot != TB_NOT_FOUND) *(Account*)(accounts + (u64)i * 128) = tb_account_load(O, slot);
    }
    if (i < n_rows) {
        u128 p = 0;
        found_p[i] = tb_pending_amount(N, pids[2 * (u64)i], pids[2 * (u64)i + 1], &p);
        P[2 * (u64)i] = tb_lo(p), P[2 * (u64)i + 1] = tb_hi(p);
    }
}

// N.T[self] is the scanned engine.  set: mask + 1 entries; ids: the set's account ids by index; bins:
// [accounts][4] u128 {debits_pending, debits_posted, credits_pending, credits_posted}, low word
// first, then the flag slot at bins + n_accounts * 8 — all zeroed on the stream before the launch.
// Workgroup b scans tiles [b, b + 1) * CHANGE_TILES of CHANGE_THREADS positions.  Dynamic LDS: the
// set's mask + 1 entries, then lds_bins (tb_change_lds_bins) bins of 64 B.
// get_change_events is <u32, false>: the LDS bins are those of the page's first accounts.
// lookup_accounts_at (k_asof.h), whose request order says nothing about hotness, is CACHED: exactly
// lds_bins_max LDS bins, each claimed by the first index that adds to it (tb_change_bin_claim), their
// tags behind them in LDS; and ENTRY u16 where the set would otherwise take all 64 KB.
template <typename ENTRY, bool CACHED>
__global__ __launch_bounds__(CHANGE_THREADS) void tb_change_effects(NodeTablesArgs N, u32 self, u64 n, u64 t_last, const u32* set,
                                                                   u32 mask, const u64* ids, u32 n_accounts, u64* bins,
                                                                   u32 lds_bins_max) {
    extern __shared__ __attribute__((aligned(16))) u8 s_lds[];
    ENTRY* s_set = (ENTRY*)s_lds;            // mask + 1 entries
    u64* s_bins = (u64*)(s_set + mask + 1);  // the bins of the first accounts of the page, or the claimed ones
    const u32 lane = threadIdx.x & 63;
    u64* flags = bins + (u64)n_accounts * BALANCE_SLOT_WORDS;
    const u32 lds_bins = CACHED || n_accounts >= lds_bins_max ? lds_bins_max : n_accounts;
    u32* s_tags = (u32*)(s_bins + lds_bins * BALANCE_SLOT_WORDS);  // CACHED: the index each LDS bin holds
    tb_scan_lds_init(s_set, set, mask, s_bins, lds_bins * BALANCE_SLOT_WORDS, s_tags, CACHED ? lds_bins : 0);
    __syncthreads();
    for (u32 t = 0; t < CHANGE_TILES; t++) {
        const u64 tile0 = ((u64)blockIdx.x * CHANGE_TILES + t) * CHANGE_THREADS, pos = tile0 + threadIdx.x;
        if (tile0 >= n) break;  // the whole workgroup alike
        ScanRecord r;
        BalanceEffect e = {0, 0};  // the record's effect on *_pending and *_posted of either side
        const u64 any = tb_scan_record(N, self, pos, n, t_last, s_set, mask, ids, flags + CHANGE_FLAG_ORPHAN, r,
                                       [&](u32 tf, u128 amount, u128 p) { e = tb_balance_effect(tf, amount, p); });
        if (any == 0) continue;  // the whole wave alike
        // The adds, a side at a time (side 0: the debit columns 0-1, side 1: the credit columns 2-3):
        // the lanes that hold the same index combine, then every first lane adds at once, into the
        // workgroup's LDS bin where the index has one, else into the bin in HBM.
#pragma unroll
        for (u32 side = 0; side < 2; side++) {
            const u32 my = r.idx[side];
            bool adds = my != CHANGE_NONE;
            u128 v[2] = {adds ? e.pend : (u128)0, adds ? e.post : (u128)0};
            u32 none = 0;
            tb_scan_combine<2>(lane, my, adds, v, none);
            u32 at = my;  // the index's LDS bin, where it has one
            if (CACHED && adds) at = tb_change_bin_claim(s_tags, lds_bins, my);
            if (adds && at < lds_bins) {
                u64* dst = s_bins + at * BALANCE_SLOT_WORDS + 4 * side;
                tb_atomic_add128(dst, v[0]);
                tb_atomic_add128(dst + 2, v[1]);
            } else if (adds) {
                u64* dst = bins + (u64)my * BALANCE_SLOT_WORDS + 4 * side;
                tb_atomic_add128(dst, v[0]);
                tb_atomic_add128(dst + 2, v[1]);
            }
        }
    }
    // The workgroup's LDS bins go to HBM: a thread per 128-bit word, the untouched ones skipped.
    __syncthreads();
    for (u32 i = threadIdx.x; i < lds_bins * 4; i += CHANGE_THREADS) {
        const u32 index = CACHED ? s_tags[i >> 2] : i >> 2;
        if (CACHED && index == CHANGE_NONE) continue;
        tb_atomic_add128(bins + (u64)index * BALANCE_SLOT_WORDS + 2 * (i & 3), tb_u128(s_bins[2 * i], s_bins[2 * i + 1]));
    }
}
