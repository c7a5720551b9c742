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
// The set is an open-addressing table of 32-bit entries {16-bit tag, account index + 1} built on the
// host; every workgroup copies it into LDS once, and a tag match is confirmed against the full id.
// The accounts that come first in the page (index < CHANGE_LDS_BINS) have their bins in LDS as well:
// a workgroup adds there and hands each bin it touched to HBM once, at its end.
// Plain launches: no grid barrier, no spin, no wait on another workgroup; every loop is bounded by
// the workgroup's tiles, the table's slots or the 64 lanes of a wave.
#pragma once

#include "k_balances.h"

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
#define CHANGE_NONE 0xFFFFFFFFu
// 512 positions a tile (two of k_query.h's) and 16 tiles a workgroup: a workgroup of eight waves
// spreads its copy of the set and its LDS bins over 8,192 records, and two such workgroups fit a CU's
// LDS at the largest set, sixteen waves a CU; 256 threads would leave eight.
#define CHANGE_THREADS 512
#define CHANGE_TILES 16
// Flag words behind the bins, in a slot of their own: {0: a post's pending transfer was not resident}.
#define CHANGE_FLAG_ORPHAN 0

// The set's hash of an account id: the low bits pick the slot, the top 16 the tag.  Independent of
// tb_home's bits and of the account table's position bits by a second mix.
__host__ __device__ static inline u64 tb_change_hash(u64 lo, u64 hi) { return tb_mix64(tb_hash_id(lo, hi) ^ 0x9e3779b97f4a7c15ULL); }
__host__ __device__ static inline u32 tb_change_entry(u64 h, u32 index) { return (u32)(h >> 48) << 16 | (index + 1); }

__host__ static inline u32 tb_change_lds_bins(u32 slots) { return slots <= CHANGE_LDS_BINS_SLOTS_MAX ? CHANGE_LDS_BINS : 0; }
__host__ static inline u32 tb_change_set_slots(u32 accounts) {
    u32 s = CHANGE_SET_SLOTS_MIN;
    while (s < 2 * accounts) s <<= 1;
    return s;
}

// The index of account (lo, hi) in the page's set, or CHANGE_NONE.  s_set: the workgroup's copy of
// the entries; ids: the accounts' ids by index (lo, hi), read on a tag match only.
__device__ static inline u32 tb_change_probe(const u32* s_set, u32 mask, const u64* ids, u64 lo, u64 hi) {
    const u64 h = tb_change_hash(lo, hi);
    const u32 tag = (u32)(h >> 48);
    u32 s = (u32)h & mask;
    for (u32 i = 0; i <= mask; i++) {
        const u32 e = s_set[s];
        if (e == 0) return CHANGE_NONE;
        if ((e >> 16) == tag) {
            const u32 index = (e & 0xFFFFu) - 1;
            if (ids[2 * (u64)index] == lo && ids[2 * (u64)index + 1] == hi) return index;
        }
        s = (s + 1) & mask;
    }
    return CHANGE_NONE;
}

// The same over a workgroup's narrowed copy of the entries (tb_change_lds_entry): {3-bit tag, index + 1}
// in 16 bits, for sets whose indices stay below 8,191.  One occupied slot in eight passes the tag and
// pays the read of the full id.
__device__ static inline u32 tb_change_probe(const u16* s_set, u32 mask, const u64* ids, u64 lo, u64 hi) {
    const u64 h = tb_change_hash(lo, hi);
    const u32 tag = (u32)(h >> 61);
    u32 s = (u32)h & mask;
    for (u32 i = 0; i <= mask; i++) {
        const u32 e = s_set[s];
        if (e == 0) return CHANGE_NONE;
        if ((e >> 13) == tag) {
            const u32 index = (e & 0x1FFFu) - 1;
            if (ids[2 * (u64)index] == lo && ids[2 * (u64)index + 1] == hi) return index;
        }
        s = (s + 1) & mask;
    }
    return CHANGE_NONE;
}

// An entry of the set as a workgroup keeps it in LDS: as it is, or narrowed to the top three bits of
// its tag and its index + 1 (at most 8,191, never zero for an entry that is not).
template <typename ENTRY>
__device__ static inline ENTRY tb_change_lds_entry(u32 e) {
    if (sizeof(ENTRY) == 4) return (ENTRY)e;
    return (ENTRY)(e ? (e >> 29) << 13 | (e & 0x1FFFu) : 0);
}

// CACHED bins: the LDS bin that holds `index`'s sums in this workgroup, claimed at its first add — one
// of the two slots the index hashes to — or CHANGE_NONE when other indices hold both (the add goes to
// HBM).  tags: [bins] the index each LDS bin holds, CHANGE_NONE while free.
__device__ static inline u32 tb_change_bin_claim(u32* tags, u32 bins, u32 index) {
    u32 s = index % bins;
#pragma unroll
    for (u32 k = 0; k < 2; k++) {
        const u32 old = atomicCAS(&tags[s], CHANGE_NONE, index);
        if (old == CHANGE_NONE || old == index) return s;
        s = ((index * 0x9E3779B1u) >> 7) % bins;
    }
    return CHANGE_NONE;
}

// Lane `from`'s value (any lane's own when `from` is itself).
__device__ static inline u128 tb_shfl128(u128 v, u32 from) {
    const u64 lo = __shfl((unsigned long long)tb_lo(v), (int)from);
    const u64 hi = __shfl((unsigned long long)tb_hi(v), (int)from);
    return tb_u128(lo, hi);
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
    const Tables& T = N.T[self];
    const u32 lane = threadIdx.x & 63;
    u64* flags = bins + (u64)n_accounts * BALANCE_SLOT_WORDS;
    const u32 lds_bins = CACHED || n_accounts >= lds_bins_max ? lds_bins_max : n_accounts;
    u32* s_tags = (u32*)(s_bins + lds_bins * BALANCE_SLOT_WORDS);  // CACHED: the index each LDS bin holds
    for (u32 i = threadIdx.x; i <= mask; i += CHANGE_THREADS) s_set[i] = tb_change_lds_entry<ENTRY>(set[i]);
    for (u32 i = threadIdx.x; i < lds_bins * BALANCE_SLOT_WORDS; i += CHANGE_THREADS) s_bins[i] = 0;
    if (CACHED) {
        for (u32 i = threadIdx.x; i < lds_bins; i += CHANGE_THREADS) s_tags[i] = CHANGE_NONE;
    }
    __syncthreads();
    for (u32 t = 0; t < CHANGE_TILES; t++) {
        const u64 tile0 = ((u64)blockIdx.x * CHANGE_TILES + t) * CHANGE_THREADS, pos = tile0 + threadIdx.x;
        if (tile0 >= n) break;  // the whole workgroup alike
        // The timestamp alone first: below the page's end (every tile of an ordered log's prefix) the
        // ids are never read.
        const u64* w = (const u64*)&T.xlog[pos < n ? pos : 0];
        const u64 ts = pos < n ? tb_log_ts(T, pos, w[15]) : 0;  // the plane: coalesced, beside chunk 7
        const bool newer = ts > t_last;
        if (__ballot(newer) == 0) continue;  // the whole wave alike
        u32 idx[2] = {CHANGE_NONE, CHANGE_NONE};  // the debit and the credit account's index
        u128 pend = 0, post = 0;                  // the record's effect on *_pending and *_posted of either side
        if (newer) {
            const ulonglong2 d = ((const ulonglong2*)w)[1], c = ((const ulonglong2*)w)[2];
            idx[0] = tb_change_probe(s_set, mask, ids, d.x, d.y);
            idx[1] = tb_change_probe(s_set, mask, ids, c.x, c.y);
        }
        if ((idx[0] & idx[1]) != CHANGE_NONE) {
            // Live: the id index holds this record's id at this position (tb_query_hit's test).
            const u64 lo = w[0], hi = w[1];
            if (tb_id_reserved(lo, hi) || tb_transfer_find(T, lo, hi) != (u32)pos) {
                idx[0] = idx[1] = CHANGE_NONE;
            } else {
                const u128 amount = tb_u128(w[6], w[7]);
                const u32 tf = (u32)(w[14] >> 48);
                u128 p = amount;
                if (tb_effect_is_post(tf) && !tb_pending_amount(N, w[8], w[9], &p)) {
                    atomicOr((unsigned long long*)(flags + CHANGE_FLAG_ORPHAN), 1ULL);
                }
                const BalanceEffect e = tb_balance_effect(tf, amount, p);
                pend = e.pend, post = e.post;
            }
        }
        // The adds, a side at a time (side 0: the debit columns 0-1, side 1: the credit columns 2-3).
        // The lanes of the wave that hold the same index combine before one of them adds.  The loop
        // visits each distinct index once and only links its lanes into a chain (each lane learns
        // the next lane of its group); one pointer-jumping pass of six steps then sums every chain at
        // once into its first lane, so the shuffles do not grow with the number of distinct indices.
        // A lane alone with its index keeps its own effect.  Then every first lane adds at once: into
        // the workgroup's LDS bin where the index has one, else into the bin in HBM.
#pragma unroll
        for (u32 side = 0; side < 2; side++) {
            const u32 my = idx[side];
            bool adds = my != CHANGE_NONE;
            u128 v0 = adds ? pend : (u128)0, v1 = adds ? post : (u128)0;
            u32 nxt = lane;  // the next lane of this lane's group; itself: none
            bool chains = false;
            u64 todo = __ballot(adds);
            while (todo) {  // at most 64 rounds: every round clears its leader's bit
                const int leader = __ffsll((unsigned long long)todo) - 1;
                const u32 b = __shfl(my, leader);
                const bool mine = my == b;  // (CHANGE_NONE lanes never equal a leader's index)
                const u64 group = __ballot(mine);
                todo &= ~group;
                if ((group & (group - 1)) == 0) continue;
                chains = true;
                if (mine) {
                    const u64 above = lane == 63 ? 0 : group & ~((2ULL << lane) - 1);
                    if (above) nxt = (u32)__ffsll((unsigned long long)above) - 1;
                    if ((int)lane != leader) adds = false;
                }
            }
            if (chains) {
                // v = the sum of the chain from this lane on: after step s it covers 2^(s+1) lanes.
#pragma unroll
                for (u32 s = 0; s < 6; s++) {
                    const bool has = nxt != lane;
                    const u128 o0 = tb_shfl128(v0, nxt), o1 = tb_shfl128(v1, nxt);
                    const u32 nn = __shfl(nxt, nxt);
                    if (has) {
                        v0 += o0, v1 += o1;
                        nxt = nn == nxt ? lane : nn;
                    }
                }
            }
            u32 at = my;  // the index's LDS bin, where it has one
            if (CACHED && adds) at = tb_change_bin_claim(s_tags, lds_bins, my);
            if (adds && at < lds_bins) {
                u64* dst = s_bins + at * BALANCE_SLOT_WORDS + 4 * side;
                tb_atomic_add128(dst, v0);
                tb_atomic_add128(dst + 2, v1);
            } else if (adds) {
                u64* dst = bins + (u64)my * BALANCE_SLOT_WORDS + 4 * side;
                tb_atomic_add128(dst, v0);
                tb_atomic_add128(dst + 2, v1);
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
