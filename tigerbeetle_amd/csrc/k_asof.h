// k_asof.h — lookup_accounts_at (include/tbgpu.h tbgpu_lookup_accounts_at): the records of up to 8,191
// accounts the caller names, as they stood at a timestamp T the caller names.
//
// No reference can answer it; here it falls out of the design of the other balance queries: nothing
// was stored at commit, the log is in HBM and the account table holds the current balances, so
//   balance_at(a, T) = current(a) - the effects of every live resident record that names a and has a
//                      timestamp strictly above T,
// per column modulo 2^128.  A member of k_account_scan.h's family whose scan *is* k_change_events.h's
// tb_change_effects, with the caller's ids as the page's accounts and T as the page's last timestamp:
//   tb_asof_gather   a lane per request position: the id's record from its owner's table, or a
//                    not-found mark (absent, reserved, or created after T); a found id enters the set;
//   tb_asof_emit     a lane per request position: a found one writes its record, the four balances
//                    less its id's bin, at its rank among the found positions.
// Its own, and every later member's with it: the set is built on the device.  An id's index is the
// smallest request position that names it, and `ids` is the request itself, so the set needs no id
// array of its own and a repeated id resolves to one bin whichever lane came first.  An insert is one
// atomicCAS on an empty slot or one atomicMin on a slot that already holds the same id (same id, same
// tag: the smaller entry is the smaller position).  A request's order says nothing about hotness, so
// the scan's LDS bins are CACHED, claimed by first use; and 8,191 ids need 16,384 slots, all 64 KB as
// 32-bit entries, so above 4,096 ids the workgroup's copy of the set is narrowed to 16 bits an entry
// (the set in HBM stays as it is), which leaves the bins their room (DESIGN.md 7h has both measured).
#pragma once

#include "k_change_events.h"

#define ASOF_IDS_MAX 8191u  // TBGPU_LOOKUP_AT_MAX: index + 1 fits the narrowed entry's 13 bits
// LDS bins of a workgroup of the scan, claimed by the indices that add first (tb_change_bin_claim):
// 28 KB of bins and their tags beside at most 32 KB of set — 8,192 entries of 32 bits up to 4,096 ids,
// 16,384 narrowed to 16 bits above — stay within 64 KB.
#define ASOF_LDS_BINS 448u

// Request position i's id into the set, under the smallest position that names it.
__device__ static inline void tb_asof_insert(u32* set, u32 mask, const u64* ids, u32 i, u64 lo, u64 hi) {
    const u64 h = tb_change_hash(lo, hi);
    const u32 mine = tb_change_entry(h, i);
    u32 s = (u32)h & mask;
    for (u32 n = 0; n <= mask; n++) {  // at most half the slots are ever taken: an empty one ends the probe
        const u32 e = atomicCAS(&set[s], 0u, mine);
        if (e == 0) return;
        if ((e >> 16) == (mine >> 16)) {
            const u32 index = (e & 0xFFFFu) - 1;
            if (ids[2 * (u64)index] == lo && ids[2 * (u64)index + 1] == hi) {
                atomicMin(&set[s], mine);
                return;
            }
        }
        s = (s + 1) & mask;
    }
}

// ids: n request ids (lo, hi); accounts: [n] their 128-B records; found: [n] 1 where the id's owner
// holds an account created at or before T (T = 0: now, every account it holds).  set: mask + 1 zeroed
// entries, or null when no scan follows.  accounts and found null: only the set is wanted (a node's
// shards other than the first, whose records nobody reads).  A single engine: world = 1, every id's
// home is 0.
__global__ __launch_bounds__(QUERY_THREADS) void tb_asof_gather(NodeTablesArgs N, const u64* ids, u32 n, u64 T, u8* accounts,
                                                                u32* found, u32* set, u32 mask) {
    const u32 i = blockIdx.x * QUERY_THREADS + threadIdx.x;
    if (i >= n) return;
    const u64 lo = ids[2 * (u64)i], hi = ids[2 * (u64)i + 1];
    const Tables& O = N.T[tb_home(lo, hi, N.world)];
    const u32 slot = tb_account_find(O, lo, hi);  // (a reserved id is never found)
    bool have = slot != TB_NOT_FOUND;
    if (have) have = T == 0 || O.acct_hot[slot].timestamp <= T;
    if (accounts) {
        if (have) *(Account*)(accounts + (u64)i * 128) = tb_account_load(O, slot);
        found[i] = have;
    }
    if (have && set) tb_asof_insert(set, mask, ids, i, lo, hi);
}

// Workgroup b answers request positions [b, b + 1) * QUERY_THREADS (tb_scan_emit_rank).  set, bins: the
// scan's (bins + n * BALANCE_SLOT_WORDS its flag slot), or null when none ran: the records go out as
// they are.  out: room for `cap` records.
__global__ __launch_bounds__(QUERY_THREADS) void tb_asof_emit(const u64* ids, u32 n, const u8* accounts, const u32* found,
                                                              const u32* set, u32 mask, const u64* bins, u32 cap, u8* out,
                                                              u64* res) {
    u32 rank, total;
    const bool have = tb_scan_emit_rank(found, n, rank, total);
    const u32 i = blockIdx.x * QUERY_THREADS + threadIdx.x;
    if ((blockIdx.x + 1) * QUERY_THREADS >= n && threadIdx.x == 0) {  // the last workgroup: every found position
        res[SCAN_RES_MATCHED] = total;
        res[SCAN_RES_ORPHAN] = bins ? bins[(u64)n * BALANCE_SLOT_WORDS + CHANGE_FLAG_ORPHAN] : 0;
    }
    if (!have || rank >= cap) return;
    const ulonglong2* src = (const ulonglong2*)(accounts + (u64)i * 128);
    ulonglong2* dst = (ulonglong2*)(out + (u64)rank * 128);
    dst[0] = src[0];
    u32 index = CHANGE_NONE;
    if (bins) index = tb_change_probe(set, mask, ids, src[0].x, src[0].y);  // a found id is in the set
#pragma unroll
    for (u32 c = 0; c < 4; c++) {
        u128 v = tb_u128(src[1 + c].x, src[1 + c].y);
        if (index != CHANGE_NONE) v -= tb_u128(bins[(u64)index * BALANCE_SLOT_WORDS + 2 * c], bins[(u64)index * BALANCE_SLOT_WORDS + 2 * c + 1]);
        dst[1 + c] = make_ulonglong2(tb_lo(v), tb_hi(v));
    }
#pragma unroll
    for (u32 q = 5; q < 8; q++) dst[q] = src[q];
}
