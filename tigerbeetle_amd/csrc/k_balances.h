// k_balances.h — get_account_balances (include/tbgpu.h tbgpu_get_account_balances): an account's four
// balances as they stood right after each of the transfers get_account_transfers returns.
//
// Later references store a balance row per transfer of an account that opted in (`history`).  Here
// nothing is stored: the log is in HBM and the account table holds the current balances, so
//   balance_after(r) = current - sum of the effects of the account's resident records newer than r,
// per column modulo 2^128, derived when asked.  The rows are chosen by the query scan (k_query.h);
// their k ascending timestamps cut the time axis into k + 1 bins, and one more scan of the log,
//   tb_balance_effects  k_query.h's tile shape and liveness probe, the account on either side, every
//                       timestamp above the oldest row's: each hit adds its effect on the account's
//                       four columns into bins[number of rows older than the record],
// leaves the host (query.h balances_finish) a suffix sum over k + 1 bins of 64 B.  Whatever order the
// log is in: a record finds its bin by binary search, never by position.  Plain launches: no grid
// barrier, no spin, no wait on another workgroup; every loop is bounded by the workgroup's tiles or the
// distinct bins of a wave.
#pragma once

#include "k_node.h"
#include "k_query.h"

// What the scan leaves in `bins`, in 64-B slots of 4 x u128 {debits_pending, debits_posted,
// credits_pending, credits_posted}, low word first: [0, k] the bins, [k + 1] the account's current
// balances as this engine's table holds them, [k + 2] words {0: a post's pending transfer was not
// resident, 1: the account was found}.  The host zeroes all of it on the stream before the launch.
#define BALANCE_SLOT_WORDS 8
#define BALANCE_SLOTS(k) ((u64)(k) + 3)
// Consecutive tiles of QUERY_THREADS log positions per workgroup.  A hot account's millions of newer
// records nearly all fall into one bin: a wave carries the sum of its current bin across its tiles and
// the workgroup merges its waves' sums, so that bin takes a few adds per 8192 records, not one per
// record or per wave.
#define BALANCE_TILES 32
#define BALANCE_NO_BIN 0xFFFFFFFFu

// Rows with a timestamp below `ts` among the k ascending row timestamps.
__device__ static inline u32 tb_balance_bin(const u64* row_ts, u32 k, u64 ts) {
    u32 lo = 0, hi = k;
    while (lo < hi) {
        const u32 mid = (lo + hi) >> 1;
        if (row_ts[mid] < ts) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The sum over the wave, in every lane.
__device__ static inline u128 tb_wave_sum128(u128 v) {
#pragma unroll
    for (u32 off = 32; off > 0; off >>= 1) {
        const u64 lo = __shfl_xor((unsigned long long)tb_lo(v), off);
        const u64 hi = __shfl_xor((unsigned long long)tb_hi(v), off);
        v += tb_u128(lo, hi);
    }
    return v;
}

// *p += v modulo 2^128, in any order beside other adders: the low add's old value says whether it
// wrapped, and every wrap carries exactly one into the high word.
__device__ static inline void tb_atomic_add128(u64* p, u128 v) {
    if (v == 0) return;
    const u64 lo = tb_lo(v);
    u64 hi = tb_hi(v);
    if (lo) {
        const u64 old = atomicAdd((unsigned long long*)p, (unsigned long long)lo);
        hi += (u64)(old + lo < old);
    }
    if (hi) atomicAdd((unsigned long long*)(p + 1), (unsigned long long)hi);
}

// One thread adds a carried sum to its bin.
__device__ static inline void tb_balance_flush(u64* bins, u32 bin, const u128 v[4]) {
    if (bin == BALANCE_NO_BIN) return;
    u64* dst = bins + (u64)bin * BALANCE_SLOT_WORDS;
#pragma unroll
    for (u32 c = 0; c < 4; c++) tb_atomic_add128(dst + 2 * c, v[c]);
}

// The balance-effect rule: how one log record moves the four balances of the accounts it names, as
// {pend, post} added to *_pending and *_posted of its debit and its credit side, modulo 2^128.  Both
// the balance history and the change stream are "current minus the effects of newer records", so this
// is the definition of their answers, on the device and in the host's walk (query.h) alike.
//   pending   +pending(amount)
//   post      -pending(p), +posted(amount): p is the pending transfer's amount (tb_pending_amount),
//             the post's own amount where the pending transfer is not resident (the caller's orphan flag)
//   void      -pending(amount): a void record stores its pending transfer's amount
//   plain     +posted(amount)
// The post case is tested first, by the predicate the callers guard the lookup with, so that lookup
// and case share one branch on the device.
struct BalanceEffect {
    u128 pend, post;
};
__host__ __device__ static inline bool tb_effect_is_post(u32 flags) { return !(flags & TF_PENDING) && (flags & TF_POST); }
__host__ __device__ static inline BalanceEffect tb_balance_effect(u32 flags, u128 amount, u128 p) {
    if (tb_effect_is_post(flags)) return {(u128)0 - p, amount};
    if (flags & TF_PENDING) return {amount, 0};
    if (flags & TF_VOID) return {(u128)0 - amount, 0};
    return {0, amount};
}

// The amount of the pending transfer (lo, hi) into *p, read on its home's table (a single engine:
// world = 1, every id's home is 0); false, and *p as it was: not resident (evicted, or never there).
__device__ static inline bool tb_pending_amount(const NodeTablesArgs& N, u64 lo, u64 hi, u128* p) {
    if (tb_id_reserved(lo, hi)) return false;
    const Tables& H = N.T[tb_home(lo, hi, N.world)];
    const u32 pp = tb_transfer_find(H, lo, hi);
    if (pp == TB_NOT_FOUND) return false;
    const u64* pw = (const u64*)&H.xlog[pp];
    *p = tb_u128(pw[6], pw[7]);
    return true;
}

// flt: the account on both sides, ts_min = the oldest row's timestamp + 1, no upper bound.
// N.T[self] is the scanned engine; a post's pending transfer is read from N.T[home(pending_id)]
// (a single engine: world = 1, every id's home is 0).  Workgroup b scans tiles [b, b + 1) *
// BALANCE_TILES.
__global__ __launch_bounds__(QUERY_THREADS) void tb_balance_effects(NodeTablesArgs N, u32 self, QueryFilter flt, u64 n,
                                                                    const u64* row_ts, u32 k, u64* bins) {
    __shared__ u32 s_bin[QUERY_WAVES];
    __shared__ u64 s_sum[QUERY_WAVES][BALANCE_SLOT_WORDS];
    const Tables& T = N.T[self];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64* tail = bins + ((u64)k + 1) * BALANCE_SLOT_WORDS;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const u32 slot = tb_account_find(T, flt.id_lo, flt.id_hi);
        if (slot != TB_NOT_FOUND) {
            const AccountBal b = tb_bal_load(T.bal, slot);
            const u128 cur[4] = {b.debits_pending, b.debits_posted, b.credits_pending, b.credits_posted};
            for (u32 c = 0; c < 4; c++) tail[2 * c] = tb_lo(cur[c]), tail[2 * c + 1] = tb_hi(cur[c]);
            tail[BALANCE_SLOT_WORDS + 1] = 1;
        }
    }
    // The wave's carried sum: the same in every lane.
    u32 held_bin = BALANCE_NO_BIN;
    u128 held[4] = {0, 0, 0, 0};
    for (u32 t = 0; t < BALANCE_TILES; t++) {
        const u64 tile0 = ((u64)blockIdx.x * BALANCE_TILES + t) * QUERY_THREADS, pos = tile0 + threadIdx.x;
        if (tile0 >= n) break;  // the whole workgroup alike
        const QueryFields f = tb_query_fields<false, QueryFilter>(T, tile0, n, nullptr);
        const bool hit = tb_query_hit(T, flt, pos, n, f);
        const u64 hits = __ballot(hit);
        if (hits == 0) continue;  // the whole wave alike
        u128 pend = 0, post = 0;  // the record's effect on *_pending and *_posted of its side(s)
        u32 bin = 0;
        bool deb = false, cred = false;
        if (hit) {
            const u64* w = (const u64*)&T.xlog[pos];
            const u128 amount = tb_u128(w[6], w[7]);
            const u32 flags = (u32)(w[14] >> 48);
            u128 p = amount;
            if (tb_effect_is_post(flags) && !tb_pending_amount(N, w[8], w[9], &p)) {
                atomicOr((unsigned long long*)(tail + BALANCE_SLOT_WORDS), 1ULL);
            }
            const BalanceEffect e = tb_balance_effect(flags, amount, p);
            pend = e.pend, post = e.post;
            deb = f.dlo == flt.id_lo && f.dhi == flt.id_hi;
            cred = f.clo == flt.id_lo && f.chi == flt.id_hi;
            bin = tb_balance_bin(row_ts, k, f.ts);
        }
        // Among the rows themselves every hit has a bin of its own; newer than the rows, neighbouring
        // hits share one.  A hit whose neighbours among the wave's hits are in other bins adds for
        // itself, all such lanes at once; the others go bin by bin through the carried sum.  (Equal
        // bins that are not neighbours — an unordered log — add separately: any grouping is exact.)
        const u64 below = hits & ((1ULL << lane) - 1), above = lane == 63 ? 0 : (hits >> (lane + 1)) << (lane + 1);
        const u32 bin_below = __shfl(bin, below ? 63 - __clzll((long long)below) : (int)lane);
        const u32 bin_above = __shfl(bin, above ? __ffsll((unsigned long long)above) - 1 : (int)lane);
        const bool run = hit && ((below && bin_below == bin) || (above && bin_above == bin));
        if (hit && !run) {
            const u128 v[4] = {deb ? pend : 0, deb ? post : 0, cred ? pend : 0, cred ? post : 0};
            tb_balance_flush(bins, bin, v);
        }
        u64 todo = __ballot(run);
        while (todo) {
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const u32 b = __shfl(bin, leader);
            const bool mine = run && bin == b;
            const u64 group = __ballot(mine);
            u128 v[4] = {mine && deb ? pend : 0, mine && deb ? post : 0, mine && cred ? pend : 0, mine && cred ? post : 0};
#pragma unroll
            for (u32 c = 0; c < 4; c++) v[c] = tb_wave_sum128(v[c]);
            if (b != held_bin) {
                if (lane == 0) tb_balance_flush(bins, held_bin, held);
                held_bin = b;
#pragma unroll
                for (u32 c = 0; c < 4; c++) held[c] = 0;
            }
#pragma unroll
            for (u32 c = 0; c < 4; c++) held[c] += v[c];
            todo &= ~group;
        }
    }
    // The waves' carried sums, merged where they share a bin.
    if (lane == 0) {
        s_bin[wave] = held_bin;
        for (u32 c = 0; c < 4; c++) s_sum[wave][2 * c] = tb_lo(held[c]), s_sum[wave][2 * c + 1] = tb_hi(held[c]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (u32 w = 1; w < QUERY_WAVES; w++) {
            if (s_bin[w] != held_bin) {
                tb_balance_flush(bins, held_bin, held);
                held_bin = s_bin[w];
                for (u32 c = 0; c < 4; c++) held[c] = 0;
            }
            for (u32 c = 0; c < 4; c++) held[c] += tb_u128(s_sum[w][2 * c], s_sum[w][2 * c + 1]);
        }
        tb_balance_flush(bins, held_bin, held);
    }
}
