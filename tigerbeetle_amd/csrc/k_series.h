// k_series.h — get_account_statement_series (include/tbgpu.h tbgpu_get_account_statement_series): for
// the accounts the caller names and B consecutive periods (bounds[k], bounds[k + 1]], the statement
// row of every (account, period) — what B tbgpu_get_account_statements calls would write, from one
// scan of the log.
//
// k_statement.h's scan sorts a record into one of two zones.  Here it sorts it into one of B + 1
// buckets: bucket k < B is the period (bounds[k], bounds[k + 1]], bucket B, the tail, is everything
// above a non-zero last bound.  Every bucket keeps the same 14 words, a side's {pending_in,
// pending_out, posted_in} and its transfer count (tb_statement_flows); the tail's balance effect is
// {pending_in - pending_out, posted_in} of its sums, tb_balance_effect read by its signs, so the tail
// needs no layout of its own.  With net(j) that pair of bucket j,
//   closing(k) = current - the sum of net(j) over k < j <= B,
//   opening(k) = closing(k) - net(k)                       (tb_statement_row's arithmetic),
// per column modulo 2^128: closing(k) is opening(k + 1) and every row is the single call's.
//   tb_asof_gather     (k_asof.h, as it is, T = the last bound) the records, the found flags, the set;
//   tb_series_effects  bins[index * (B + 1) + bucket] += the record's sums, for every record above bounds[0];
//   tb_series_emit     a lane per (found account, bucket): the suffix sum over the account's later
//                      buckets is a segmented scan over the lanes, so no lane walks B buckets.
// A member of k_account_scan.h's family.  Its own: after the record step, and only for a live hit, the
// bucket, a binary search of at most 12 steps over the bounds in LDS; the in-wave combine and the
// claimed LDS bins go by the key index * (B + 1) + bucket: one wave can hold one account below
// bounds[0], in many buckets and in the tail at once.
#pragma once

#include "k_statement.h"

#define SERIES_ROWS_MAX 4095u  // TBGPU_SERIES_ROWS_MAX: n * n_buckets, 256-B rows in one message body
// A bin, in 64-bit words: per side (debit, then credit) {pending_in, pending_out, posted_in} of two
// words each and the side's transfer count — k_statement.h's zone 1.
#define SERIES_BIN_WORDS (2 * STATEMENT_SIDE_WORDS)
// Keys: index * (B + 1) + bucket, index < n and n * B <= 4,095, so below n * (B + 1) <= 8,190.
#define SERIES_KEYS_MAX (2 * SERIES_ROWS_MAX)
#define SERIES_SEARCH_STEPS 12  // 2^12 > 4,095 bounds
// LDS beside the claimed bins: the set's slots of 32 bits and the B + 1 bounds.  n * B <= 4,095 keeps
// them from both being large: 8,192 slots and 2 bounds (n = 4,095), or 256 slots and 4,096 bounds
// (B = 4,095), 33,792 B at most.
#define SERIES_LDS_FIXED_MAX (256u * 4 + (SERIES_ROWS_MAX + 1) * 8)
// The claimed bins: 116 B each with the tag.  176 of them, 20,416 B, keep the largest workgroup at
// 54,208 B, three workgroups a CU (160 KB of LDS), as tb_statement_effects has; DESIGN.md 7m has the
// counts measured.  The macro can be set from the compiler's command line for such a build.
#ifndef SERIES_LDS_BINS
#define SERIES_LDS_BINS 176u
#endif
// tb_series_emit reads the request's found flags in chunks of its workgroup's size: 16 x 256 >= 4,095.
#define SERIES_EMIT_CHUNKS ((SERIES_ROWS_MAX + QUERY_THREADS) / QUERY_THREADS)

__host__ static inline size_t tb_series_lds_bytes(u32 slots, u32 n_buckets) {
    return (size_t)slots * 4 + ((size_t)n_buckets + 1) * 8 + (size_t)SERIES_LDS_BINS * (SERIES_BIN_WORDS * 8 + 4);
}

// N.T[self] is the scanned engine.  bounds: n_buckets + 1 words as the caller gave them (a last bound
// of 0: no upper end, kept in LDS as 2^64-1, which no valid bound equals).  set: mask + 1 entries
// built by tb_asof_gather; ids: the request; bins: [n_ids * (n_buckets + 1)][SERIES_BIN_WORDS] by key,
// then the flag word {a post's pending transfer was not resident} — all zeroed on the stream before
// the launch.  Workgroup b scans tiles [b, b + 1) * CHANGE_TILES of CHANGE_THREADS positions.
// Dynamic LDS (tb_series_lds_bytes): the bounds, the set's entries, SERIES_LDS_BINS bins, their tags.
__global__ __launch_bounds__(CHANGE_THREADS) void tb_series_effects(NodeTablesArgs N, u32 self, u64 n, const u64* bounds,
                                                                   u32 n_buckets, const u32* set, u32 mask, const u64* ids,
                                                                   u32 n_ids, u64* bins) {
    extern __shared__ __attribute__((aligned(16))) u8 s_lds[];
    u64* s_bounds = (u64*)s_lds;                       // n_buckets + 1 words
    u32* s_set = (u32*)(s_bounds + n_buckets + 1);     // mask + 1 entries
    u64* s_bins = (u64*)(s_set + mask + 1);            // the claimed bins (mask + 1 is even: 8-B aligned)
    u32* s_tags = (u32*)(s_bins + SERIES_LDS_BINS * SERIES_BIN_WORDS);  // the key each holds
    const u32 lane = threadIdx.x & 63;
    const u32 stride = n_buckets + 1;  // keys of one index
    u64* flags = bins + (u64)n_ids * stride * SERIES_BIN_WORDS;
    for (u32 i = threadIdx.x; i <= n_buckets; i += CHANGE_THREADS) {
        const u64 b = bounds[i];
        s_bounds[i] = i == n_buckets && b == 0 ? ~0ULL : b;
    }
    tb_scan_lds_init(s_set, set, mask, s_bins, SERIES_LDS_BINS * SERIES_BIN_WORDS, s_tags, SERIES_LDS_BINS);
    __syncthreads();
    const u64 t_open = s_bounds[0];
    for (u32 t = 0; t < CHANGE_TILES; t++) {
        const u64 tile0 = ((u64)blockIdx.x * CHANGE_TILES + t) * CHANGE_THREADS, pos = tile0 + threadIdx.x;
        if (tile0 >= n) break;  // the whole workgroup alike
        ScanRecord r;
        u128 a[3] = {0, 0, 0};  // {pending_in, pending_out, posted_in}
        u32 bucket = 0;
        const u64 any = tb_scan_record(N, self, pos, n, t_open, s_set, mask, ids, flags, r, [&](u32 tf, u128 amount, u128 p) {
            const StatementFlows f = tb_statement_flows(tf, amount, p);
            a[0] = f.pending_in, a[1] = f.pending_out, a[2] = f.posted_in;
            // The bucket: the number of bounds[1 .. n_buckets] below ts — the smallest k with
            // ts <= bounds[k + 1], or n_buckets, the tail, above them all.
            u32 lo_k = 0, hi_k = n_buckets;
#pragma unroll 1
            for (u32 s = 0; s < SERIES_SEARCH_STEPS && lo_k < hi_k; s++) {
                const u32 mid = (lo_k + hi_k) >> 1;
                if (s_bounds[1 + mid] < r.ts) lo_k = mid + 1;
                else hi_k = mid;
            }
            bucket = lo_k;
        });
        if (any == 0) continue;  // the whole wave alike
        // The adds, a side at a time: the lanes that hold the same key combine, then every first lane
        // adds at once, into the workgroup's LDS bin where the key has claimed one, else into the bin
        // in HBM.
#pragma unroll
        for (u32 side = 0; side < 2; side++) {
            const u32 index = r.idx[side];
            bool adds = index != CHANGE_NONE;
            const u32 my = adds ? index * stride + bucket : CHANGE_NONE;  // (below SERIES_KEYS_MAX)
            u128 v[3] = {adds ? a[0] : (u128)0, adds ? a[1] : (u128)0, adds ? a[2] : (u128)0};
            u32 count = adds ? 1 : 0;  // the lanes summed: the bucket's transfers
            tb_scan_combine<3>(lane, my, adds, v, count);
            if (!adds) continue;
            const u32 at = tb_change_bin_claim(s_tags, SERIES_LDS_BINS, my);
            u64* bin = at != CHANGE_NONE ? s_bins + at * SERIES_BIN_WORDS : bins + (u64)my * SERIES_BIN_WORDS;
            u64* dst = bin + STATEMENT_SIDE_WORDS * side;
            tb_atomic_add128(dst, v[0]);
            tb_atomic_add128(dst + 2, v[1]);
            tb_atomic_add128(dst + 4, v[2]);
            atomicAdd((unsigned long long*)(dst + 6), (unsigned long long)count);
        }
    }
    // The workgroup's claimed bins go to HBM: a thread per word-pair column and the two counts, the
    // unclaimed bins skipped (tb_atomic_add128 skips a zero sum).
    __syncthreads();
    for (u32 i = threadIdx.x; i < SERIES_LDS_BINS * 8; i += CHANGE_THREADS) {
        const u32 b = i / 8, part = i % 8, key = s_tags[b];
        if (key == CHANGE_NONE) continue;
        const u64* src = s_bins + b * SERIES_BIN_WORDS;
        u64* dst = bins + (u64)key * SERIES_BIN_WORDS;
        if (part < 6) {  // the six sums: three a side
            const u32 o = STATEMENT_SIDE_WORDS * (part / 3) + 2 * (part % 3);
            tb_atomic_add128(dst + o, tb_u128(src[o], src[o + 1]));
        } else {  // the two counts
            const u32 o = STATEMENT_SIDE_WORDS * (part - 6) + 6;
            if (src[o]) atomicAdd((unsigned long long*)(dst + o), (unsigned long long)src[o]);
        }
    }
}

// A bucket's net effect on the four columns {debits_pending, debits_posted, credits_pending,
// credits_posted}: {pending_in - pending_out, posted_in} a side.
__host__ __device__ static inline void tb_series_net(const u64* bin, u128 net[4]) {
#pragma unroll
    for (u32 side = 0; side < 2; side++) {
        const u64* z = bin + STATEMENT_SIDE_WORDS * side;
        net[2 * side] = tb_u128(z[0], z[1]) - tb_u128(z[2], z[3]);
        net[2 * side + 1] = tb_u128(z[4], z[5]);
    }
}

// Workgroup b writes rows [b, b + 1) * QUERY_THREADS; row g is bucket g % n_buckets of the found
// account of rank g / n_buckets.  Every workgroup ranks the whole request for itself (at most 4,095
// flags, 16 a thread, by ballots and one wave's scan of the 64 counts), so none waits for another.  A row's closing is the account's current balances
// (tb_flows_row's `closing`) less the nets of its later buckets and the tail: lane (r, k) loads net(k + 1), a segmented suffix
// scan over the wave's lanes sums them within each account, the waves' heads carry across waves, and
// what lies past the workgroup's last row — buckets of its last account only — is summed by all of
// its threads together.  out: room for `cap` rows of STATEMENT_ROW_BYTES.
__global__ __launch_bounds__(QUERY_THREADS) void tb_series_emit(const u64* ids, u32 n, u32 n_buckets, const u8* accounts,
                                                                const u32* found, const u32* set, u32 mask, const u64* bins,
                                                                u32 cap, u8* out, u64* res) {
    __shared__ u32 s_cnt[SERIES_EMIT_CHUNKS * QUERY_WAVES];  // found positions of a (chunk, wave), then those before it
    __shared__ u32 s_pos[QUERY_THREADS + 1];  // the request position of the workgroup's j-th account
    __shared__ u32 s_first[QUERY_WAVES], s_last[QUERY_WAVES];  // the rank at a wave's lane 0 and lane 63
    __shared__ u64 s_head[QUERY_WAVES][8];                     // lane 0's suffix sum
    __shared__ u64 s_ext[QUERY_WAVES][8];                      // the waves' shares of what lies past the workgroup
    static_assert(SERIES_EMIT_CHUNKS * QUERY_WAVES == 64 && SERIES_EMIT_CHUNKS <= 32, "one wave scans the counts; a flag a chunk fits 32 bits");
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 stride = n_buckets + 1;
    // The whole request's found flags, chunk c's position c * QUERY_THREADS + thread to this thread:
    // the loads are coalesced and independent, and (chunk, wave) order is request order.
    u32 flags = 0;
#pragma unroll
    for (u32 c = 0; c < SERIES_EMIT_CHUNKS; c++) {
        const u32 j = c * QUERY_THREADS + threadIdx.x;
        const bool f = j < n && found[j] != 0;
        const u64 b = __ballot(f);
        if (f) flags |= 1u << c;
        if (lane == 0) s_cnt[c * QUERY_WAVES + wave] = (u32)__popcll(b);
    }
    __syncthreads();
    u32 total = 0;
    if (wave == 0) {  // the 64 counts into their exclusive prefix sums, the total behind them
        const u32 own = s_cnt[lane];
        u32 incl = own;
#pragma unroll
        for (u32 off = 1; off < 64; off <<= 1) {
            const u32 o = __shfl_up(incl, off);
            if (lane >= off) incl += o;
        }
        s_cnt[lane] = incl - own;
        if (lane == 63) s_first[0] = incl;  // (borrowed until the barrier below)
    }
    __syncthreads();
    total = s_first[0];
    const u32 row0 = blockIdx.x * QUERY_THREADS, r0 = row0 / n_buckets;
    const u32 rows = total * n_buckets;  // (at most 4,095)
#pragma unroll
    for (u32 c = 0; c < SERIES_EMIT_CHUNKS; c++) {
        const bool f = (flags >> c) & 1;
        const u64 b = __ballot(f);
        const u32 rank = s_cnt[c * QUERY_WAVES + wave] + (u32)__popcll(b & ((1ULL << lane) - 1));
        if (f && rank >= r0 && rank - r0 <= QUERY_THREADS) s_pos[rank - r0] = c * QUERY_THREADS + threadIdx.x;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        res[SCAN_RES_MATCHED] = rows;
        res[SCAN_RES_ORPHAN] = bins[(u64)n * stride * SERIES_BIN_WORDS];
    }
    __syncthreads();
    const u32 g = row0 + threadIdx.x;
    const bool have = g < rows;
    const u32 r = have ? g / n_buckets : CHANGE_NONE, k = have ? g % n_buckets : 0;
    u32 index = CHANGE_NONE;  // every lane probes for itself: a found id is in the set
    if (have) {
        const u32 j = s_pos[r - r0];
        index = tb_change_probe(set, mask, ids, ids[2 * (u64)j], ids[2 * (u64)j + 1]);
    }
    u128 x[4] = {0, 0, 0, 0};
    if (index != CHANGE_NONE) tb_series_net(bins + ((u64)index * stride + k + 1) * SERIES_BIN_WORDS, x);
    // The segmented suffix scan: accounts are runs of lanes, so lane + off is in this lane's run
    // exactly when it holds the same rank.
#pragma unroll
    for (u32 off = 1; off < 64; off <<= 1) {
        const u32 from = lane + off < 64 ? lane + off : lane;
        const u32 ro = __shfl(r, from);
        const bool same = lane + off < 64 && ro == r && have;
#pragma unroll
        for (u32 c = 0; c < 4; c++) {
            const u128 o = tb_shfl128(x[c], from);
            if (same) x[c] += o;
        }
    }
    if (lane == 0) {
        s_first[wave] = r;
#pragma unroll
        for (u32 c = 0; c < 4; c++) s_head[wave][2 * c] = tb_lo(x[c]), s_head[wave][2 * c + 1] = tb_hi(x[c]);
    }
    if (lane == 63) s_last[wave] = r;
    // Past the workgroup's last row: the later buckets of that row's account, the tail among them.
    const u32 g_end = row0 + QUERY_THREADS - 1;
    u128 e[4] = {0, 0, 0, 0};
    if (g_end < rows) {
        const u32 r_end = g_end / n_buckets, k_end = g_end % n_buckets, j_end = s_pos[r_end - r0];
        const u32 i_end = tb_change_probe(set, mask, ids, ids[2 * (u64)j_end], ids[2 * (u64)j_end + 1]);
        if (i_end != CHANGE_NONE) {
            for (u32 j = k_end + 2 + threadIdx.x; j <= n_buckets; j += QUERY_THREADS) {
                u128 net[4];
                tb_series_net(bins + ((u64)i_end * stride + j) * SERIES_BIN_WORDS, net);
#pragma unroll
                for (u32 c = 0; c < 4; c++) e[c] += net[c];
            }
        }
    }
#pragma unroll
    for (u32 off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (u32 c = 0; c < 4; c++) e[c] += tb_shfl128(e[c], lane ^ off);
    }
    if (lane == 0) {
#pragma unroll
        for (u32 c = 0; c < 4; c++) s_ext[wave][2 * c] = tb_lo(e[c]), s_ext[wave][2 * c + 1] = tb_hi(e[c]);
    }
    __syncthreads();
    if (!have || index == CHANGE_NONE) return;
    // The carry into this lane's run: only a run that reaches the wave's last lane goes on.
    if (r == s_last[wave]) {
        bool open = true;  // the run goes on past the waves seen so far
        for (u32 w = wave + 1; w < QUERY_WAVES && open; w++) {
            if (s_first[w] != r) {
                open = false;
                break;
            }
#pragma unroll
            for (u32 c = 0; c < 4; c++) x[c] += tb_u128(s_head[w][2 * c], s_head[w][2 * c + 1]);
            open = s_last[w] == r;
        }
        if (open) {
            for (u32 w = 0; w < QUERY_WAVES; w++) {
#pragma unroll
                for (u32 c = 0; c < 4; c++) x[c] += tb_u128(s_ext[w][2 * c], s_ext[w][2 * c + 1]);
            }
        }
    }
    if (g >= cap) return;
    const u64* account = (const u64*)(accounts + (u64)s_pos[r - r0] * 128);
    u128 closing[4];
#pragma unroll
    for (u32 c = 0; c < 4; c++) closing[c] = tb_u128(account[2 + 2 * c], account[3 + 2 * c]) - x[c];
    u64 row[32];
    tb_flows_row(account, bins + ((u64)index * stride + k) * SERIES_BIN_WORDS, closing, row);
    ulonglong2* dst = (ulonglong2*)(out + (u64)g * STATEMENT_ROW_BYTES);
#pragma unroll
    for (u32 q = 0; q < 16; q++) dst[q] = make_ulonglong2(row[2 * q], row[2 * q + 1]);
}
