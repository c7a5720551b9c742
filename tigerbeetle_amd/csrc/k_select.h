// k_select.h — the first k of a table's keys, selected on the device in memory that does not grow with
// the keys ("The select"): a most-significant-digit radix select of the k-th smallest
// key, SEL_BITS bits a pass, over a key of SRC::WORDS 64-bit words, most significant first.
//
// The key source SRC is a small struct passed by value: `static constexpr u32 WORDS`, and a device
// member `bool key(u64 slot, u64 (&K)[WORDS]) const` that yields slot's key or false: the slot holds
// nothing.  The table is covered in tiles of QUERY_THREADS slots; counts[b] is how many slots of tile b
// hold a key, and every step skips a tile whose count is zero.
//
// The caller zeroes the state and the histograms that follow it on the stream, fills counts, and
// writes SEL_TOTAL, SEL_RANK = k, SEL_PREFIX = the bits every key shares (any value where SEL_VARIES
// is set) and SEL_VARIES.  Then, enqueued back to back (query.h select_enqueue):
//   tb_select_hist /  a pass histograms the digit of the keys that carry the prefix chosen so far (LDS
//   tb_select_pick    per workgroup, non-returning global atomics to merge) and one workgroup picks
//                     the digit under which the SEL_RANK-th smallest key falls.  A pass exits on what it
//                     reads from device memory unless the total exceeds k, the select is not done, and
//                     two keys differ in its digit.  Where the picked digit's keys are all wanted —
//                     the rank is their count — the prefix is final: every bit below the digit becomes
//                     one, SEL_DONE is set and the remaining passes exit;
//   tb_select_collect the keys at or below the prefix (every key when the total is at most k) append
//                     {key words, slot} to a k-entry buffer through one counter.  Keys are unique, so
//                     exactly min(k, total) qualify; the store is guarded by index < k all the same;
//   tb_select_rank    for the caller's emit kernel: rank by counting over the collected entries.
// Plain launches: no grid barrier, no spin, no wait on another workgroup; every loop is bounded by the
// grid, by k or by a constant.
#pragma once

#include "k_query.h"

#define SEL_BITS 11u
#define SEL_BINS (1u << SEL_BITS)
#define SEL_WORD_PASSES 6u  // 6 x 11 bits cover a 64-bit word
#define SEL_KEY_WORDS_MAX 4u
#define SEL_TILES 4u        // tiles one workgroup of tb_select_hist / tb_select_collect covers
#define SEL_EMIT_LANES 16u  // lanes that share a key in tb_select_rank
#define SEL_EMIT_KEYS (QUERY_THREADS / SEL_EMIT_LANES)

// Device state of one select, u64 words, two 128-byte lines: a caller's own words sit beside the
// select's, from SEL_CALLER in the first line and from SEL_WORDS on; then the histograms: u32
// [passes][SEL_BINS].  The first line's free words let a caller that gathers key bits with atomics
// keep them where they were measured: k_counterparties.h's CP_ONES.
enum : u32 {
    SEL_TOTAL = 0,    // M: the keys
    SEL_RANK = 1,     // the selected key is the SEL_RANK-th smallest (from 1) among the keys with the prefix
    SEL_DONE = 2,     // the prefix is final: every key at or below it is wanted
    SEL_SCANS = 3,    // select passes that ran (each one table scan)
    SEL_NKEYS = 4,    // tb_select_collect's counter
    SEL_PREFIX = 5,   // [SEL_KEY_WORDS_MAX] the digits of the selected key chosen so far
    SEL_CALLER = 9,   // [7] the caller's
    SEL_VARIES = 16,  // [SEL_KEY_WORDS_MAX] a set bit: two keys differ there
    SEL_WORDS = 20,
};
#define SEL_STATE_BYTES(words, passes) ((u64)(words) * 8 + (u64)(passes) * SEL_BINS * 4)

__device__ static inline u32 sel_word(u32 pass) { return pass / SEL_WORD_PASSES; }
__device__ static inline u32 sel_shift(u32 pass) { return SEL_BITS * (SEL_WORD_PASSES - 1 - pass % SEL_WORD_PASSES); }

// Whether select pass `pass` has a digit to decide.  The same for every thread of every workgroup.
__device__ static inline bool sel_pass_runs(const u64* st, u32 k, u32 pass) {
    if (st[SEL_TOTAL] <= k || st[SEL_DONE]) return false;
    return ((st[SEL_VARIES + sel_word(pass)] >> sel_shift(pass)) & (SEL_BINS - 1)) != 0;
}

// Whether a is below (LESS) or above (!LESS) b, N words, most significant first.
template <bool LESS, u32 N>
__device__ static inline bool sel_differs(const u64* a, const u64* b) {
    bool is = false, decided = false;
#pragma unroll
    for (u32 q = 0; q < N; q++) {
        if (!decided && a[q] != b[q]) is = LESS ? a[q] < b[q] : a[q] > b[q], decided = true;
    }
    return is;
}

template <typename SRC>
__global__ __launch_bounds__(QUERY_THREADS) void tb_select_hist(SRC S, const u32* counts, u64 nblocks, u32 k, u32 pass, const u64* st,
                                                                u32* hist) {
    __shared__ u32 s_hist[SEL_BINS];
    if (!sel_pass_runs(st, k, pass)) return;
    for (u32 i = threadIdx.x; i < SEL_BINS; i += QUERY_THREADS) s_hist[i] = 0;
    __syncthreads();
    u64 prefix[SRC::WORDS];
#pragma unroll
    for (u32 q = 0; q < SRC::WORDS; q++) prefix[q] = st[SEL_PREFIX + q];
    const u32 w = sel_word(pass), shift = sel_shift(pass), above = shift + SEL_BITS;
    bool any = false;
    for (u32 t = 0; t < SEL_TILES; t++) {
        const u64 b = (u64)blockIdx.x * SEL_TILES + t;
        if (b >= nblocks || counts[b] == 0) continue;  // the whole workgroup alike
        any = true;
        u64 K[SRC::WORDS];
        if (!S.key(b * QUERY_THREADS + threadIdx.x, K)) continue;
        bool has = above >= 64 || (K[w] >> above) == (prefix[w] >> above);  // the digits chosen before `pass`
#pragma unroll
        for (u32 q = 0; q < SRC::WORDS; q++) has = has && (q >= w || K[q] == prefix[q]);
        if (has) atomicAdd(&s_hist[(K[w] >> shift) & (SEL_BINS - 1)], 1u);
    }
    if (!any) return;
    __syncthreads();
    u32* out = hist + (u64)pass * SEL_BINS;
    for (u32 i = threadIdx.x; i < SEL_BINS; i += QUERY_THREADS) {
        const u32 c = s_hist[i];
        if (c) __hip_atomic_fetch_add(&out[i], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(1024) void tb_select_pick(u32 k, u32 pass, const u32* hist, u64* st) {
    __shared__ u32 s_wave[1024 / 64];
    static_assert(SEL_BINS == 2 * 1024, "two bins a thread");
    if (!sel_pass_runs(st, k, pass)) return;
    const u32* h = hist + (u64)pass * SEL_BINS;
    const u32 c0 = h[2 * threadIdx.x], c1 = h[2 * threadIdx.x + 1];
    u32 all;
    const u64 before = tb_block_excl_sum(c0 + c1, s_wave, &all);
    const u32 w = sel_word(pass), shift = sel_shift(pass);
    const u64 rank = st[SEL_RANK], prefix = st[SEL_PREFIX + w];
    __syncthreads();  // every thread has read the state before one rewrites it
    if (rank > before && rank <= before + c0 + c1) {
        const bool second = rank > before + c0;
        const u64 digit = 2 * threadIdx.x + second, left = rank - before - (second ? c0 : 0);
        u64 p = (prefix & ~((u64)(SEL_BINS - 1) << shift)) | digit << shift;
        if (left == (second ? c1 : c0)) {
            p |= (1ULL << shift) - 1;
            for (u32 q = w + 1; q < SEL_KEY_WORDS_MAX; q++) st[SEL_PREFIX + q] = ~0ULL;
            st[SEL_DONE] = 1;
        }
        st[SEL_PREFIX + w] = p;
        st[SEL_RANK] = left;
        st[SEL_SCANS] += 1;
    }
}

template <typename SRC>
__global__ __launch_bounds__(QUERY_THREADS) void tb_select_collect(SRC S, const u32* counts, u64 nblocks, u32 k, u64* st, u64* keys) {
    const bool all = st[SEL_TOTAL] <= k;  // every key
    u64 limit[SRC::WORDS];
#pragma unroll
    for (u32 q = 0; q < SRC::WORDS; q++) limit[q] = all ? ~0ULL : st[SEL_PREFIX + q];
    for (u32 t = 0; t < SEL_TILES; t++) {
        const u64 b = (u64)blockIdx.x * SEL_TILES + t;
        if (b >= nblocks || counts[b] == 0) continue;
        const u64 slot = b * QUERY_THREADS + threadIdx.x;
        u64 K[SRC::WORDS];
        if (!S.key(slot, K) || sel_differs<false, SRC::WORDS>(K, limit)) continue;
        const u64 i = atomicAdd((unsigned long long*)&st[SEL_NKEYS], 1ULL);
        if (i < k) {
            u64* dst = keys + i * (SRC::WORDS + 1);
#pragma unroll
            for (u32 q = 0; q < SRC::WORDS; q++) dst[q] = K[q];
            dst[SRC::WORDS] = slot;
        }
    }
}

// For an emit kernel of QUERY_THREADS threads and a workgroup per SEL_EMIT_KEYS entries: the rank by
// counting of entry i = blockIdx.x * SEL_EMIT_KEYS + threadIdx.x / SEL_EMIT_LANES among the n collected
// entries of W key words and the slot, compared whole, into `mine` and the result (whole in each of
// the entry's lanes).  SEL_EMIT_LANES lanes share an entry, each comparing it with its share of a
// staged tile (one serial loop over 8190 entries a lane took most of a query's time); their counts
// meet by shuffles.  A tile's tail, and `mine` for i >= n, is all-ones, which ranks before no entry.
// Every thread of the workgroup calls it.
template <u32 W>
__device__ static inline u32 tb_select_rank(const u64* keys, u32 n, u64 (&mine)[W + 1]) {
    constexpr u32 E = W + 1;
    __shared__ __attribute__((aligned(16))) u64 s_key[QUERY_THREADS][E];
    if (E % 2 == 0) keys = (const u64*)__builtin_assume_aligned(keys, 16);
    const u32 sub = threadIdx.x % SEL_EMIT_LANES, i = blockIdx.x * SEL_EMIT_KEYS + threadIdx.x / SEL_EMIT_LANES;
#pragma unroll
    for (u32 q = 0; q < E; q++) mine[q] = i < n ? keys[(u64)i * E + q] : ~0ULL;
    u32 rank = 0;
    for (u32 t0 = 0; t0 < n; t0 += QUERY_THREADS) {
        const u32 j = t0 + threadIdx.x;
#pragma unroll
        for (u32 q = 0; q < E; q++) s_key[threadIdx.x][q] = j < n ? keys[(u64)j * E + q] : ~0ULL;
        __syncthreads();
#pragma unroll
        for (u32 s = 0; s < QUERY_THREADS / SEL_EMIT_LANES; s++) rank += sel_differs<true, E>(s_key[s * SEL_EMIT_LANES + sub], mine);
        __syncthreads();
    }
#pragma unroll
    for (u32 off = SEL_EMIT_LANES / 2; off > 0; off >>= 1) rank += __shfl_xor(rank, off);
    return rank;
}
