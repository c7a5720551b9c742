// k_query_filter.h — query_accounts (include/tbgpu.h tbgpu_query_accounts): which accounts carry these
// user_data_128 / user_data_64 / user_data_32 / ledger / code values, inside a timestamp window, the
// first k by timestamp (the last k under REVERSED).  query_transfers is k_query.h's scan with
// QueryFieldFilter as its predicate.
//
// The account table is an open-addressing hash table: its slots are in no order, so the k smallest
// timestamps of the matches are SELECTED on the device, in memory that does not grow with the matches:
//   tb_qa_count    a tile of QUERY_THREADS slots per workgroup: how many match, their smallest and
//                  largest timestamp.  The 32-B hot entry decides liveness, owner, ledger, code and
//                  window; the 32-B cold entry is read only under a user_data_* filter, by slots that
//                  passed the hot tests;
//   tb_qa_scan     one workgroup: the total M and the matches' global minimum and maximum;
//   tb_qa_hist /   M > k only: a most-significant-digit radix select of the k-th smallest value of
//   tb_qa_pick     v = timestamp - min (v = max - timestamp under REVERSED, so "smallest" is always
//                  the wanted end), QA_BITS bits a pass.  A pass histograms the digit of the matches
//                  that carry the prefix chosen so far (LDS per workgroup, non-returning global atomics
//                  to merge) and one workgroup picks the digit.  The passes are enqueued back to back;
//                  a pass whose digit the span max - min already decides (it is zero), or any pass
//                  when M <= k, exits on what it reads from device memory;
//   tb_qa_collect  the matches with v <= the selected value append {v, slot} to a k-entry key buffer
//                  through one counter.  Account timestamps are unique, so exactly k qualify; the
//                  store is guarded by index < k all the same;
//   tb_qa_emit     rank by counting: sixteen lanes to a key, the keys staged through LDS a tile at a
//                  time; out[rank] = the whole account at that slot, with its current balances.
// Every scan kernel skips a tile whose count is zero.  Plain launches: no grid barrier, no spin, no
// wait on another workgroup; every loop is bounded by the grid, by k or by a constant.
#pragma once

#include "k_query.h"

#define QA_BITS 11
#define QA_BINS (1u << QA_BITS)
#define QA_PASSES 6  // 6 x 11 bits cover a 64-bit span
#define QA_TILES 4   // tiles one workgroup of tb_qa_hist / tb_qa_collect covers

// Device state of one query, u64 words.
enum : u32 {
    QA_TOTAL = 0,   // M: the matches
    QA_MIN = 1,     // their smallest timestamp
    QA_MAX = 2,     // ... and largest
    QA_PREFIX = 3,  // the digits of the selected value chosen so far
    QA_RANK = 4,    // the selected value is the QA_RANK-th smallest (from 1) among the matches with the prefix
    QA_SCANS = 5,   // select passes that ran (each one table scan)
    QA_NKEYS = 6,   // tb_qa_collect's counter
    QA_WORDS = 8,
};

struct QaPred {
    QueryFieldFilter f;
    u32 world, self;  // a node shard answers for the accounts it owns (world 0: no owner test)
    u32 cold;         // a user_data_* field is filtered
};

__device__ static inline u32 qa_shift(u32 pass) { return QA_BITS * (QA_PASSES - 1 - pass); }

// The matching slot's timestamp, or 0.
__device__ static inline u64 tb_qa_hit(const Tables& T, const QaPred& P, u64 slot, u64 cap) {
    if (slot >= cap) return 0;
    const ulonglong2* e = (const ulonglong2*)&T.acct_hot[slot];
    const ulonglong2 id = e[0], r = e[1];
    const u64 ts = r.y;
    const u32 ledger = (u32)r.x, code = (u32)(r.x >> 32) & 0xFFFF;
    if (ts == 0 || tb_id_reserved(id.x, id.y) || ts < P.f.ts_min || ts > P.f.ts_max) return 0;
    if ((P.f.ledger && ledger != P.f.ledger) || (P.f.code && code != P.f.code)) return 0;
    if (P.world && tb_home(id.x, id.y, P.world) != P.self) return 0;
    if (P.cold) {
        const ulonglong2* c = (const ulonglong2*)&T.acct_cold[slot];
        const ulonglong2 a = c[0], b = c[1];
        if (P.f.wants_u128() && (a.x != P.f.u128_lo || a.y != P.f.u128_hi)) return 0;
        if ((P.f.u64v && b.x != P.f.u64v) || (P.f.u32v && (u32)b.y != P.f.u32v)) return 0;
    }
    return ts;
}

__global__ __launch_bounds__(QUERY_THREADS) void tb_qa_count(Tables T, QaPred P, u64 cap, u32* counts, u64* mins, u64* maxs) {
    __shared__ u64 s_max[QUERY_WAVES], s_min[QUERY_WAVES];
    __shared__ u32 s_cnt[QUERY_WAVES];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 ts = tb_qa_hit(T, P, (u64)blockIdx.x * QUERY_THREADS + threadIdx.x, cap);
    u64 lo = ts ? ts : ~0ULL, hi = ts;
#pragma unroll
    for (u32 off = 32; off > 0; off >>= 1) {
        const u64 a = __shfl_xor((unsigned long long)lo, off), b = __shfl_xor((unsigned long long)hi, off);
        lo = min(lo, a);
        hi = max(hi, b);
    }
    const u64 m = __ballot(ts != 0);
    if (lane == 0) {
        s_min[wave] = lo;
        s_max[wave] = hi;
        s_cnt[wave] = __popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 c = 0;
        u64 mn = ~0ULL, mx = 0;
        for (u32 w = 0; w < QUERY_WAVES; w++) {
            c += s_cnt[w];
            mn = min(mn, s_min[w]);
            mx = max(mx, s_max[w]);
        }
        counts[blockIdx.x] = c;
        mins[blockIdx.x] = mn;
        maxs[blockIdx.x] = mx;
    }
}

// One workgroup, each thread a run of tiles: the state of the select that follows.
__global__ __launch_bounds__(1024) void tb_qa_scan(const u32* counts, const u64* mins, const u64* maxs, u64 nblocks, u32 k,
                                                   u64* st) {
    __shared__ u64 s_cnt[1024 / 64], s_min[1024 / 64], s_max[1024 / 64];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 per = (nblocks + 1023) / 1024;
    const u64 k0 = min(nblocks, (u64)threadIdx.x * per), k1 = min(nblocks, k0 + per);
    u64 c = 0, lo = ~0ULL, hi = 0;
    for (u64 b = k0; b < k1; b++) {
        if (counts[b] == 0) continue;
        c += counts[b];
        lo = min(lo, mins[b]);
        hi = max(hi, maxs[b]);
    }
#pragma unroll
    for (u32 off = 32; off > 0; off >>= 1) {
        c += __shfl_xor((unsigned long long)c, off);
        lo = min(lo, (u64)__shfl_xor((unsigned long long)lo, off));
        hi = max(hi, (u64)__shfl_xor((unsigned long long)hi, off));
    }
    if (lane == 0) {
        s_cnt[wave] = c;
        s_min[wave] = lo;
        s_max[wave] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        c = 0, lo = ~0ULL, hi = 0;
        for (u32 w = 0; w < 1024 / 64; w++) {
            c += s_cnt[w];
            lo = min(lo, s_min[w]);
            hi = max(hi, s_max[w]);
        }
        st[QA_TOTAL] = c;
        st[QA_MIN] = c ? lo : 0;
        st[QA_MAX] = hi;
        st[QA_PREFIX] = 0;
        st[QA_RANK] = k;
        st[QA_SCANS] = 0;
        st[QA_NKEYS] = 0;
    }
}

// Whether select pass `pass` has a digit to decide: more matches than wanted, and a span that
// reaches the digit.  The same for every thread of every workgroup of the pass.
__device__ static inline bool qa_pass_runs(const u64* st, u32 k, u32 pass) {
    return st[QA_TOTAL] > k && ((st[QA_MAX] - st[QA_MIN]) >> qa_shift(pass)) != 0;
}

__device__ static inline u64 qa_value(const u64* st, u32 reversed, u64 ts) {
    return reversed ? st[QA_MAX] - ts : ts - st[QA_MIN];
}

// Whether v carries the digits chosen before `pass`.
__device__ static inline bool qa_has_prefix(u64 v, u64 prefix, u32 pass) {
    const u32 above = qa_shift(pass) + QA_BITS;
    return above >= 64 || (v >> above) == (prefix >> above);
}

__global__ __launch_bounds__(QUERY_THREADS) void tb_qa_hist(Tables T, QaPred P, u64 cap, const u32* counts, u64 nblocks, u32 k,
                                                            u32 reversed, u32 pass, const u64* st, u32* hist) {
    __shared__ u32 s_hist[QA_BINS];
    if (!qa_pass_runs(st, k, pass)) return;
    for (u32 i = threadIdx.x; i < QA_BINS; i += QUERY_THREADS) s_hist[i] = 0;
    __syncthreads();
    const u64 prefix = st[QA_PREFIX];
    const u32 shift = qa_shift(pass);
    bool any = false;
    for (u32 t = 0; t < QA_TILES; t++) {
        const u64 b = (u64)blockIdx.x * QA_TILES + t;
        if (b >= nblocks || counts[b] == 0) continue;  // the whole workgroup alike
        any = true;
        const u64 ts = tb_qa_hit(T, P, b * QUERY_THREADS + threadIdx.x, cap);
        if (ts == 0) continue;
        const u64 v = qa_value(st, reversed, ts);
        if (qa_has_prefix(v, prefix, pass)) atomicAdd(&s_hist[(v >> shift) & (QA_BINS - 1)], 1u);
    }
    if (!any) return;
    __syncthreads();
    u32* out = hist + (u64)pass * QA_BINS;
    for (u32 i = threadIdx.x; i < QA_BINS; i += QUERY_THREADS) {
        const u32 c = s_hist[i];
        if (c) __hip_atomic_fetch_add(&out[i], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One workgroup: the digit under which the QA_RANK-th smallest value falls.
__global__ __launch_bounds__(1024) void tb_qa_pick(u32 k, u32 pass, const u32* hist, u64* st) {
    __shared__ u32 s_wave[1024 / 64];
    static_assert(QA_BINS == 2 * 1024, "two bins a thread");
    if (!qa_pass_runs(st, k, pass)) return;
    const u32* h = hist + (u64)pass * QA_BINS;
    const u32 c0 = h[2 * threadIdx.x], c1 = h[2 * threadIdx.x + 1];
    u32 all;
    const u64 before = tb_block_excl_sum(c0 + c1, s_wave, &all);
    const u64 rank = st[QA_RANK], prefix = st[QA_PREFIX];
    __syncthreads();  // every thread has read the state before one rewrites it
    if (rank > before && rank <= before + c0 + c1) {
        const bool second = rank > before + c0;
        st[QA_PREFIX] = prefix | ((u64)(2 * threadIdx.x + second) << qa_shift(pass));
        st[QA_RANK] = rank - before - (second ? c0 : 0);
        st[QA_SCANS] += 1;
    }
}

__global__ __launch_bounds__(QUERY_THREADS) void tb_qa_collect(Tables T, QaPred P, u64 cap, const u32* counts, u64 nblocks,
                                                               u32 k, u32 reversed, u64* st, u64* keys) {
    const u64 limit = st[QA_TOTAL] > k ? st[QA_PREFIX] : ~0ULL;  // the selected value; M <= k: every match
    for (u32 t = 0; t < QA_TILES; t++) {
        const u64 b = (u64)blockIdx.x * QA_TILES + t;
        if (b >= nblocks || counts[b] == 0) continue;
        const u64 slot = b * QUERY_THREADS + threadIdx.x;
        const u64 ts = tb_qa_hit(T, P, slot, cap);
        if (ts == 0) continue;
        const u64 v = qa_value(st, reversed, ts);
        if (v > limit) continue;
        const u64 i = atomicAdd((unsigned long long*)&st[QA_NKEYS], 1ULL);
        if (i < k) {
            keys[2 * i] = v;
            keys[2 * i + 1] = slot;
        }
    }
}

// Rank by counting over the collected keys (at most k): key i goes to out[its rank by {v, slot}].
// QA_EMIT_LANES lanes share a key, each comparing it with its share of a staged tile (one serial loop
// over 8190 keys a lane took most of the query's time); their counts meet by shuffles.  A tile's tail
// is padded with {~0, ~0}, which ranks before no key.
#define QA_EMIT_LANES 16
#define QA_EMIT_KEYS (QUERY_THREADS / QA_EMIT_LANES)
__global__ __launch_bounds__(QUERY_THREADS) void tb_qa_emit(Tables T, u64 cap, u32 k, const u64* st, const u64* keys, u8* out) {
    __shared__ __attribute__((aligned(16))) ulonglong2 s_key[QUERY_THREADS];
    const u32 n = (u32)min((u64)k, st[QA_NKEYS]);
    if (blockIdx.x * QA_EMIT_KEYS >= n) return;
    const ulonglong2* key = (const ulonglong2*)keys;
    const u32 sub = threadIdx.x % QA_EMIT_LANES, i = blockIdx.x * QA_EMIT_KEYS + threadIdx.x / QA_EMIT_LANES;
    const ulonglong2 pad{~0ULL, ~0ULL};
    const ulonglong2 mine = i < n ? key[i] : pad;
    u32 rank = 0;
    for (u32 t0 = 0; t0 < n; t0 += QUERY_THREADS) {
        const u32 j = t0 + threadIdx.x;
        s_key[threadIdx.x] = j < n ? key[j] : pad;
        __syncthreads();
#pragma unroll
        for (u32 s = 0; s < QUERY_THREADS / QA_EMIT_LANES; s++) {
            const ulonglong2 o = s_key[s * QA_EMIT_LANES + sub];
            rank += o.x < mine.x || (o.x == mine.x && o.y < mine.y);
        }
        __syncthreads();
    }
#pragma unroll
    for (u32 off = QA_EMIT_LANES / 2; off > 0; off >>= 1) rank += __shfl_xor(rank, off);
    if (sub == 0 && i < n && rank < k && mine.y < cap) *(Account*)(out + (u64)rank * 128) = tb_account_load(T, (u32)mine.y);
}
