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
//   the select     M > k only: k_select.h's, over the one-word key v = timestamp - min (v = max -
//                  timestamp under REVERSED, so "smallest" is always the wanted end).  tb_qa_scan starts
//                  it: the prefix zero, and `varies` the span max - min with every bit below its top bit
//                  set, so the passes that run are those whose digit the span reaches;
//   tb_qa_emit     tb_select_rank by {v, slot}; out[rank] = the whole account at that slot, with its
//                  current balances.
// Every scan kernel skips a tile whose count is zero.  Plain launches: no grid barrier, no spin, no
// wait on another workgroup; every loop is bounded by the grid, by k or by a constant.
#pragma once

#include "k_select.h"

#define QA_PASSES SEL_WORD_PASSES  // the key is one word

// Device state of one query, u64 words: the select's, with the matches' bounds beside them.
enum : u32 {
    QA_MIN = SEL_CALLER,      // the matches' smallest timestamp
    QA_MAX = SEL_CALLER + 1,  // ... and largest
    QA_WORDS = SEL_WORDS,
};
#define QA_STATE_BYTES SEL_STATE_BYTES(QA_WORDS, QA_PASSES)

struct QaPred {
    QueryFieldFilter f;
    u32 world, self;  // a node shard answers for the accounts it owns (world 0: no owner test)
    u32 cold;         // a user_data_* field is filtered
};

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
        const u64 span = c ? hi - lo : 0;
        st[SEL_TOTAL] = c;
        st[QA_MIN] = c ? lo : 0;
        st[QA_MAX] = hi;
        st[SEL_PREFIX] = 0;
        st[SEL_RANK] = k;
        st[SEL_VARIES] = span ? ~0ULL >> __clzll(span) : 0;
    }
}

// The select's key source: v of the matching slot.  st: the query's state, for the bounds.
struct QaSource {
    static constexpr u32 WORDS = 1;
    Tables T;
    QaPred P;
    u64 cap;
    u32 reversed;
    const u64* st;
    __device__ bool key(u64 slot, u64 (&K)[WORDS]) const {
        const u64 ts = tb_qa_hit(T, P, slot, cap);
        if (ts == 0) return false;  // before the bounds are read: the collect re-reads them after every atomic
        K[0] = reversed ? st[QA_MAX] - ts : ts - st[QA_MIN];
        return true;
    }
};

__global__ __launch_bounds__(QUERY_THREADS) void tb_qa_emit(Tables T, u64 cap, u32 k, const u64* st, const u64* keys, u8* out) {
    const u32 n = (u32)min((u64)k, st[SEL_NKEYS]);
    if (blockIdx.x * SEL_EMIT_KEYS >= n) return;
    u64 mine[2];  // {v, slot}
    const u32 rank = tb_select_rank<1>(keys, n, mine);
    if (threadIdx.x % SEL_EMIT_LANES == 0 && mine[1] < cap && rank < k) *(Account*)(out + (u64)rank * 128) = tb_account_load(T, (u32)mine[1]);
}
