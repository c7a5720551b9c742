// k_query.h — get_account_transfers (include/tbgpu.h tbgpu_get_account_transfers): which resident
// transfers touched one account, by timestamp, under a limit.
//
// The reference keeps debit_account_id / credit_account_id index trees on the transfers groove for
// this query (src/state_machine.zig:140-178).  Here the transfer log is an array of 128-B records in
// HBM whose order is timestamp order (except after a load or an upsert), so the query
// is a scan of 40 bytes of every record followed by an ordered compaction under the limit:
//   tb_query_count    a tile of QUERY_THREADS log positions per workgroup: how many match, their
//                     smallest and largest timestamp, and whether they rise with position;
//   tb_query_scan     one workgroup: the exclusive bases, the total, and whether the whole log's
//                     matches are in timestamp order (every tile ordered, its minimum above the
//                     running maximum);
//   tb_query_scatter  ordered: the matches whose rank falls among the wanted k write their record at
//                     that rank (from the other end under REVERSED); every other workgroup exits;
//   tb_query_keys /   unordered (loads and upserts only): {timestamp, position} keys of the matches
//   tb_query_gather   of a range of tiles that fits the key buffer, a round at a time; the host keeps
//                     the best k and one gather copies their records.
// Plain launches: no grid barrier, no spin, no wait on another workgroup; every loop is bounded by
// the grid or by k.
#pragma once

#include <type_traits>

#include "pass.h"

#define QUERY_THREADS 256
#define QUERY_WAVES (QUERY_THREADS / 64)

struct QueryFields {
    u64 dlo, dhi, clo, chi, ts;
};

// The predicate is a template parameter of the scan (tb_query_fields, tb_query_hit and the kernels
// that call them): a filter names the bytes it reads (Fields) and its test of them (pass); the
// window, the liveness probe and everything after the test are shared.
struct QueryFilter {  // get_account_transfers: one account on the wanted sides
    typedef QueryFields Fields;
    u64 id_lo, id_hi;
    u64 ts_min, ts_max;  // inclusive; ts_max = ~0: no upper bound
    u32 debits, credits;
    __device__ bool pass(const QueryFields& f) const {
        return (debits && f.dlo == id_lo && f.dhi == id_hi) || (credits && f.clo == id_lo && f.chi == id_hi);
    }
};

struct QueryFieldVals {
    u64 u128_lo, u128_hi, u64v, ts;
    u32 u32v, ledger, code;
};

// query_transfers / query_accounts (k_query_filter.h): every non-zero field equals the stored one.
struct QueryFieldFilter {
    typedef QueryFieldVals Fields;
    u64 u128_lo, u128_hi, u64v;
    u64 ts_min, ts_max;  // as above
    u32 u32v, ledger, code;
    __host__ __device__ bool wants_u128() const { return (u128_lo | u128_hi) != 0; }
    __device__ bool pass(const QueryFieldVals& f) const {
        return (!wants_u128() || (f.u128_lo == u128_lo && f.u128_hi == u128_hi)) && (!u64v || f.u64v == u64v) &&
               (!u32v || f.u32v == u32v) && (!ledger || f.ledger == ledger) && (!code || f.code == code);
    }
};

// get_pending_transfers (k_pending.h): the records whose flags say `pending`, with an account on a
// wanted side if one is named, whose state at `now` is among the wanted ones.  The state bits are
// TBGPU_PENDING_* (include/tbgpu.h).
#define PENDING_OPEN (1u << 4)
#define PENDING_EXPIRED (1u << 5)
#define PENDING_POSTED (1u << 6)
#define PENDING_VOIDED (1u << 7)
#define PENDING_STATES (PENDING_OPEN | PENDING_EXPIRED | PENDING_POSTED | PENDING_VOIDED)

struct QueryPendingFields {
    u64 ts;
    u32 timeout, flags;
};

struct QueryPendingFilter {
    typedef QueryPendingFields Fields;
    u64 id_lo, id_hi;    // 0 (both words): any account
    u64 ts_min, ts_max;  // as above
    u64 now;             // the clock for expiry
    u32 debits, credits;
    u32 want;            // PENDING_* bits
    u8* states;          // [k] the kept rows' state, written by the kernel that writes the row
    // The state a post or void arriving at `now` would find (k_validate.h, after its amount checks): the
    // posted byte at the record's own position, then the timeout.  The expiry is a u64 sum that
    // saturates: a wrapped one never expires.
    __device__ u32 state(const QueryPendingFields& f, const u8* xposted, u64 pos) const {
        const u8 st = xposted[pos];
        if (st == POSTED_POSTED) return PENDING_POSTED;
        if (st == POSTED_VOIDED) return PENDING_VOIDED;
        if (f.timeout) {
            u64 expiry = f.ts + (u64)f.timeout * 1000000000ULL;
            if (expiry < f.ts) expiry = ~0ULL;
            if (expiry <= now) return PENDING_EXPIRED;
        }
        return PENDING_OPEN;
    }
    // Called for a record inside the window: the account ids (chunks 1-2) are read only when an
    // account is named, the posted byte only for a pending record that passed it.
    __device__ bool pass(const QueryPendingFields& f, const Tables& T, u64 pos) const {
        if (!(f.flags & TF_PENDING)) return false;
        if ((id_lo | id_hi) != 0) {
            const ulonglong2* c = (const ulonglong2*)&T.xlog[pos];
            bool side = false;
            if (debits) {
                const ulonglong2 d = c[1];
                side = d.x == id_lo && d.y == id_hi;
            }
            if (!side && credits) {
                const ulonglong2 cr = c[2];
                side = cr.x == id_lo && cr.y == id_hi;
            }
            if (!side) return false;
        }
        return (state(f, T.xposted, pos) & want) != 0;
    }
};

// The 40 bytes the test needs of the record at `pos`: both account ids (bytes 16-47) and the
// timestamp (byte 120).  COOP = false: the lane reads its own record (two 16-B loads and one 8-B
// load, 128 B apart from its neighbours').  COOP = true: the wave reads chunks 1, 2 and 7 of its 64
// records with neighbouring lanes on neighbouring chunks and hands them over through LDS.
// The field filter reads chunks 5, 6 and 7 — user_data_128; user_data_64, user_data_32; ledger, code
// and the timestamp, the last word of chunk 7 — three 16-B loads per lane, lane-per-record only.
// The pending filter reads chunks 6 and 7 — the timeout; the flags and the timestamp — two 16-B loads
// per lane, lane-per-record only; what else it needs it reads in its test (QueryPendingFilter::pass).
template <bool COOP, typename F>
__device__ static inline typename F::Fields tb_query_fields(const Tables& T, u64 tile0, u64 n, u64* s_raw) {
    if constexpr (std::is_same<F, QueryPendingFilter>::value) {
        static_assert(!COOP, "the pending filter has no cooperative load shape");
        QueryPendingFields v{0, 0, 0};
        const u64 pos = tile0 + threadIdx.x;
        if (pos < n) {
            const ulonglong2* c = (const ulonglong2*)&T.xlog[pos];
            const ulonglong2 b = c[6], d = c[7];
            v.timeout = (u32)(b.y >> 32), v.flags = (u32)(d.x >> 48), v.ts = tb_log_ts(T, pos, d.y);
        }
        return v;
    } else if constexpr (std::is_same<F, QueryFieldFilter>::value) {
        static_assert(!COOP, "the field filter has no cooperative load shape");
        QueryFieldVals v{0, 0, 0, 0, 0, 0, 0};
        const u64 pos = tile0 + threadIdx.x;
        if (pos < n) {
            const ulonglong2* c = (const ulonglong2*)&T.xlog[pos];
            const ulonglong2 a = c[5], b = c[6], d = c[7];
            v.u128_lo = a.x, v.u128_hi = a.y, v.u64v = b.x, v.u32v = (u32)b.y;
            v.ledger = (u32)d.x, v.code = (u32)(d.x >> 32) & 0xFFFF, v.ts = tb_log_ts(T, pos, d.y);
        }
        return v;
    } else {
    QueryFields f{0, 0, 0, 0, 0};
    if (!COOP) {
        const u64 pos = tile0 + threadIdx.x;
        if (pos < n) {
            const ulonglong2* c = (const ulonglong2*)&T.xlog[pos];
            const ulonglong2 d = c[1], cr = c[2];
            f.ts = tb_log_ts(T, pos, ((const u64*)c)[15]);
            f.dlo = d.x, f.dhi = d.y, f.clo = cr.x, f.chi = cr.y;
        }
        return f;
    }
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 wave0 = tile0 + (u64)wave * 64;
    ulonglong2* s = (ulonglong2*)s_raw + wave * 192;
#pragma unroll
    for (u32 j = 0; j < 3; j++) {
        const u32 idx = j * 64 + lane, r = idx / 3, q = idx % 3;
        ulonglong2 v{0, 0};
        if (wave0 + r < n) v = ((const ulonglong2*)&T.xlog[wave0 + r])[q == 2 ? 7 : q + 1];
        s[idx] = v;
    }
    __syncthreads();
    const ulonglong2 d = s[lane * 3], cr = s[lane * 3 + 1], t = s[lane * 3 + 2];
    f.dlo = d.x, f.dhi = d.y, f.clo = cr.x, f.chi = cr.y, f.ts = t.y;
    // A zero field of a record inside the log: the plane, one coalesced 8-B load per lane.
    if (f.ts == 0 && wave0 + lane < n) f.ts = T.xts[wave0 + lane];
    return f;
    }
}

// Whether the record at `pos` answers the filter: the filter's own test (the account on a wanted
// side; the fields equal), the timestamp in the window, and — only then — live: the id index holds its id at this position (tb_delta_live's test).
// A dead position (a failed event, a withdrawn speculative record, a rolled-back chain member) can
// hold any bytes, so reserved ids never reach the probe.
template <typename F>
__device__ static inline bool tb_query_hit(const Tables& T, const F& flt, u64 pos, u64 n, const typename F::Fields& f) {
    if (pos >= n || f.ts == 0 || f.ts < flt.ts_min || f.ts > flt.ts_max) return false;
    if constexpr (std::is_same<F, QueryPendingFilter>::value) {
        if (!flt.pass(f, T, pos)) return false;
    } else {
        if (!flt.pass(f)) return false;
    }
    const u64* idw = (const u64*)&T.xlog[pos];
    const u64 lo = idw[0], hi = idw[1];
    if (tb_id_reserved(lo, hi)) return false;
    return tb_transfer_find(T, lo, hi) == (u32)pos;
}

template <bool COOP, typename F>
__global__ __launch_bounds__(QUERY_THREADS) void tb_query_count(Tables T, F flt, u64 n, u32* counts, u64* mins,
                                                                u64* maxs, u32* ordered) {
    __shared__ __attribute__((aligned(16))) u64 s_chunks[COOP ? QUERY_WAVES * 192 * 2 : 2];
    __shared__ u64 s_max[QUERY_WAVES], s_min[QUERY_WAVES];
    __shared__ u32 s_cnt[QUERY_WAVES], s_bad[QUERY_WAVES];
    const u64 tile0 = (u64)blockIdx.x * QUERY_THREADS;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const typename F::Fields f = tb_query_fields<COOP, F>(T, tile0, n, s_chunks);
    const bool hit = tb_query_hit(T, flt, tile0 + threadIdx.x, n, f);
    // The largest matched timestamp at the lanes before this one: the wave's prefix maximum.
    u64 incl = hit ? f.ts : 0;
#pragma unroll
    for (u32 off = 1; off < 64; off <<= 1) {
        const u64 o = __shfl_up((unsigned long long)incl, off);
        if (lane >= off && o > incl) incl = o;
    }
    u64 before = __shfl_up((unsigned long long)incl, 1);
    if (lane == 0) before = 0;
    u64 lo = hit ? f.ts : ~0ULL;
#pragma unroll
    for (u32 off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_xor((unsigned long long)lo, off);
        if (o < lo) lo = o;
    }
    const u64 m = __ballot(hit);
    if (lane == 63) s_max[wave] = incl;
    if (lane == 0) {
        s_min[wave] = lo;
        s_cnt[wave] = __popcll(m);
    }
    __syncthreads();
    for (u32 w = 0; w < wave; w++) before = max(before, s_max[w]);
    const u64 bad = __ballot(hit && f.ts <= before);
    if (lane == 0) s_bad[wave] = bad != 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 c = 0, b = 0;
        u64 mn = ~0ULL, mx = 0;
        for (u32 w = 0; w < QUERY_WAVES; w++) {
            c += s_cnt[w];
            b |= s_bad[w];
            mn = min(mn, s_min[w]);
            mx = max(mx, s_max[w]);
        }
        counts[blockIdx.x] = c;
        mins[blockIdx.x] = mn;
        maxs[blockIdx.x] = mx;
        ordered[blockIdx.x] = !b;
    }
}

// One workgroup, each thread a run of tiles (tb_delta_scan_blocks' shape): base[k] = matches before
// tile k, res[0] = the total, res[1] = 1 when the matches are in timestamp order over the whole log.
__global__ __launch_bounds__(1024) void tb_query_scan(const u32* counts, const u64* mins, const u64* maxs, const u32* ordered,
                                                      u64 nblocks, u64* base, u64* res) {
    __shared__ u32 s_wave[1024 / 64];
    __shared__ u64 s_wmax[1024 / 64];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 per = (nblocks + 1023) / 1024;
    const u64 k0 = min(nblocks, (u64)threadIdx.x * per), k1 = min(nblocks, k0 + per);
    u32 local = 0;
    u64 lmax = 0;
    for (u64 k = k0; k < k1; k++) {
        local += counts[k];
        if (counts[k]) lmax = max(lmax, maxs[k]);
    }
    u32 all;
    u64 run = tb_block_excl_sum(local, s_wave, &all);
    // The largest matched timestamp in the runs before this thread's.
    u64 incl = lmax;
#pragma unroll
    for (u32 off = 1; off < 64; off <<= 1) {
        const u64 o = __shfl_up((unsigned long long)incl, off);
        if (lane >= off && o > incl) incl = o;
    }
    u64 seen = __shfl_up((unsigned long long)incl, 1);
    if (lane == 0) seen = 0;
    if (lane == 63) s_wmax[wave] = incl;
    __syncthreads();
    for (u32 w = 0; w < wave; w++) seen = max(seen, s_wmax[w]);
    int bad = 0;
    for (u64 k = k0; k < k1; k++) {
        base[k] = run;
        run += counts[k];
        if (counts[k]) {
            bad |= !ordered[k] || mins[k] <= seen;
            seen = max(seen, maxs[k]);
        }
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        res[0] = all;
        res[1] = !bad;
    }
}

// The lane's rank among its tile's matches.
__device__ static inline u32 tb_query_tile_rank(bool hit, u32* s_cnt) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 m = __ballot(hit);
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    u32 r = __popcll(m & ((1ULL << lane) - 1));
    for (u32 w = 0; w < wave; w++) r += s_cnt[w];
    return r;
}

// Ordered log: rank = position among the matches = position by timestamp.  The first k ranks (the
// last k under `reversed`, newest first) write their whole record to out[0, k).
template <typename F>
__global__ __launch_bounds__(QUERY_THREADS) void tb_query_scatter(Tables T, F flt, u64 n, const u32* counts,
                                                                  const u64* base, const u64* res, u32 k, u32 reversed,
                                                                  u8* out) {
    __shared__ u32 s_cnt[QUERY_WAVES];
    const u64 total = res[0], b0 = base[blockIdx.x], c = counts[blockIdx.x];
    const u64 kk = min((u64)k, total), lo = reversed ? total - kk : 0, hi = lo + kk;
    if (!res[1] || c == 0 || b0 >= hi || b0 + c <= lo) return;  // the whole workgroup alike
    const u64 pos = (u64)blockIdx.x * QUERY_THREADS + threadIdx.x;
    const typename F::Fields f = tb_query_fields<false, F>(T, (u64)blockIdx.x * QUERY_THREADS, n, nullptr);
    const bool hit = tb_query_hit(T, flt, pos, n, f);
    const u64 rank = b0 + tb_query_tile_rank(hit, s_cnt);
    if (!hit || rank < lo || rank >= hi) return;
    const u64 dst = reversed ? total - 1 - rank : rank;
    if (dst < k) {
        *(Transfer*)(out + dst * 128) = tb_log_load(T, pos);
        if constexpr (std::is_same<F, QueryPendingFilter>::value) flt.states[dst] = (u8)flt.state(f, T.xposted, pos);
    }
}

// Unordered log, one round: the matches of tiles [wg0, wg0 + gridDim.x) as {timestamp, position}
// keys, in log order from keys[0]; the host chose the range so that they fit keys_cap.
template <typename F>
__global__ __launch_bounds__(QUERY_THREADS) void tb_query_keys(Tables T, F flt, u64 n, u64 wg0, const u32* counts,
                                                               const u64* base, u64* keys, u64 keys_cap) {
    __shared__ u32 s_cnt[QUERY_WAVES];
    const u64 b = wg0 + blockIdx.x;
    if (counts[b] == 0) return;
    const u64 pos = b * QUERY_THREADS + threadIdx.x;
    const typename F::Fields f = tb_query_fields<false, F>(T, b * QUERY_THREADS, n, nullptr);
    const bool hit = tb_query_hit(T, flt, pos, n, f);
    const u64 rank = base[b] - base[wg0] + tb_query_tile_rank(hit, s_cnt);
    if (hit && rank < keys_cap) {
        keys[2 * rank] = f.ts;
        keys[2 * rank + 1] = pos;
    }
}

// The records at m chosen log positions, in that order.
__global__ __launch_bounds__(QUERY_THREADS) void tb_query_gather(Tables T, const u64* positions, u32 m, u64 n, u8* out) {
    const u32 i = blockIdx.x * QUERY_THREADS + threadIdx.x;
    if (i >= m) return;
    const u64 pos = positions[i];
    if (pos < n) *(Transfer*)(out + (u64)i * 128) = tb_log_load(T, pos);
}
