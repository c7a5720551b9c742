// k_query_many.h — get_account_transfers_many (include/tbgpu.h tbgpu_get_account_transfers_many): up to
// 64 account filters answered by one read of the transfer log.
//
// One filter's scan (k_query.h) is bound by the log's bytes, so the bytes are shared: every record is
// loaded once and tested against the whole filter set, a 64-bit mask per lane (bit i: filter i).
//   the set         built by the host (query.h query_many_table) and copied into LDS by every
//                   workgroup: an open-addressing table of 128 slots from account id to the mask of
//                   the filters naming it, the masks of the filters that want debits and credits, and
//                   the filters' windows;
//   tb_qm_count     a chunk of `tiles` consecutive tiles of QUERY_THREADS positions per workgroup,
//                   walked in order with the loads of QUERY_MANY_DEPTH tiles in flight: matches per
//                   filter, the smallest and largest timestamp of any hit, whether the chunk's hits
//                   (of all filters, as one sequence) rise with position, and which tiles hold a hit;
//   tb_qm_scan      one workgroup: per filter the exclusive bases over the chunks and the total, and
//                   one word — the union of all hits is in timestamp order over the whole log, which
//                   is sufficient for every filter's own matches to be;
//   tb_qm_scatter   one workgroup per chunk; it exits unless some filter's wanted ranks meet the
//                   chunk's, then walks the chunk's tiles that hold a hit, a filter's running rank in
//                   the lane of its number, and writes each wanted record once per filter.
// A union out of timestamp order (loads, upserts) is answered filter by filter through k_query.h.
// Plain launches: no grid barrier, no spin, no wait on another workgroup; every loop is bounded by
// the grid, the chunk or 64.
#pragma once

#include "k_query.h"

#define QUERY_MANY_FILTERS 64
#define QUERY_MANY_SLOTS 128  // >= 2 x the distinct ids: an empty slot ends every probe
#define QUERY_MANY_TILES 64   // tiles of a chunk (tbgpu_bench_query_many_tiles shrinks it)
#define QUERY_MANY_DEPTH 4    // tiles whose loads are in flight together
static_assert(QUERY_MANY_TILES * QUERY_WAVES <= QUERY_THREADS, "a thread per {tile, wave} of a chunk");
static_assert(QUERY_MANY_TILES <= 64, "a chunk's tiles are one u64 of bits");

struct QueryManyTable {
    ulonglong2 id[QUERY_MANY_SLOTS];  // {lo, hi}; {0, 0}: empty (never a valid filter's id)
    u64 mask[QUERY_MANY_SLOTS];       // the filters naming the id
    u64 ts_min[QUERY_MANY_FILTERS], ts_max[QUERY_MANY_FILTERS];  // inclusive; ts_max = ~0: open
    u32 k[QUERY_MANY_FILTERS];        // records wanted
    u64 debits, credits, reversed;    // the filters that want the debit side, the credit side, newest first
    u64 windows;                      // != 0: some filter has a window
};
static_assert(sizeof(QueryManyTable) % 8 == 0, "copied into LDS by words");

__host__ __device__ static inline u32 tb_qm_slot(u64 lo, u64 hi) {
    return (u32)(((lo ^ (hi * 0x9E3779B97F4A7C15ULL)) * 0xD6E8FEB86659FD93ULL) >> 57) & (QUERY_MANY_SLOTS - 1);
}

__device__ static inline void tb_qm_load_table(QueryManyTable* s, const QueryManyTable* tab) {
    for (u32 i = threadIdx.x; i < sizeof(QueryManyTable) / 8; i += QUERY_THREADS) ((u64*)s)[i] = ((const u64*)tab)[i];
}

__device__ static inline u64 tb_qm_lookup(const QueryManyTable* s, u64 lo, u64 hi) {
    u32 h = tb_qm_slot(lo, hi);
    for (u32 i = 0; i < QUERY_MANY_SLOTS; i++) {
        const ulonglong2 e = s->id[h];
        if ((e.x | e.y) == 0) return 0;
        if (e.x == lo && e.y == hi) return s->mask[h];
        h = (h + 1) & (QUERY_MANY_SLOTS - 1);
    }
    return 0;
}

// The filters the record at `pos` answers: tb_query_hit for the whole set.  The account on a wanted
// side, the timestamp in the filter's window, and — once, whatever the number of bits — live.
__device__ static inline u64 tb_qm_hit(const Tables& T, const QueryManyTable* s, u64 pos, u64 n, const QueryFields& f) {
    if (pos >= n || f.ts == 0) return 0;
    u64 m = (tb_qm_lookup(s, f.dlo, f.dhi) & s->debits) | (tb_qm_lookup(s, f.clo, f.chi) & s->credits);
    if (m == 0) return 0;
    if (s->windows) {
        for (u64 r = m; r; r &= r - 1) {
            const u32 i = __builtin_ctzll(r);
            if (f.ts < s->ts_min[i] || f.ts > s->ts_max[i]) m &= ~(1ULL << i);
        }
        if (m == 0) return 0;
    }
    const u64* idw = (const u64*)&T.xlog[pos];
    const u64 lo = idw[0], hi = idw[1];
    if (tb_id_reserved(lo, hi)) return 0;
    return tb_transfer_find(T, lo, hi) == (u32)pos ? m : 0;
}

// A value every lane of the wave holds alike, where the compiler can see it.
__device__ static inline u64 tb_qm_uniform(u64 v) {
    const u32 lo = __builtin_amdgcn_readfirstlane((u32)v), hi = __builtin_amdgcn_readfirstlane((u32)(v >> 32));
    return ((u64)hi << 32) | lo;
}

__device__ static inline u64 tb_qm_wave_or(u64 v) {
#pragma unroll
    for (u32 off = 32; off > 0; off >>= 1) v |= __shfl_xor((unsigned long long)v, off);
    return tb_qm_uniform(v);
}

// counts: [chunks][64]; cmin, cmax, cord, ctiles: [chunks].  A chunk without a hit: cmax = 0.
__global__ __launch_bounds__(QUERY_THREADS) void tb_qm_count(Tables T, const QueryManyTable* tab, u64 n, u32 tiles,
                                                             u32* counts, u64* cmin, u64* cmax, u32* cord, u64* ctiles) {
    __shared__ __attribute__((aligned(16))) QueryManyTable s_tab;
    __shared__ u32 s_cnt[QUERY_MANY_FILTERS];
    __shared__ u64 s_segmin[QUERY_THREADS], s_segmax[QUERY_THREADS];  // per {tile, wave} of the chunk, in log order
    __shared__ u64 s_wmin[QUERY_WAVES], s_wmax[QUERY_WAVES];
    __shared__ u64 s_tiles;
    __shared__ u32 s_bad;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    tb_qm_load_table(&s_tab, tab);
    if (threadIdx.x < QUERY_MANY_FILTERS) s_cnt[threadIdx.x] = 0;
    s_segmin[threadIdx.x] = ~0ULL, s_segmax[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_tiles = 0, s_bad = 0;
    __syncthreads();
    const u64 nb = (n + QUERY_THREADS - 1) / QUERY_THREADS;
    const u64 t_first = (u64)blockIdx.x * tiles, t_end = min(nb, t_first + tiles);
    for (u64 t0 = t_first; t0 < t_end; t0 += QUERY_MANY_DEPTH) {
        QueryFields f[QUERY_MANY_DEPTH];
#pragma unroll
        for (u32 j = 0; j < QUERY_MANY_DEPTH; j++) {
            f[j] = QueryFields{0, 0, 0, 0, 0};
            if (t0 + j < t_end) f[j] = tb_query_fields<false, QueryFilter>(T, (t0 + j) * QUERY_THREADS, n, nullptr);
        }
#pragma unroll
        for (u32 j = 0; j < QUERY_MANY_DEPTH; j++) {
            if (t0 + j >= t_end) break;  // the whole workgroup alike
            const u64 m = tb_qm_hit(T, &s_tab, (t0 + j) * QUERY_THREADS + threadIdx.x, n, f[j]);
            if (__ballot(m != 0) == 0) continue;  // the wave alike
            const u64 ts = f[j].ts;
            // The largest hit timestamp at the lanes before this one, as tb_query_count.
            u64 incl = m ? ts : 0;
#pragma unroll
            for (u32 off = 1; off < 64; off <<= 1) {
                const u64 o = __shfl_up((unsigned long long)incl, off);
                if (lane >= off && o > incl) incl = o;
            }
            u64 before = __shfl_up((unsigned long long)incl, 1);
            if (lane == 0) before = 0;
            const u64 bad = __ballot(m != 0 && ts <= before);
            u64 lo = m ? ts : ~0ULL;
#pragma unroll
            for (u32 off = 32; off > 0; off >>= 1) {
                const u64 o = __shfl_xor((unsigned long long)lo, off);
                if (o < lo) lo = o;
            }
            const u32 local = (u32)(t0 + j - t_first);
            if (lane == 63) s_segmax[local * QUERY_WAVES + wave] = incl;
            if (lane == 0) {
                s_segmin[local * QUERY_WAVES + wave] = lo;
                if (bad) s_bad = 1;
                atomicOr((unsigned long long*)&s_tiles, 1ULL << local);
            }
            for (u64 r = tb_qm_wave_or(m); r; r &= r - 1) {
                const u32 bit = __builtin_ctzll(r);
                const u32 c = __popcll(__ballot((m >> bit) & 1));
                if (lane == 0) atomicAdd(&s_cnt[bit], c);
            }
        }
    }
    __syncthreads();
    // The chunk's order: a segment's smallest hit above every earlier segment's largest.
    const u64 mn = s_segmin[threadIdx.x], mx = s_segmax[threadIdx.x];
    u64 incl = mx;
#pragma unroll
    for (u32 off = 1; off < 64; off <<= 1) {
        const u64 o = __shfl_up((unsigned long long)incl, off);
        if (lane >= off && o > incl) incl = o;
    }
    u64 seen = __shfl_up((unsigned long long)incl, 1);
    if (lane == 0) seen = 0;
    u64 lo = mn;
#pragma unroll
    for (u32 off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_xor((unsigned long long)lo, off);
        if (o < lo) lo = o;
    }
    if (lane == 63) s_wmax[wave] = incl;
    if (lane == 0) s_wmin[wave] = lo;
    __syncthreads();
    for (u32 w = 0; w < wave; w++) seen = max(seen, s_wmax[w]);
    const int bad = __syncthreads_or((mx != 0 && mn <= seen) || s_bad != 0);
    if (threadIdx.x < QUERY_MANY_FILTERS) counts[(u64)blockIdx.x * QUERY_MANY_FILTERS + threadIdx.x] = s_cnt[threadIdx.x];
    if (threadIdx.x == 0) {
        u64 a = ~0ULL, b = 0;
        for (u32 w = 0; w < QUERY_WAVES; w++) a = min(a, s_wmin[w]), b = max(b, s_wmax[w]);
        cmin[blockIdx.x] = a;
        cmax[blockIdx.x] = b;
        cord[blockIdx.x] = !bad;
        ctiles[blockIdx.x] = s_tiles;
    }
}

// res: the filters' totals, `ordered`, then where each filter's records start in `out` and their sum.
#define QM_RES_ORDERED QUERY_MANY_FILTERS
#define QM_RES_START (QUERY_MANY_FILTERS + 1)
#define QM_RES_RECORDS (2 * QUERY_MANY_FILTERS + 1)
#define QM_RES_WORDS (2 * QUERY_MANY_FILTERS + 2)

// One workgroup; lane = filter, wave = one of 16 runs of chunks.  base[c][f] = filter f's matches
// before chunk c, res[f] = its total, res[QM_RES_ORDERED] = 1 when the union of all hits is in
// timestamp order over the whole log (tb_query_scan's test over the chunks).  The answers lie packed
// in `out`, so that one copy brings them over: res[QM_RES_START + f] = the records of the filters
// before f, min(k, total) each, and res[QM_RES_RECORDS] = all of them.
__global__ __launch_bounds__(1024) void tb_qm_scan(const QueryManyTable* tab, const u32* counts, const u64* cmin,
                                                   const u64* cmax, const u32* cord, u64 nc, u32* base, u64* res) {
    __shared__ u32 s_sum[1024 / 64][QUERY_MANY_FILTERS];
    __shared__ u64 s_wmax[1024 / 64];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    {
        const u64 per = (nc + 15) / 16, c0 = min(nc, (u64)wave * per), c1 = min(nc, c0 + per);
        u32 local = 0;
        for (u64 c = c0; c < c1; c++) local += counts[c * QUERY_MANY_FILTERS + lane];
        s_sum[wave][lane] = local;
        __syncthreads();
        u32 run = 0, all = 0;
        for (u32 w = 0; w < 1024 / 64; w++) {
            const u32 v = s_sum[w][lane];
            all += v;
            if (w < wave) run += v;
        }
        for (u64 c = c0; c < c1; c++) {
            base[c * QUERY_MANY_FILTERS + lane] = run;
            run += counts[c * QUERY_MANY_FILTERS + lane];
        }
        if (wave == 0) {
            res[lane] = all;
            const u32 m = min(tab->k[lane], all);
            u32 incl = m;
#pragma unroll
            for (u32 off = 1; off < 64; off <<= 1) {
                const u32 o = __shfl_up(incl, off);
                if (lane >= off) incl += o;
            }
            res[QM_RES_START + lane] = incl - m;
            if (lane == 63) res[QM_RES_RECORDS] = incl;
        }
    }
    const u64 per = (nc + 1023) / 1024;
    const u64 k0 = min(nc, (u64)threadIdx.x * per), k1 = min(nc, k0 + per);
    u64 lmax = 0;
    for (u64 k = k0; k < k1; k++) lmax = max(lmax, cmax[k]);
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
        if (cmax[k]) {
            bad |= !cord[k] || cmin[k] <= seen;
            seen = max(seen, cmax[k]);
        }
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) res[QM_RES_ORDERED] = !bad;
}

// Ordered union: filter f's rank = position among its matches = position by timestamp.  Its first k
// ranks (its last k under REVERSED, newest first) write their record to out[f][0, k); a record that
// answers several filters is written once per filter.  out: the filters' records, packed (tb_qm_scan).
__global__ __launch_bounds__(QUERY_THREADS) void tb_qm_scatter(Tables T, const QueryManyTable* tab, u64 n, u32 tiles,
                                                               const u32* counts, const u32* base, const u64* ctiles,
                                                               const u64* res, u8* out) {
    __shared__ __attribute__((aligned(16))) QueryManyTable s_tab;
    __shared__ u64 s_lo[QUERY_MANY_FILTERS], s_hi[QUERY_MANY_FILTERS], s_total[QUERY_MANY_FILTERS], s_start[QUERY_MANY_FILTERS];
    __shared__ u32 s_w[2][QUERY_WAVES][QUERY_MANY_FILTERS];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 tmask = ctiles[blockIdx.x];
    if (!res[QM_RES_ORDERED] || tmask == 0) return;  // the whole workgroup alike
    // Every wave alike: lane f decides for filter f and keeps its running rank.
    const u64 total = res[lane], kk = min((u64)tab->k[lane], total);
    const u64 lo = ((tab->reversed >> lane) & 1) ? total - kk : 0, hi = lo + kk;
    const u32 c = counts[(u64)blockIdx.x * QUERY_MANY_FILTERS + lane];
    u64 run = base[(u64)blockIdx.x * QUERY_MANY_FILTERS + lane];
    const u64 want = tb_qm_uniform(__ballot(c != 0 && run < hi && run + c > lo));
    if (want == 0) return;
    if (wave == 0) s_lo[lane] = lo, s_hi[lane] = hi, s_total[lane] = total, s_start[lane] = res[QM_RES_START + lane];
    tb_qm_load_table(&s_tab, tab);
    __syncthreads();
    u32 it = 0;
    for (u64 r = tmask; r; r &= r - 1, it ^= 1) {
        const u64 tile0 = ((u64)blockIdx.x * tiles + (u32)__builtin_ctzll(r)) * QUERY_THREADS, pos = tile0 + threadIdx.x;
        const QueryFields f = tb_query_fields<false, QueryFilter>(T, tile0, n, nullptr);
        const u64 m = tb_qm_hit(T, &s_tab, pos, n, f) & want;
        u64 wor = 0;
        u32 mine = 0;  // lane f: the wave's matches of filter f
        if (__ballot(m != 0)) {
            wor = tb_qm_wave_or(m);
            for (u64 q = wor; q; q &= q - 1) {
                const u32 bit = __builtin_ctzll(q);
                const u32 cnt = __popcll(__ballot((m >> bit) & 1));
                if (lane == bit) mine = cnt;
            }
        }
        s_w[it][wave][lane] = mine;
        __syncthreads();  // s_w[it] is written again two tiles on, behind the next tile's barrier
        u32 before = 0, tot = 0;
        for (u32 w = 0; w < QUERY_WAVES; w++) {
            const u32 v = s_w[it][w][lane];
            tot += v;
            if (w < wave) before += v;
        }
        for (u64 q = wor; q; q &= q - 1) {
            const u32 bit = __builtin_ctzll(q);
            const bool has = (m >> bit) & 1;
            const u64 b = __ballot(has);
            const u64 start = __shfl((unsigned long long)(run + before), (int)bit);
            if (!has) continue;
            const u64 rank = start + __popcll(b & ((1ULL << lane) - 1));
            if (rank < s_lo[bit] || rank >= s_hi[bit]) continue;
            const u64 dst = ((s_tab.reversed >> bit) & 1) ? s_total[bit] - 1 - rank : rank;
            if (dst < s_tab.k[bit]) *(Transfer*)(out + (s_start[bit] + dst) * 128) = tb_log_load(T, pos);
        }
        run += tot;
    }
}
