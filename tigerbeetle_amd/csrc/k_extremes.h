// k_extremes.h — get_account_balance_extremes (include/tbgpu.h tbgpu_get_account_balance_extremes):
// for up to 4,095 accounts the caller names, a period (t_open, t_end] and a measure — a combination of
// the four balance columns with coefficients -1, 0, +1 — the lowest and the highest value the measure
// reached during the period, when each was first reached, and the measure at both ends.
//
// Every other member of k_account_scan.h's family sums: its combine is commutative and its bins take
// adds in any order.  A running value's extremes depend on the order of the records, so this member's
// combine is an associative operator that does not commute (tb_extreme_compose), and it is composed in
// log order at every level:
//   a wave      the lanes that hold the same account are linked into a chain (tb_scan_link) and the
//               six-step pointer-jumping pass composes each chain into its first lane, the lower lane
//               always the left operand.  A record names two accounts, and an account may sit on the
//               debit side of one lane and the credit side of another, so a wave's 64 records go
//               through the pass as two halves of 32 records x 2 sides, a (record, side) item a lane:
//               items of one account are then in log order by lane, and the halves follow each other;
//   a tile      the waves with a hit apply their groups to the account's claimed LDS bin one wave
//               after the other, a barrier between them; without a bin, to the account's cell of this
//               slab in HBM, which no other workgroup touches;
//   a slab      one workgroup walks its slab of consecutive tiles front to back, and writes its claimed
//               bins to its row of the dense [S][n] element array at its end;
//   the log     tb_extreme_emit folds an account's S elements in slab order.
// Nothing waits on another workgroup: a slab is a workgroup's own, and the fold is the next launch.
// Every composition checks that its right operand starts after its left one ends; a log whose
// positions do not follow its timestamps (tbgpu_load_transfers out of order) raises `unordered`, and
// the host answers by the exact path (query.h).
// Records above t_end are order-free: the measure's step summed per account (zone 0), by the family's
// chains and atomics, as k_integral.h's zone 0.
//   closing = measure(current) - zone 0,  opening = closing - the period's net,
//   low = min(opening, opening + lo),  high = max(opening, opening + hi);  ties go to the earlier.
#pragma once

#include "k_integral.h"
#include "extreme_op.h"

#define EXTREME_IDS_MAX 4095u  // TBGPU_EXTREMES_MAX
#define EXTREME_ROW_BYTES 192u
#define EXTREME_ELEM_WORDS 14u  // an ExtremeElem as it lies in a bin, a cell and the element array
// A bin in LDS: the slab's element so far, then the account's zone 0 sum (three words).
#define EXTREME_ZONE0 14u
#define EXTREME_BIN_WORDS 17u
// The set of 4,095 ids stays 32-bit in LDS (at most 8,192 slots, 32 KB).  Beside it 224 bins of 136 B
// with a 4-B tag each, 31,360 B, and the 64 B of the tile's hit words: 64,192 B at the largest set.  A
// slab walk runs S workgroups, far fewer than the family's one a span, so it is sized for the most
// bins a workgroup can hold, not for workgroups a CU.
#ifndef EXTREME_LDS_BINS
#define EXTREME_LDS_BINS 224u
#endif
#define EXTREME_WAVES (CHANGE_THREADS / 64)
// The most slabs a call is cut into: a lane of the emit folds that many elements one after the other.
#define EXTREME_SLABS_MAX 1024u
// The flag words behind zone 0's sums.
#define EXTREME_FLAG_ORPHAN 0
#define EXTREME_FLAG_UNORDERED 1
#define EXTREME_FLAG_WORDS 2

// coefficient * magnitude as a signed 192-bit value; `negative`: the magnitude stands for its negative.
__host__ __device__ static inline U192 tb_extreme_term(int coef, u128 magnitude, bool negative) {
    U192 x = {0, 0, 0};
    if (coef == 0) return x;
    x.w0 = tb_lo(magnitude), x.w1 = tb_hi(magnitude);
    return (coef < 0) != negative ? tb_neg192(x) : x;
}
// Coefficient c of {debits_pending, debits_posted, credits_pending, credits_posted}: byte c of the
// request's measure, a signed 8-bit value.
__host__ __device__ static inline int tb_extreme_coef(u64 measure, u32 c) { return (int)(int8_t)(u8)(measure >> (8 * c)); }

// The measure's step when a record moves side `side`'s (0: debit, 1: credit) two columns by `e`
// (tb_balance_effect); `released`: e.pend is the negative of a hold that is let go (a post, a void).
// One step a record and side: a post's release and its posting land together.
__host__ __device__ static inline U192 tb_extreme_step(u64 measure, u32 side, BalanceEffect e, bool released) {
    const U192 pend = tb_extreme_term(tb_extreme_coef(measure, 2 * side), released ? (u128)0 - e.pend : e.pend, released);
    return tb_add192(pend, tb_extreme_term(tb_extreme_coef(measure, 2 * side + 1), e.post, false));
}
// The measure of four balance columns, each an unsigned 128-bit value {lo, hi}.
__host__ __device__ static inline U192 tb_extreme_measure_of(u64 measure, const u64* columns) {
    U192 v = {0, 0, 0};
#pragma unroll
    for (u32 c = 0; c < 4; c++) v = tb_add192(v, tb_extreme_term(tb_extreme_coef(measure, c), tb_u128(columns[2 * c], columns[2 * c + 1]), false));
    return v;
}

__device__ static inline ExtremeElem tb_extreme_shfl(const ExtremeElem& e, u32 from) {
    ExtremeElem o;
    o.sum = tb_shfl192(e.sum, from), o.lo = tb_shfl192(e.lo, from), o.hi = tb_shfl192(e.hi, from);
    o.t_lo = __shfl((unsigned long long)e.t_lo, (int)from), o.t_hi = __shfl((unsigned long long)e.t_hi, (int)from);
    o.count = __shfl((unsigned long long)e.count, (int)from);
    o.first_ts = __shfl((unsigned long long)e.first_ts, (int)from), o.last_ts = __shfl((unsigned long long)e.last_ts, (int)from);
    return o;
}

// The chain pass for the operator: afterwards a chain's first lane holds its group's composition in
// lane order.  After step s a lane's element covers the 2^(s+1) lanes of its chain from itself on and
// nxt is the lane behind them, so the lane's own element — the lower lanes — is always the left operand.
__device__ static inline void tb_extreme_chain(u32 lane, u32 nxt, ExtremeElem& e, bool* unordered) {
#pragma unroll
    for (u32 s = 0; s < 6; s++) {
        const bool has = nxt != lane;
        const ExtremeElem o = tb_extreme_shfl(e, nxt);
        const u32 nn = __shfl(nxt, nxt);
        if (has) {
            e = tb_extreme_compose(e, o, unordered);
            nxt = nn == nxt ? lane : nn;
        }
    }
}

// The order-free chain pass over one 192-bit sum (zone 0).
__device__ static inline void tb_extreme_chain_sum(u32 lane, u32 nxt, U192& v) {
#pragma unroll
    for (u32 s = 0; s < 6; s++) {
        const bool has = nxt != lane;
        const U192 o = tb_shfl192(v, nxt);
        const u32 nn = __shfl(nxt, nxt);
        if (has) {
            v = tb_add192(v, o);
            nxt = nn == nxt ? lane : nn;
        }
    }
}

// A cell of the element array while its workgroup walks: read and written past the CU's L1, so that a
// wave reads what an earlier wave of the workgroup, or an earlier lane of its own, wrote.
__device__ static inline ExtremeElem tb_extreme_cell_load(u64* cell) {
    u64 w[EXTREME_ELEM_WORDS];
#pragma unroll
    for (u32 k = 0; k < EXTREME_ELEM_WORDS; k++) w[k] = __hip_atomic_load(cell + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return tb_extreme_load(w);
}
__device__ static inline void tb_extreme_cell_store(u64* cell, const ExtremeElem& e) {
    u64 w[EXTREME_ELEM_WORDS];
    tb_extreme_store(w, e);
#pragma unroll
    for (u32 k = 0; k < EXTREME_ELEM_WORDS; k++) __hip_atomic_store(cell + k, w[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// N.T[self] is the scanned engine — one engine, world = 1.  set: mask + 1 entries (at most 8,192) built
// by tb_asof_gather; ids: the request.  Workgroup b walks tiles [b, b + 1) * slab_tiles of CHANGE_THREADS
// positions, front to back.  elems: [gridDim.x][n_ids][EXTREME_ELEM_WORDS]; zone0: [n_ids][3], then the
// EXTREME_FLAG_WORDS — both zeroed on the stream before the launch.  t_end is not 0.
// Dynamic LDS: the set's entries, EXTREME_LDS_BINS bins, their tags, two rows of EXTREME_WAVES hit words.
__global__ __launch_bounds__(CHANGE_THREADS) void tb_extreme_effects(NodeTablesArgs N, u32 self, u64 n, u64 t_open, u64 t_end,
                                                                    u64 measure, const u32* set, u32 mask, const u64* ids, u32 n_ids,
                                                                    u32 slab_tiles, u64* elems, u64* zone0) {
    extern __shared__ __attribute__((aligned(16))) u8 s_lds[];
    u32* s_set = (u32*)s_lds;                // mask + 1 entries
    u64* s_bins = (u64*)(s_set + mask + 1);  // the claimed bins
    u32* s_tags = (u32*)(s_bins + EXTREME_LDS_BINS * EXTREME_BIN_WORDS);  // the index each holds
    u32* s_hit = s_tags + EXTREME_LDS_BINS;  // [2][EXTREME_WAVES] by the tile's parity: the wave has a record of the period
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64* flags = zone0 + (u64)n_ids * 3;
    u64* cells = elems + (u64)blockIdx.x * n_ids * EXTREME_ELEM_WORDS;  // this slab's row
    tb_scan_lds_init(s_set, set, mask, s_bins, EXTREME_LDS_BINS * EXTREME_BIN_WORDS, s_tags, EXTREME_LDS_BINS);
    __syncthreads();
    for (u32 t = 0; t < slab_tiles; t++) {
        const u64 tile0 = ((u64)blockIdx.x * slab_tiles + t) * CHANGE_THREADS, pos = tile0 + threadIdx.x;
        if (tile0 >= n) break;  // the whole workgroup alike
        ScanRecord r;
        U192 step[2] = {{0, 0, 0}, {0, 0, 0}};  // the measure's step on the debit and on the credit account
        const u64 any = tb_scan_record(N, self, pos, n, t_open, s_set, mask, ids, flags + EXTREME_FLAG_ORPHAN, r,
                                       [&](u32 tf, u128 amount, u128 p) {
                                           const BalanceEffect e = tb_balance_effect(tf, amount, p);
                                           const bool released = tb_effect_is_post(tf) || (!(tf & TF_PENDING) && (tf & TF_VOID));
                                           step[0] = tb_extreme_step(measure, 0, e, released);
                                           step[1] = tb_extreme_step(measure, 1, e, released);
                                       });
        const bool named = any != 0 && (r.idx[0] & r.idx[1]) != CHANGE_NONE;
        const bool above = named && r.ts > t_end, within = named && !above;
        // Zone 0, order-free, a side at a time: chains, then every first lane adds at once.
        if (__ballot(above)) {
#pragma unroll
            for (u32 side = 0; side < 2; side++) {
                const u32 index = r.idx[side];
                bool adds = above && index != CHANGE_NONE;
                U192 v = adds ? step[side] : U192{0, 0, 0};
                u32 nxt;
                if (tb_scan_link(lane, index, adds, nxt)) tb_extreme_chain_sum(lane, nxt, v);
                if (!adds) continue;
                const u32 at = tb_change_bin_claim(s_tags, EXTREME_LDS_BINS, index);
                tb_atomic_add192(at != CHANGE_NONE ? s_bins + at * EXTREME_BIN_WORDS + EXTREME_ZONE0 : zone0 + (u64)index * 3, v);
            }
        }
        // The period's records, in order.  Which waves have one is the tile's: a tile without any goes
        // on at once, a tile with one such wave needs no order among waves, and otherwise the waves
        // with a hit take their turn, a barrier behind each.
        u32* hit = s_hit + (t & 1) * EXTREME_WAVES;
        const bool mine = __ballot(within) != 0;
        if (lane == 0) hit[wave] = mine;
        __syncthreads();
        u32 hits = 0;
#pragma unroll
        for (u32 w = 0; w < EXTREME_WAVES; w++) hits += hit[w];
        if (hits == 0) continue;  // the whole workgroup alike
        for (u32 w = 0; w < EXTREME_WAVES; w++) {
            if (!hit[w]) continue;  // the whole workgroup alike
            if (w == wave) {
                bool unordered = false;
                // Two halves of 32 records: lane l of half h stands for record 32h + l / 2, side l % 2.
#pragma unroll 1
                for (u32 h = 0; h < 2; h++) {
                    const u32 src = 32 * h + (lane >> 1), side = lane & 1;
                    const u32 i0 = __shfl(r.idx[0], src), i1 = __shfl(r.idx[1], src);
                    const u64 ts = __shfl((unsigned long long)r.ts, (int)src);
                    const bool in = __shfl((u32)within, src) != 0;
                    const U192 s0 = tb_shfl192(step[0], src), s1 = tb_shfl192(step[1], src);
                    const u32 index = side ? i1 : i0;
                    bool adds = in && index != CHANGE_NONE;
                    if (__ballot(adds) == 0) continue;  // the whole wave alike
                    ExtremeElem e = adds ? tb_extreme_leaf(side ? s1 : s0, ts) : tb_extreme_empty();
                    u32 nxt;
                    if (tb_scan_link(lane, index, adds, nxt)) tb_extreme_chain(lane, nxt, e, &unordered);
                    if (adds) {  // a group's first lane: the group goes behind what the slab has of the account
                        const u32 at = tb_change_bin_claim(s_tags, EXTREME_LDS_BINS, index);
                        if (at != CHANGE_NONE) {
                            u64* bin = s_bins + at * EXTREME_BIN_WORDS;
                            tb_extreme_store(bin, tb_extreme_compose(tb_extreme_load(bin), e, &unordered));
                        } else {
                            u64* cell = cells + (u64)index * EXTREME_ELEM_WORDS;
                            tb_extreme_cell_store(cell, tb_extreme_compose(tb_extreme_cell_load(cell), e, &unordered));
                        }
                    }
                    __threadfence_block();  // the second half's first lanes read what the first half's wrote
                }
                if (unordered) atomicOr((unsigned long long*)(flags + EXTREME_FLAG_UNORDERED), 1ULL);
            }
            if (hits > 1) __syncthreads();
        }
    }
    // The workgroup's claimed bins: the element behind what the cell holds (an account that lost its
    // claim's race never has both), the zone 0 sum into HBM's.
    __syncthreads();
    for (u32 b = threadIdx.x; b < EXTREME_LDS_BINS; b += CHANGE_THREADS) {
        const u32 index = s_tags[b];
        if (index == CHANGE_NONE) continue;
        const u64* bin = s_bins + b * EXTREME_BIN_WORDS;
        const ExtremeElem e = tb_extreme_load(bin);
        if (e.count) {
            bool unordered = false;
            u64* cell = cells + (u64)index * EXTREME_ELEM_WORDS;
            tb_extreme_cell_store(cell, tb_extreme_compose(tb_extreme_cell_load(cell), e, &unordered));
            if (unordered) atomicOr((unsigned long long*)(flags + EXTREME_FLAG_UNORDERED), 1ULL);
        }
        tb_atomic_add192(zone0 + (u64)index * 3, {bin[EXTREME_ZONE0], bin[EXTREME_ZONE0 + 1], bin[EXTREME_ZONE0 + 2]});
    }
}

// Workgroup b answers request positions [b, b + 1) * QUERY_THREADS (tb_scan_emit_rank): a found one
// folds its account's `slabs` elements in slab order and writes its row at its rank; a fold out of order
// raises zone0's `unordered` word, which the host reads once the launch is over.  out: room for `cap`
// rows of EXTREME_ROW_BYTES.
__global__ __launch_bounds__(QUERY_THREADS) void tb_extreme_emit(const u64* ids, u32 n, const u8* accounts, const u32* found,
                                                                 const u32* set, u32 mask, const u64* elems, u32 slabs,
                                                                 u64* zone0, u64 t_open, u64 t_end, u64 measure, u32 cap, u8* out,
                                                                 u64* res) {
    u32 rank, total;
    const bool have = tb_scan_emit_rank(found, n, rank, total);
    const u32 i = blockIdx.x * QUERY_THREADS + threadIdx.x;
    if ((blockIdx.x + 1) * QUERY_THREADS >= n && threadIdx.x == 0) {  // the last workgroup: every found position
        res[SCAN_RES_MATCHED] = total;
        res[SCAN_RES_ORPHAN] = zone0[(u64)n * 3 + EXTREME_FLAG_ORPHAN];
    }
    if (!have || rank >= cap) return;
    const u64* account = (const u64*)(accounts + (u64)i * 128);
    const u32 index = tb_change_probe(set, mask, ids, account[0], account[1]);  // a found id is in the set
    if (index == CHANGE_NONE) return;
    bool unordered = false;
    ExtremeElem e = tb_extreme_empty();
    for (u32 s = 0; s < slabs; s++) {
        const u64* cell = elems + ((u64)s * n + index) * EXTREME_ELEM_WORDS;
        if (cell[11] == 0) continue;  // an empty element: most slabs of most accounts
        e = tb_extreme_compose(e, tb_extreme_load(cell), &unordered);
    }
    if (unordered) atomicOr((unsigned long long*)(zone0 + (u64)n * 3 + EXTREME_FLAG_UNORDERED), 1ULL);
    const U192 closing = tb_sub192(tb_extreme_measure_of(measure, account + 2), {zone0[(u64)index * 3], zone0[(u64)index * 3 + 1], zone0[(u64)index * 3 + 2]});
    u64 row[EXTREME_ROW_BYTES / 8];
    tb_extreme_row(account[0], account[1], tb_sub192(closing, e.sum), e, t_open, t_end, measure, row);
    ulonglong2* dst = (ulonglong2*)(out + (u64)rank * EXTREME_ROW_BYTES);
#pragma unroll
    for (u32 q = 0; q < EXTREME_ROW_BYTES / 16; q++) dst[q] = make_ulonglong2(row[2 * q], row[2 * q + 1]);
}

