// k_matrix.h — get_account_flow_matrix (include/tbgpu.h tbgpu_get_account_flow_matrix): for a list
// of debit accounts, a list of credit accounts and a period (t_open, t_close], what every debit
// account paid every credit account — one 96-byte cell per pair, dense and row-major.
//
// No reference can answer it.  The other members of k_account_scan.h's family key a record by one
// account, once per side; here the key is the pair, a record has one key, and it has one only when
// both of its sides are asked for, each on its own list:
//   tb_asof_gather     (k_asof.h, as it is, T = t_close) over the two lists laid end to end, the debit
//                      ids first: the found flags of every position and one set, an id's index being
//                      the smallest position that names it in either list;
//   the maps           row_of[index] and col_of[index], 16 bits each: the first debit position and the
//                      first credit position that name the id, MATRIX_NONE where that list does not.
//                      The host builds them from the ids alone (account_scan_host.h scan_pair_maps);
//   tb_matrix_effects  bins[row * n_credit + col] += the record's gross flows and one transfer, for
//                      every live record of the period whose debit id has a row and whose credit id
//                      has a column;
//   tb_matrix_emit     a lane per requested pair: one whose two positions are found writes its cell at
//                      (debit rank) * found_credit + (credit rank).
// One set and two maps, not two narrowed sets: a record's two ids are probed against the same 32-bit
// entries whichever list they belong to (an id in both lists, the netting request, is held once), and
// the maps cost 4 bytes a position where a second set costs 4 to 8.  Its own beside the maps: the
// record step (tb_matrix_record) — the upper bound is tested with the lower on the timestamp alone,
// the liveness probe runs only for a pair hit, and the orphan flag rises only there; the combine runs
// once a tile, not once a side.
#pragma once

#include "k_statement.h"

#define MATRIX_CELLS_MAX 4095u     // TBGPU_FLOW_MATRIX_CELLS_MAX: n_debit * n_credit
#define MATRIX_IDS_MAX 4096u       // n_debit + n_credit where their product is at most 4,095: 1 + 4,095
#define MATRIX_CELL_BYTES 96u
#define MATRIX_NONE 0xFFFFu        // a map's entry: the id is not in that list
// A bin, in 64-bit words, in the cell's order: {posted, pending_in, pending_out} of two words each and
// the transfer count.
#define MATRIX_BIN_WORDS 7
// The claimed bins: 60 B each with the tag.  The largest request keeps 8,192 slots of set (32 KB) and
// 4,096 positions of maps (16 KB) in LDS, which leaves 16 KB: 273 bins at most.  256 measured best
// where bins matter most — a square request over the hottest accounts of a skewed log, 3,969 keys a
// workgroup all in use — and level with 128 elsewhere; 64 lose that leg by half and win only the
// longest lists, where they let a third workgroup onto the CU (DESIGN.md 7o has all three measured).
// The macro can be set from the compiler's command line for such a build.
#ifndef MATRIX_LDS_BINS
#define MATRIX_LDS_BINS 256u
#endif
#define MATRIX_EMIT_CHUNK (MATRIX_IDS_MAX / QUERY_THREADS)  // found flags a thread of the emit ranks

__host__ static inline size_t tb_matrix_lds_bytes(u32 slots, u32 n_ids) {
    return (size_t)slots * 4 + (size_t)MATRIX_LDS_BINS * (MATRIX_BIN_WORDS * 8 + 4) + (size_t)n_ids * 4;
}

// The record step of this member.  N.T[self] is the scanned engine, n its log's end.  Returns the
// wave's ballot of the lanes whose timestamp lies in the period — 0, the whole wave alike: nothing but
// the timestamp plane was read.  Otherwise both ids are read where wanted; the credit id is probed only
// where the debit id has a row, and only a record with a row and a column pays the liveness probe
// (tb_query_hit's test).  A live pair hit gets key = row * n_credit + col and calls body(tf, amount, p)
// as tb_scan_record does; *orphan rises only there: a post that names one asked side, or none, or lies
// outside the period never reads its pending transfer.
template <typename BODY>
__device__ static inline u64 tb_matrix_record(const NodeTablesArgs& N, u32 self, u64 pos, u64 n, u64 t_open, u64 t_close,
                                              const u32* s_set, u32 mask, const u64* ids, const u16* s_row, const u16* s_col,
                                              u32 n_credit, u64* orphan, u32& key, BODY body) {
    const Tables& T = N.T[self];
    const u64* w = (const u64*)&T.xlog[pos < n ? pos : 0];
    const u64 ts = pos < n ? tb_log_ts(T, pos, w[15]) : 0;  // the plane: coalesced, beside chunk 7
    const bool wanted = ts > t_open && (t_close == 0 || ts <= t_close);
    key = CHANGE_NONE;
    const u64 any = __ballot(wanted);
    if (any == 0) return 0;
    u32 row = MATRIX_NONE, col = MATRIX_NONE;
    if (wanted) {
        const ulonglong2 d = ((const ulonglong2*)w)[1];
        const u32 di = tb_change_probe(s_set, mask, ids, d.x, d.y);
        if (di != CHANGE_NONE) row = s_row[di];
        if (row != MATRIX_NONE) {
            const ulonglong2 c = ((const ulonglong2*)w)[2];
            const u32 ci = tb_change_probe(s_set, mask, ids, c.x, c.y);
            if (ci != CHANGE_NONE) col = s_col[ci];
        }
    }
    if (row != MATRIX_NONE && col != MATRIX_NONE) {
        const u64 lo = w[0], hi = w[1];
        if (!tb_id_reserved(lo, hi) && tb_transfer_find(T, lo, hi) == (u32)pos) {
            const u128 amount = tb_u128(w[6], w[7]);
            const u32 tf = (u32)(w[14] >> 48);
            u128 p = amount;
            if (tb_effect_is_post(tf) && !tb_pending_amount(N, w[8], w[9], &p)) atomicOr((unsigned long long*)orphan, 1ULL);
            body(tf, amount, p);
            key = row * n_credit + col;
        }
    }
    return any;
}

// N.T[self] is the scanned engine.  set: mask + 1 entries built by tb_asof_gather over ids, the
// n_ids = n_debit + n_credit request ids, debit list first; maps: row_of[n_ids], then col_of[n_ids];
// bins: [n_debit * n_credit][MATRIX_BIN_WORDS] by key, then the flag word {a post in a cell had lost
// its pending transfer} — all zeroed on the stream before the launch.  t_close = 0: no upper end.
// Workgroup b scans tiles [b, b + 1) * CHANGE_TILES of CHANGE_THREADS positions.  Dynamic LDS
// (tb_matrix_lds_bytes): the set's entries, MATRIX_LDS_BINS bins, their tags, the two maps.
__global__ __launch_bounds__(CHANGE_THREADS) void tb_matrix_effects(NodeTablesArgs N, u32 self, u64 n, u64 t_open, u64 t_close,
                                                                   const u32* set, u32 mask, const u64* ids, u32 n_ids,
                                                                   const u16* maps, u32 n_credit, u32 n_keys, u64* bins) {
    extern __shared__ __attribute__((aligned(16))) u8 s_lds[];
    u32* s_set = (u32*)s_lds;                // mask + 1 entries
    u64* s_bins = (u64*)(s_set + mask + 1);  // the claimed bins (mask + 1 is even: 8-B aligned)
    u32* s_tags = (u32*)(s_bins + MATRIX_LDS_BINS * MATRIX_BIN_WORDS);  // the key each holds
    u16* s_row = (u16*)(s_tags + MATRIX_LDS_BINS);                      // n_ids entries
    u16* s_col = s_row + n_ids;                                         // likewise
    const u32 lane = threadIdx.x & 63;
    u64* flags = bins + (u64)n_keys * MATRIX_BIN_WORDS;
    for (u32 i = threadIdx.x; i < 2 * n_ids; i += CHANGE_THREADS) s_row[i] = maps[i];  // both maps: they lie end to end
    tb_scan_lds_init(s_set, set, mask, s_bins, MATRIX_LDS_BINS * MATRIX_BIN_WORDS, s_tags, MATRIX_LDS_BINS);
    __syncthreads();
    for (u32 t = 0; t < CHANGE_TILES; t++) {
        const u64 tile0 = ((u64)blockIdx.x * CHANGE_TILES + t) * CHANGE_THREADS, pos = tile0 + threadIdx.x;
        if (tile0 >= n) break;  // the whole workgroup alike
        u32 key;
        u128 v[3] = {0, 0, 0};  // {posted, pending_in, pending_out}
        const u64 any = tb_matrix_record(N, self, pos, n, t_open, t_close, s_set, mask, ids, s_row, s_col, n_credit, flags, key,
                                         [&](u32 tf, u128 amount, u128 p) {
                                             const StatementFlows f = tb_statement_flows(tf, amount, p);
                                             v[0] = f.posted_in, v[1] = f.pending_in, v[2] = f.pending_out;
                                         });
        if (any == 0) continue;  // the whole wave alike
        // The adds, once: a record has one key.  The lanes that hold the same pair combine, then every
        // first lane adds at once, into the workgroup's LDS bin where the key has claimed one, else
        // into the bin in HBM.
        bool adds = key != CHANGE_NONE && key < n_keys;  // (a key is below n_keys: the maps hold list positions)
        u32 count = adds ? 1 : 0;                        // the lanes summed: the cell's transfers
        tb_scan_combine<3>(lane, key, adds, v, count);
        if (!adds) continue;
        const u32 at = tb_change_bin_claim(s_tags, MATRIX_LDS_BINS, key);
        u64* bin = at != CHANGE_NONE ? s_bins + at * MATRIX_BIN_WORDS : bins + (u64)key * MATRIX_BIN_WORDS;
        tb_atomic_add128(bin, v[0]);
        tb_atomic_add128(bin + 2, v[1]);
        tb_atomic_add128(bin + 4, v[2]);
        atomicAdd((unsigned long long*)(bin + 6), (unsigned long long)count);
    }
    // The workgroup's claimed bins go to HBM: a thread per sum and per count, the unclaimed bins
    // skipped (tb_atomic_add128 skips a zero sum).
    __syncthreads();
    for (u32 i = threadIdx.x; i < MATRIX_LDS_BINS * 4; i += CHANGE_THREADS) {
        const u32 b = i / 4, part = i % 4, key = s_tags[b];
        if (key == CHANGE_NONE) continue;
        const u64* src = s_bins + b * MATRIX_BIN_WORDS;
        u64* dst = bins + (u64)key * MATRIX_BIN_WORDS;
        if (part < 3) {
            tb_atomic_add128(dst + 2 * part, tb_u128(src[2 * part], src[2 * part + 1]));
        } else if (src[6]) {
            atomicAdd((unsigned long long*)(dst + 6), (unsigned long long)src[6]);
        }
    }
}

// One cell of 12 words {debit id, credit id, posted, pending_in, pending_out, transfers, 0} from the
// pair's ids and its bin — the sum of every engine's.  Device and host alike: a node's host writes its
// cells with it.
__host__ __device__ static inline void tb_matrix_cell(const u64* debit_id, const u64* credit_id, const u64* bin, u64* cell) {
    cell[0] = debit_id[0], cell[1] = debit_id[1];
    cell[2] = credit_id[0], cell[3] = credit_id[1];
#pragma unroll
    for (u32 q = 0; q < MATRIX_BIN_WORDS; q++) cell[4 + q] = bin[q];
    cell[11] = 0;
}

// Workgroup b answers the requested pairs [b, b + 1) * QUERY_THREADS, pair j being debit position
// j / n_credit and credit position j % n_credit.  Every workgroup ranks both lists itself, so none waits
// for another: a thread counts the found flags of MATRIX_EMIT_CHUNK consecutive positions of the
// concatenated request (found: [n_debit + n_credit], the debit list first), the workgroup scans the 256
// counts, and s_rank[i] is the found positions before i — of both lists; a credit position's rank is
// that less found_debit = s_rank[n_debit].  out: room for `cap` cells of MATRIX_CELL_BYTES.
__global__ __launch_bounds__(QUERY_THREADS) void tb_matrix_emit(const u64* ids, u32 n_debit, u32 n_credit, const u32* found,
                                                                const u32* set, u32 mask, const u16* maps, const u64* bins,
                                                                u32 cap, u8* out, u64* res) {
    __shared__ u16 s_rank[MATRIX_IDS_MAX + 1];
    __shared__ u32 s_wave[QUERY_WAVES];
    const u32 n = n_debit + n_credit, n_keys = n_debit * n_credit;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 first = threadIdx.x * MATRIX_EMIT_CHUNK;
    u32 mine = 0;
#pragma unroll
    for (u32 k = 0; k < MATRIX_EMIT_CHUNK; k++) mine += first + k < n && found[first + k] != 0;
    u32 incl = mine;  // the wave's inclusive scan of the counts
#pragma unroll
    for (u32 off = 1; off < 64; off <<= 1) {
        const u32 o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    u32 before = incl - mine;
    for (u32 w = 0; w < wave; w++) before += s_wave[w];
#pragma unroll
    for (u32 k = 0; k < MATRIX_EMIT_CHUNK; k++) {
        if (first + k > n) break;
        s_rank[first + k] = (u16)before;  // (position n: every found position)
        if (first + k < n) before += found[first + k] != 0;
    }
    if (threadIdx.x == QUERY_THREADS - 1 && first + MATRIX_EMIT_CHUNK == n) s_rank[n] = (u16)before;  // n = 4,096
    __syncthreads();
    const u32 found_debit = s_rank[n_debit], found_credit = s_rank[n] - found_debit;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        res[SCAN_RES_MATCHED] = (u64)found_debit * found_credit;
        res[SCAN_RES_ORPHAN] = bins[(u64)n_keys * MATRIX_BIN_WORDS];
    }
    const u32 j = blockIdx.x * QUERY_THREADS + threadIdx.x;
    if (j >= n_keys) return;
    const u32 dpos = j / n_credit, cpos = n_debit + j % n_credit;
    if (found[dpos] == 0 || found[cpos] == 0) return;
    const u32 at = s_rank[dpos] * found_credit + (s_rank[cpos] - found_debit);
    if (at >= cap) return;
    const u64* debit_id = ids + 2 * (u64)dpos;
    const u64* credit_id = ids + 2 * (u64)cpos;
    const u32 di = tb_change_probe(set, mask, ids, debit_id[0], debit_id[1]);  // a found id is in the set
    const u32 ci = tb_change_probe(set, mask, ids, credit_id[0], credit_id[1]);
    if (di == CHANGE_NONE || ci == CHANGE_NONE) return;
    const u32 row = maps[di], col = maps[n + ci];
    if (row >= n_debit || col >= n_credit) return;  // (MATRIX_NONE included)
    u64 cell[MATRIX_CELL_BYTES / 8];
    tb_matrix_cell(debit_id, credit_id, bins + ((u64)row * n_credit + col) * MATRIX_BIN_WORDS, cell);
    ulonglong2* dst = (ulonglong2*)(out + (u64)at * MATRIX_CELL_BYTES);
#pragma unroll
    for (u32 q = 0; q < MATRIX_CELL_BYTES / 16; q++) dst[q] = make_ulonglong2(cell[2 * q], cell[2 * q + 1]);
}
