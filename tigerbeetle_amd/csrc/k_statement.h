// k_statement.h — get_account_statements (include/tbgpu.h tbgpu_get_account_statements): for up to
// 4,095 accounts the caller names and a period (t_open, t_close], each account's balances at the
// period's start and at its end, its gross flows in between and its transfer counts.
//
// No reference can answer it; here it is lookup_accounts_at (k_asof.h) asked once instead of twice,
// and with the gross flows that closing minus opening cannot give.  Nothing was stored at commit: one
// scan sorts each live record that names a requested account into one of two zones,
//   zone 0, above t_close:  the four balance effects (tb_balance_effect), k_asof.h's sum at T = t_close;
//   zone 1, in the period:  pending_in, pending_out, posted_in of the record's side, and one transfer,
// and
//   closing = current - zone 0,
//   opening = closing - the period's net: x_pending - x_pending_in + x_pending_out, x_posted - x_posted_in,
// per column modulo 2^128, which is k_asof.h's formula at T = t_open: the period's net effect is
// {pending_in - pending_out, posted_in}, the same rule read by its signs (tb_statement_flows).
//   tb_asof_gather        (k_asof.h, as it is, T = t_close) the owners' records, the found flags, the set;
//   tb_statement_effects  bins[index] += the record's zone sums, for every record above t_open;
//   tb_statement_emit     a lane per request position: a found one writes its 256-byte row at its rank.
// A member of k_account_scan.h's family.  Its own: a bin is 22 words, and the lanes of a wave may hold
// one account in both zones (t_close falls mid-wave), so the combine's key is (index, zone).
#pragma once

#include "k_asof.h"

#define STATEMENT_IDS_MAX 4095u  // TBGPU_STATEMENTS_MAX: 256-B rows in one message body
#define STATEMENT_ROW_BYTES 256u
// A bin, in 64-bit words.  Zone 0, words [0, 8): k_asof.h's bin — {debits_pending, debits_posted,
// credits_pending, credits_posted} effects, low word first.  Zone 1, words [8, 22): per side (debit,
// then credit) {pending_in, pending_out, posted_in} of two words each and the side's transfer count.
#define STATEMENT_ZONE1 8
#define STATEMENT_SIDE_WORDS 7
#define STATEMENT_BIN_WORDS 22
// The set of 4,095 ids has at most 8,192 slots of 32 bits, 32 KB, so it stays as it is in LDS.  The
// claimed bins beside it: 112 of 176 B with a 4-B tag each, 20,160 B — 52,928 B a workgroup at the
// largest set, three workgroups a CU (160 KB of LDS), 24 waves.  176 bins, the most that 64 KB hold,
// leave two workgroups a CU and measured slower on every leg; 40 bins, four workgroups a CU, lose
// the Zipf legs to HBM adds (DESIGN.md 7k has all four measured).
#define STATEMENT_LDS_BINS 112u

// The gross flows of one record on the *_pending and *_posted columns of either of its sides: what
// tb_balance_effect nets, kept apart — effect.pend = pending_in - pending_out, effect.post =
// posted_in — in tb_balance_effect's order of cases.  p: the pending transfer's amount (a post), the
// post's own where that is not resident.
struct StatementFlows {
    u128 pending_in, pending_out, posted_in;
};
__host__ __device__ static inline StatementFlows tb_statement_flows(u32 flags, u128 amount, u128 p) {
    if (tb_effect_is_post(flags)) return {0, p, amount};
    if (flags & TF_PENDING) return {amount, 0, 0};
    if (flags & TF_VOID) return {0, amount, 0};
    return {0, 0, amount};
}

// N.T[self] is the scanned engine.  set: mask + 1 entries (at most 8,192) built by tb_asof_gather;
// ids: the request; bins: [n_ids][STATEMENT_BIN_WORDS], then the flag word {a post's pending transfer
// was not resident} — all zeroed on the stream before the launch.  t_close = 0: no upper end, nothing
// lands in zone 0.  Workgroup b scans tiles [b, b + 1) * CHANGE_TILES of CHANGE_THREADS positions.
// Dynamic LDS: the set's entries, STATEMENT_LDS_BINS bins, their tags.
__global__ __launch_bounds__(CHANGE_THREADS) void tb_statement_effects(NodeTablesArgs N, u32 self, u64 n, u64 t_open, u64 t_close,
                                                                      const u32* set, u32 mask, const u64* ids, u32 n_ids,
                                                                      u64* bins) {
    extern __shared__ __attribute__((aligned(16))) u8 s_lds[];
    u32* s_set = (u32*)s_lds;                // mask + 1 entries
    u64* s_bins = (u64*)(s_set + mask + 1);  // the claimed bins
    u32* s_tags = (u32*)(s_bins + STATEMENT_LDS_BINS * STATEMENT_BIN_WORDS);  // the index each holds
    const u32 lane = threadIdx.x & 63;
    u64* flags = bins + (u64)n_ids * STATEMENT_BIN_WORDS;
    tb_scan_lds_init(s_set, set, mask, s_bins, STATEMENT_LDS_BINS * STATEMENT_BIN_WORDS, s_tags, STATEMENT_LDS_BINS);
    __syncthreads();
    for (u32 t = 0; t < CHANGE_TILES; t++) {
        const u64 tile0 = ((u64)blockIdx.x * CHANGE_TILES + t) * CHANGE_THREADS, pos = tile0 + threadIdx.x;
        if (tile0 >= n) break;  // the whole workgroup alike
        ScanRecord r;
        u128 a[3] = {0, 0, 0};  // zone 0: {pend, post, -}; zone 1: {pending_in, pending_out, posted_in}
        const u64 any = tb_scan_record(N, self, pos, n, t_open, s_set, mask, ids, flags, r, [&](u32 tf, u128 amount, u128 p) {
            if (t_close != 0 && r.ts > t_close) {
                const BalanceEffect e = tb_balance_effect(tf, amount, p);
                a[0] = e.pend, a[1] = e.post;
            } else {
                const StatementFlows f = tb_statement_flows(tf, amount, p);
                a[0] = f.pending_in, a[1] = f.pending_out, a[2] = f.posted_in;
            }
        });
        if (any == 0) continue;  // the whole wave alike
        const u32 zone = t_close != 0 && r.ts > t_close ? 0 : 1;
        // The adds, a side at a time: the lanes that hold the same (index, zone) combine, then every
        // first lane adds at once, into the workgroup's LDS bin where the index has claimed one, else
        // into the bin in HBM.
#pragma unroll
        for (u32 side = 0; side < 2; side++) {
            const u32 index = r.idx[side];
            bool adds = index != CHANGE_NONE;
            const u32 my = adds ? index * 2 + zone : CHANGE_NONE;  // (an index is below 4,095)
            u128 v[3] = {adds ? a[0] : (u128)0, adds ? a[1] : (u128)0, adds ? a[2] : (u128)0};
            u32 count = adds ? 1 : 0;  // the lanes summed: zone 1's transfers
            tb_scan_combine<3>(lane, my, adds, v, count);
            if (!adds) continue;
            const u32 at = tb_change_bin_claim(s_tags, STATEMENT_LDS_BINS, index);
            u64* bin = at != CHANGE_NONE ? s_bins + at * STATEMENT_BIN_WORDS : bins + (u64)index * STATEMENT_BIN_WORDS;
            if (zone == 0) {
                tb_atomic_add128(bin + 4 * side, v[0]);
                tb_atomic_add128(bin + 4 * side + 2, v[1]);
            } else {
                u64* dst = bin + STATEMENT_ZONE1 + STATEMENT_SIDE_WORDS * side;
                tb_atomic_add128(dst, v[0]);
                tb_atomic_add128(dst + 2, v[1]);
                tb_atomic_add128(dst + 4, v[2]);
                atomicAdd((unsigned long long*)(dst + 6), (unsigned long long)count);
            }
        }
    }
    // The workgroup's claimed bins go to HBM: a thread per word-pair column and the two counts, the
    // unclaimed bins skipped (tb_atomic_add128 skips a zero sum).
    __syncthreads();
    for (u32 i = threadIdx.x; i < STATEMENT_LDS_BINS * 12; i += CHANGE_THREADS) {
        const u32 b = i / 12, part = i % 12, index = s_tags[b];
        if (index == CHANGE_NONE) continue;
        const u64* src = s_bins + b * STATEMENT_BIN_WORDS;
        u64* dst = bins + (u64)index * STATEMENT_BIN_WORDS;
        if (part < 4) {  // zone 0's four columns
            tb_atomic_add128(dst + 2 * part, tb_u128(src[2 * part], src[2 * part + 1]));
        } else if (part < 10) {  // zone 1's six sums: three a side
            const u32 q = part - 4, o = STATEMENT_ZONE1 + STATEMENT_SIDE_WORDS * (q / 3) + 2 * (q % 3);
            tb_atomic_add128(dst + o, tb_u128(src[o], src[o + 1]));
        } else {  // zone 1's two counts
            const u32 o = STATEMENT_ZONE1 + STATEMENT_SIDE_WORDS * (part - 10) + 6;
            if (src[o]) atomicAdd((unsigned long long*)(dst + o), (unsigned long long)src[o]);
        }
    }
}

// One row of 32 words {id, opening[8], closing[8], the six sums, the two counts} from the account's
// record, the period's sums — `sides`: STATEMENT_SIDE_WORDS a side, the sum of every engine's — and
// the balances at the period's end: opening = closing - {pending_in - pending_out, posted_in} a side.
// Device and host alike: a node's host writes its rows with it; k_series.h's rows are these.
__host__ __device__ static inline void tb_flows_row(const u64* account /* 128-B record */, const u64* sides, const u128 closing[4],
                                                    u64* row) {
    row[0] = account[0], row[1] = account[1];
#pragma unroll
    for (u32 side = 0; side < 2; side++) {
        const u64* z = sides + STATEMENT_SIDE_WORDS * side;
        const u128 pending_in = tb_u128(z[0], z[1]), pending_out = tb_u128(z[2], z[3]), posted_in = tb_u128(z[4], z[5]);
        const u32 c = 2 * side;  // the side's *_pending column; c + 1: its *_posted
        const u128 close_pending = closing[c], close_posted = closing[c + 1];
        const u128 open_pending = close_pending - pending_in + pending_out, open_posted = close_posted - posted_in;
        row[2 + 2 * c] = tb_lo(open_pending), row[3 + 2 * c] = tb_hi(open_pending);
        row[4 + 2 * c] = tb_lo(open_posted), row[5 + 2 * c] = tb_hi(open_posted);
        row[10 + 2 * c] = tb_lo(close_pending), row[11 + 2 * c] = tb_hi(close_pending);
        row[12 + 2 * c] = tb_lo(close_posted), row[13 + 2 * c] = tb_hi(close_posted);
#pragma unroll
        for (u32 q = 0; q < 6; q++) row[18 + 6 * side + q] = z[q];
        row[30 + side] = z[6];
    }
}

// One request position's row from its account's record and its id's bin: closing = current - zone 0.
__host__ __device__ static inline void tb_statement_row(const u64* account /* 128-B record */, const u64* bin, u64* row) {
    u128 closing[4];
#pragma unroll
    for (u32 c = 0; c < 4; c++) closing[c] = tb_u128(account[2 + 2 * c], account[3 + 2 * c]) - tb_u128(bin[2 * c], bin[2 * c + 1]);
    tb_flows_row(account, bin + STATEMENT_ZONE1, closing, row);
}

// Workgroup b answers request positions [b, b + 1) * QUERY_THREADS (tb_scan_emit_rank).
// out: room for `cap` rows of STATEMENT_ROW_BYTES.
__global__ __launch_bounds__(QUERY_THREADS) void tb_statement_emit(const u64* ids, u32 n, const u8* accounts, const u32* found,
                                                                   const u32* set, u32 mask, const u64* bins, u32 cap, u8* out,
                                                                   u64* res) {
    u32 rank, total;
    const bool have = tb_scan_emit_rank(found, n, rank, total);
    const u32 i = blockIdx.x * QUERY_THREADS + threadIdx.x;
    if ((blockIdx.x + 1) * QUERY_THREADS >= n && threadIdx.x == 0) {  // the last workgroup: every found position
        res[SCAN_RES_MATCHED] = total;
        res[SCAN_RES_ORPHAN] = bins[(u64)n * STATEMENT_BIN_WORDS];
    }
    if (!have || rank >= cap) return;
    const u64* account = (const u64*)(accounts + (u64)i * 128);
    const u32 index = tb_change_probe(set, mask, ids, account[0], account[1]);  // a found id is in the set
    if (index == CHANGE_NONE) return;
    u64 row[32];
    tb_statement_row(account, bins + (u64)index * STATEMENT_BIN_WORDS, row);
    ulonglong2* dst = (ulonglong2*)(out + (u64)rank * STATEMENT_ROW_BYTES);
#pragma unroll
    for (u32 q = 0; q < 16; q++) dst[q] = make_ulonglong2(row[2 * q], row[2 * q + 1]);
}
