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
// The scan is modelled on tb_change_effects<u32, true>: the timestamp alone first, the liveness probe
// on a set hit only, the wave's lanes combined before one adds, LDS bins claimed by first use.  What
// differs: a bin is 22 words, not 8, and the lanes of a wave may hold one account in both zones
// (t_close falls mid-wave), so the combine groups by (index, zone).
// Plain launches: no grid barrier, no spin, no wait on another workgroup; every loop is bounded by
// the workgroup's tiles, the set's slots, a workgroup's share of the found flags or the 64 lanes of a
// wave.
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
// What tb_statement_emit leaves in `res`, as tb_asof_emit does.
#define STATEMENT_RES_MATCHED 0
#define STATEMENT_RES_ORPHAN 1
#define STATEMENT_RES_WORDS 2

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
    const Tables& T = N.T[self];
    const u32 lane = threadIdx.x & 63;
    u64* flags = bins + (u64)n_ids * STATEMENT_BIN_WORDS;
    for (u32 i = threadIdx.x; i <= mask; i += CHANGE_THREADS) s_set[i] = set[i];
    for (u32 i = threadIdx.x; i < STATEMENT_LDS_BINS * STATEMENT_BIN_WORDS; i += CHANGE_THREADS) s_bins[i] = 0;
    for (u32 i = threadIdx.x; i < STATEMENT_LDS_BINS; i += CHANGE_THREADS) s_tags[i] = CHANGE_NONE;
    __syncthreads();
    for (u32 t = 0; t < CHANGE_TILES; t++) {
        const u64 tile0 = ((u64)blockIdx.x * CHANGE_TILES + t) * CHANGE_THREADS, pos = tile0 + threadIdx.x;
        if (tile0 >= n) break;  // the whole workgroup alike
        // The timestamp alone first: at or below t_open (every tile of an ordered log's prefix) the
        // ids are never read.
        const u64* w = (const u64*)&T.xlog[pos < n ? pos : 0];
        const u64 ts = pos < n ? tb_log_ts(T, pos, w[15]) : 0;  // the plane: coalesced, beside chunk 7
        const bool wanted = ts > t_open;
        if (__ballot(wanted) == 0) continue;  // the whole wave alike
        const u32 zone = t_close != 0 && ts > t_close ? 0 : 1;
        u32 idx[2] = {CHANGE_NONE, CHANGE_NONE};  // the debit and the credit account's index
        u128 a0 = 0, a1 = 0, a2 = 0;              // zone 0: {pend, post, -}; zone 1: {pending_in, pending_out, posted_in}
        if (wanted) {
            const ulonglong2 d = ((const ulonglong2*)w)[1], c = ((const ulonglong2*)w)[2];
            idx[0] = tb_change_probe(s_set, mask, ids, d.x, d.y);
            idx[1] = tb_change_probe(s_set, mask, ids, c.x, c.y);
        }
        if ((idx[0] & idx[1]) != CHANGE_NONE) {
            // Live: the id index holds this record's id at this position (tb_query_hit's test).
            const u64 lo = w[0], hi = w[1];
            if (tb_id_reserved(lo, hi) || tb_transfer_find(T, lo, hi) != (u32)pos) {
                idx[0] = idx[1] = CHANGE_NONE;
            } else {
                const u128 amount = tb_u128(w[6], w[7]);
                const u32 tf = (u32)(w[14] >> 48);
                u128 p = amount;
                if (tb_effect_is_post(tf) && !tb_pending_amount(N, w[8], w[9], &p)) {
                    atomicOr((unsigned long long*)flags, 1ULL);
                }
                if (zone == 0) {
                    const BalanceEffect e = tb_balance_effect(tf, amount, p);
                    a0 = e.pend, a1 = e.post;
                } else {
                    const StatementFlows f = tb_statement_flows(tf, amount, p);
                    a0 = f.pending_in, a1 = f.pending_out, a2 = f.posted_in;
                }
            }
        }
        // The adds, a side at a time.  The lanes of the wave that hold the same (index, zone) combine
        // before one of them adds, by tb_change_effects' chains: the loop visits each distinct key
        // once and links its lanes, one pointer-jumping pass of six steps sums every chain into its
        // first lane.  Then every first lane adds at once: into the workgroup's LDS bin where the
        // index has claimed one, else into the bin in HBM.
#pragma unroll
        for (u32 side = 0; side < 2; side++) {
            const u32 index = idx[side];
            bool adds = index != CHANGE_NONE;
            const u32 my = adds ? index * 2 + zone : CHANGE_NONE;  // (an index is below 4,095)
            u128 v0 = adds ? a0 : (u128)0, v1 = adds ? a1 : (u128)0, v2 = adds ? a2 : (u128)0;
            u32 count = adds ? 1 : 0;  // the lanes summed: zone 1's transfers
            u32 nxt = lane;            // the next lane of this lane's group; itself: none
            bool chains = false;
            u64 todo = __ballot(adds);
            while (todo) {  // at most 64 rounds: every round clears its leader's bit
                const int leader = __ffsll((unsigned long long)todo) - 1;
                const u32 b = __shfl(my, leader);
                const bool mine = my == b;  // (CHANGE_NONE lanes never equal a leader's key)
                const u64 group = __ballot(mine);
                todo &= ~group;
                if ((group & (group - 1)) == 0) continue;
                chains = true;
                if (mine) {
                    const u64 above = lane == 63 ? 0 : group & ~((2ULL << lane) - 1);
                    if (above) nxt = (u32)__ffsll((unsigned long long)above) - 1;
                    if ((int)lane != leader) adds = false;
                }
            }
            if (chains) {
                // v = the sum of the chain from this lane on: after step s it covers 2^(s+1) lanes.
#pragma unroll
                for (u32 s = 0; s < 6; s++) {
                    const bool has = nxt != lane;
                    const u128 o0 = tb_shfl128(v0, nxt), o1 = tb_shfl128(v1, nxt), o2 = tb_shfl128(v2, nxt);
                    const u32 oc = __shfl(count, nxt);
                    const u32 nn = __shfl(nxt, nxt);
                    if (has) {
                        v0 += o0, v1 += o1, v2 += o2, count += oc;
                        nxt = nn == nxt ? lane : nn;
                    }
                }
            }
            if (!adds) continue;
            const u32 at = tb_change_bin_claim(s_tags, STATEMENT_LDS_BINS, index);
            u64* bin = at != CHANGE_NONE ? s_bins + at * STATEMENT_BIN_WORDS : bins + (u64)index * STATEMENT_BIN_WORDS;
            if (zone == 0) {
                tb_atomic_add128(bin + 4 * side, v0);
                tb_atomic_add128(bin + 4 * side + 2, v1);
            } else {
                u64* dst = bin + STATEMENT_ZONE1 + STATEMENT_SIDE_WORDS * side;
                tb_atomic_add128(dst, v0);
                tb_atomic_add128(dst + 2, v1);
                tb_atomic_add128(dst + 4, v2);
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

// One request position's row from its account's record and its id's bin (the sum of every engine's):
// 32 words {id, opening[8], closing[8], the six sums, the two counts}.  Device and host alike: a node's
// host writes its rows with it.
__host__ __device__ static inline void tb_statement_row(const u64* account /* 128-B record */, const u64* bin, u64* row) {
    row[0] = account[0], row[1] = account[1];
#pragma unroll
    for (u32 side = 0; side < 2; side++) {
        const u64* z1 = bin + STATEMENT_ZONE1 + STATEMENT_SIDE_WORDS * side;
        const u128 pending_in = tb_u128(z1[0], z1[1]), pending_out = tb_u128(z1[2], z1[3]), posted_in = tb_u128(z1[4], z1[5]);
        const u32 c = 2 * side;  // the side's *_pending column; c + 1: its *_posted
        const u128 close_pending = tb_u128(account[2 + 2 * c], account[3 + 2 * c]) - tb_u128(bin[2 * c], bin[2 * c + 1]);
        const u128 close_posted = tb_u128(account[4 + 2 * c], account[5 + 2 * c]) - tb_u128(bin[2 * c + 2], bin[2 * c + 3]);
        const u128 open_pending = close_pending - pending_in + pending_out, open_posted = close_posted - posted_in;
        row[2 + 2 * c] = tb_lo(open_pending), row[3 + 2 * c] = tb_hi(open_pending);
        row[4 + 2 * c] = tb_lo(open_posted), row[5 + 2 * c] = tb_hi(open_posted);
        row[10 + 2 * c] = tb_lo(close_pending), row[11 + 2 * c] = tb_hi(close_pending);
        row[12 + 2 * c] = tb_lo(close_posted), row[13 + 2 * c] = tb_hi(close_posted);
#pragma unroll
        for (u32 q = 0; q < 6; q++) row[18 + 6 * side + q] = z1[q];
        row[30 + side] = z1[6];
    }
}

// Workgroup b answers request positions [b, b + 1) * QUERY_THREADS, ranked as tb_asof_emit ranks
// them: its base is a sum over found[0, b * QUERY_THREADS), so no workgroup waits for another.
// out: room for `cap` rows of STATEMENT_ROW_BYTES.
__global__ __launch_bounds__(QUERY_THREADS) void tb_statement_emit(const u64* ids, u32 n, const u8* accounts, const u32* found,
                                                                   const u32* set, u32 mask, const u64* bins, u32 cap, u8* out,
                                                                   u64* res) {
    __shared__ u32 s_part[QUERY_WAVES];
    __shared__ u32 s_wave[QUERY_WAVES];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 first = blockIdx.x * QUERY_THREADS, i = first + threadIdx.x;
    u32 before = 0;
    for (u32 j = threadIdx.x; j < first; j += QUERY_THREADS) before += found[j];
#pragma unroll
    for (u32 off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off);
    const bool have = i < n && found[i] != 0;
    const u64 mine = __ballot(have);
    if (lane == 0) s_part[wave] = before, s_wave[wave] = (u32)__popcll(mine);
    __syncthreads();
    u32 rank = (u32)__popcll(mine & ((1ULL << lane) - 1));
    u32 total = 0;
    for (u32 w = 0; w < QUERY_WAVES; w++) {
        rank += s_part[w];
        if (w < wave) rank += s_wave[w];
        total += s_part[w] + s_wave[w];
    }
    if (first + QUERY_THREADS >= n && threadIdx.x == 0) {  // the last workgroup: every found position
        res[STATEMENT_RES_MATCHED] = total;
        res[STATEMENT_RES_ORPHAN] = bins[(u64)n * STATEMENT_BIN_WORDS];
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
