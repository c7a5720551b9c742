// k_integral.h — get_account_balance_integrals (include/tbgpu.h tbgpu_get_account_balance_integrals):
// for up to 4,095 accounts the caller names and a period (t_open, t_end], each account's balances at
// the period's start and end and the time integral of each balance over the period — how much was
// held for how long, balance x nanoseconds, what an average daily balance, an interest or an
// overdraft fee starts from.
//
// No reference can answer it; here it is get_account_statements' scan (k_statement.h) with a weighted
// term.  Nothing was stored at commit and the log needs no order:
//   integral = opening * L + the sum of effect(r) * (t_end - r.timestamp) over the period's records,
// L = t_end - t_open, per column modulo 2^192: a record moves the balance from its timestamp to the
// period's end.  One scan sorts each live record that names a requested account into one of two zones,
//   zone 0, above t_end:    the four balance effects (tb_balance_effect), k_asof.h's sum at T = t_end;
//   zone 1, in the period:  the same four effects unweighted, the period's net that `opening` needs,
//                           and the four effects times (t_end - timestamp) as 192-bit values,
// and
//   closing = current - zone 0,  opening = closing - zone 1's net  (modulo 2^128, k_asof.h's formula
//   at t_end and at t_open),     integral = opening * L + zone 1's weighted sums  (modulo 2^192).
// The arithmetic is what is new.  A 128-bit effect times a 64-bit weight is a 192-bit product
// (tb_mul192), and a post or a void releases a hold: its effect on a *_pending column is negative.
// The choice here: a negative contribution is added as its two's complement modulo 2^192 (tb_neg192),
// not kept as a separate out-sum — one 3-word sum a column, a 28-word bin, and the row's
// `opening * L + sum` needs no subtraction.  The true integral is below 2^192 (a balance is below 2^128,
// L below 2^64), so the modular sum is exact wherever the balances the definition walks through are
// the ledger's own; sums wrap and unwrap on the way in registers (tb_add192), in the in-wave combine,
// in the LDS bins and in the HBM bins (tb_atomic_add192) alike, with carries across both word borders.
//   tb_asof_gather        (k_asof.h, as it is, T = t_end) the owners' records, the found flags, the set;
//   tb_integral_effects   bins[index] += the record's zone sums, for every record above t_open;
//   tb_integral_emit      a lane per request position: a found one writes its 256-byte row at its rank.
// A member of k_account_scan.h's family.  Its own: the 28-word bin, and a chain pass that sums a column
// at a time, so that one 128-bit and one 192-bit sum are live at once.
#pragma once

#include "k_asof.h"

#define INTEGRAL_IDS_MAX 4095u  // TBGPU_INTEGRALS_MAX: 256-B rows in one message body
#define INTEGRAL_ROW_BYTES 256u
// A bin, in 64-bit words.  Column c of {debits_pending, debits_posted, credits_pending,
// credits_posted} (side s holds columns 2s and 2s + 1).  Zone 0, words [0, 8): k_asof.h's bin, column
// c's effect at 2c, low word first.  Zone 1's net, words [8, 16): the same layout.  Zone 1's weighted
// sums, words [16, 28): column c's three words at 16 + 3c, low word first.
#define INTEGRAL_ZONE1 8
#define INTEGRAL_WEIGHTED 16
#define INTEGRAL_BIN_WORDS 28
// The set of 4,095 ids has at most 8,192 slots of 32 bits, 32 KB, so it stays as it is in LDS.  The
// claimed bins beside it: 88 of 224 B with a 4-B tag each, 20,064 B — 52,832 B a workgroup at the
// largest set, three workgroups a CU (160 KB of LDS), 24 waves, as tb_statement_effects has.  140
// bins, about the most that 64 KB hold, leave two workgroups a CU and measured slower on every leg
// that reads ids; 56 bins, still three workgroups a CU, lose the Zipf legs to HBM adds (DESIGN.md 7l
// has all three measured).  The macro can be set from the compiler's command line for such a build.
#ifndef INTEGRAL_LDS_BINS
#define INTEGRAL_LDS_BINS 88u
#endif

// A value modulo 2^192, low word first.
struct U192 {
    u64 w0, w1, w2;
};
__host__ __device__ static inline U192 tb_add192(U192 a, U192 b) {
    const u128 lo = (u128)a.w0 + b.w0;
    const u128 mid = (u128)a.w1 + b.w1 + tb_hi(lo);  // either carry may reach the third word
    return {tb_lo(lo), tb_lo(mid), a.w2 + b.w2 + tb_hi(mid)};
}
__host__ __device__ static inline U192 tb_neg192(U192 a) { return tb_add192({~a.w0, ~a.w1, ~a.w2}, {1, 0, 0}); }
// a * w exactly: 128 x 64 -> 192 bits.
__host__ __device__ static inline U192 tb_mul192(u128 a, u64 w) {
    const u128 p0 = (u128)tb_lo(a) * w, p1 = (u128)tb_hi(a) * w;
    const u128 mid = (u128)tb_hi(p0) + tb_lo(p1);
    return {tb_lo(p0), tb_lo(mid), tb_hi(p1) + tb_hi(mid)};  // (below 2^192: the last sum cannot wrap)
}

// p[0..2] += v modulo 2^192, in any order beside other adders, in tb_atomic_add128's style: a word at
// a time, each add's old value says whether it wrapped, and every wrap carries exactly one upward.
// The middle word takes v.w1 plus the low word's carry; that sum can itself wrap (v.w1 = 2^64 - 1 with
// a carry: nothing to add to the middle word, one to the third), and so can the add.  Never both.
__device__ static inline void tb_atomic_add192(u64* p, U192 v) {
    u64 mid = v.w1, top = v.w2;
    if (v.w0) {
        const u64 old = atomicAdd((unsigned long long*)p, (unsigned long long)v.w0);
        const u64 carry = (u64)(old + v.w0 < old);
        mid += carry;
        top += (u64)(mid < carry);
    }
    if (mid) {
        const u64 old = atomicAdd((unsigned long long*)(p + 1), (unsigned long long)mid);
        top += (u64)(old + mid < old);
    }
    if (top) atomicAdd((unsigned long long*)(p + 2), (unsigned long long)top);
}

// Lane `from`'s value (any lane's own when `from` is itself).
__device__ static inline U192 tb_shfl192(U192 v, u32 from) {
    return {(u64)__shfl((unsigned long long)v.w0, (int)from), (u64)__shfl((unsigned long long)v.w1, (int)from),
            (u64)__shfl((unsigned long long)v.w2, (int)from)};
}

// N.T[self] is the scanned engine.  set: mask + 1 entries (at most 8,192) built by tb_asof_gather;
// ids: the request; bins: [n_ids][INTEGRAL_BIN_WORDS], then the flag word {a post's pending transfer
// was not resident} — all zeroed on the stream before the launch.  t_end is not 0.  Workgroup b scans
// tiles [b, b + 1) * CHANGE_TILES of CHANGE_THREADS positions.
// Dynamic LDS: the set's entries, INTEGRAL_LDS_BINS bins, their tags.
__global__ __launch_bounds__(CHANGE_THREADS) void tb_integral_effects(NodeTablesArgs N, u32 self, u64 n, u64 t_open, u64 t_end,
                                                                     const u32* set, u32 mask, const u64* ids, u32 n_ids,
                                                                     u64* bins) {
    extern __shared__ __attribute__((aligned(16))) u8 s_lds[];
    u32* s_set = (u32*)s_lds;                // mask + 1 entries
    u64* s_bins = (u64*)(s_set + mask + 1);  // the claimed bins
    u32* s_tags = (u32*)(s_bins + INTEGRAL_LDS_BINS * INTEGRAL_BIN_WORDS);  // the index each holds
    const u32 lane = threadIdx.x & 63;
    u64* flags = bins + (u64)n_ids * INTEGRAL_BIN_WORDS;
    tb_scan_lds_init(s_set, set, mask, s_bins, INTEGRAL_LDS_BINS * INTEGRAL_BIN_WORDS, s_tags, INTEGRAL_LDS_BINS);
    __syncthreads();
    for (u32 t = 0; t < CHANGE_TILES; t++) {
        const u64 tile0 = ((u64)blockIdx.x * CHANGE_TILES + t) * CHANGE_THREADS, pos = tile0 + threadIdx.x;
        if (tile0 >= n) break;  // the whole workgroup alike
        ScanRecord r;
        u128 a0 = 0, a1 = 0;    // the record's effect on its sides' *_pending and *_posted
        bool released = false;  // a0 is negative: a post or a void releases a hold
        const u64 any = tb_scan_record(N, self, pos, n, t_open, s_set, mask, ids, flags, r, [&](u32 tf, u128 amount, u128 p) {
            const BalanceEffect e = tb_balance_effect(tf, amount, p);
            a0 = e.pend, a1 = e.post;
            released = tb_effect_is_post(tf) || (!(tf & TF_PENDING) && (tf & TF_VOID));  // tb_balance_effect's cases by sign
        });
        if (any == 0) continue;  // the whole wave alike
        const u64 ts = r.ts;
        const u32 zone = ts > t_end ? 0 : 1;
        // The adds, a side at a time: the lanes that hold the same (index, zone) are linked into
        // chains, then every first lane adds at once, into the workgroup's LDS bin where the index
        // has claimed one, else into the bin in HBM.
#pragma unroll
        for (u32 side = 0; side < 2; side++) {
            const u32 index = r.idx[side];
            const bool named = index != CHANGE_NONE;
            bool adds = named;  // after the chains: this lane adds its chain's sum
            const u32 my = adds ? index * 2 + zone : CHANGE_NONE;  // (an index is below 4,095)
            const bool weighted = __ballot(adds && zone == 1) != 0;  // the whole wave alike
            u32 nxt;  // the next lane of this lane's group; itself: none
            const bool chains = tb_scan_link(lane, my, adds, nxt);
            // A column at a time, *_pending then *_posted, so that one 128-bit and one 192-bit sum are
            // live at once: v = the side's effect, x (zone 1) = the effect times (t_end - ts), and after
            // step s of the chain pass both cover 2^(s+1) lanes of the chain from this lane on.
            u32 at = CHANGE_NONE;
            if (adds) at = tb_change_bin_claim(s_tags, INTEGRAL_LDS_BINS, index);
            u64* bin = at != CHANGE_NONE ? s_bins + at * INTEGRAL_BIN_WORDS : bins + (u64)(adds ? index : 0) * INTEGRAL_BIN_WORDS;
#pragma unroll
            for (u32 q = 0; q < 2; q++) {
                const bool negative = q == 0 && released;
                u128 v = named ? (q == 0 ? a0 : a1) : (u128)0;
                U192 x = {0, 0, 0};
                if (named && zone == 1) {
                    x = tb_mul192(negative ? (u128)0 - v : v, t_end - ts);
                    if (negative) x = tb_neg192(x);
                }
                if (chains) {
                    u32 to = nxt;
#pragma unroll
                    for (u32 s = 0; s < 6; s++) {
                        const bool has = to != lane;
                        const u128 o = tb_shfl128(v, to);
                        const u32 nn = __shfl(to, to);
                        if (weighted) {
                            const U192 y = tb_shfl192(x, to);
                            if (has) x = tb_add192(x, y);
                        }
                        if (has) {
                            v += o;
                            to = nn == to ? lane : nn;
                        }
                    }
                }
                if (!adds) continue;
                tb_atomic_add128(bin + (zone == 0 ? 0 : INTEGRAL_ZONE1) + 4 * side + 2 * q, v);
                if (zone == 1) tb_atomic_add192(bin + INTEGRAL_WEIGHTED + 6 * side + 3 * q, x);
            }
        }
    }
    // The workgroup's claimed bins go to HBM: a thread per column sum — eight of two words, four of
    // three — the unclaimed bins skipped (the adds skip a zero sum).
    __syncthreads();
    for (u32 i = threadIdx.x; i < INTEGRAL_LDS_BINS * 12; i += CHANGE_THREADS) {
        const u32 b = i / 12, part = i % 12, index = s_tags[b];
        if (index == CHANGE_NONE) continue;
        const u64* src = s_bins + b * INTEGRAL_BIN_WORDS;
        u64* dst = bins + (u64)index * INTEGRAL_BIN_WORDS;
        if (part < 8) {  // zone 0's four columns, zone 1's four nets
            tb_atomic_add128(dst + 2 * part, tb_u128(src[2 * part], src[2 * part + 1]));
        } else {  // zone 1's four weighted sums
            const u32 o = INTEGRAL_WEIGHTED + 3 * (part - 8);
            tb_atomic_add192(dst + o, {src[o], src[o + 1], src[o + 2]});
        }
    }
}

// One request position's row from its account's record and its id's bin (the sum of every engine's):
// 32 words {id, opening[8], closing[8], integral[12], t_open, t_end}.  Device and host alike: a node's
// host writes its rows with it.
__host__ __device__ static inline void tb_integral_row(const u64* account /* 128-B record */, const u64* bin, u64 t_open, u64 t_end,
                                                       u64* row) {
    row[0] = account[0], row[1] = account[1];
    const u64 length = t_end - t_open;
#pragma unroll
    for (u32 c = 0; c < 4; c++) {
        const u128 closing = tb_u128(account[2 + 2 * c], account[3 + 2 * c]) - tb_u128(bin[2 * c], bin[2 * c + 1]);
        const u128 opening = closing - tb_u128(bin[INTEGRAL_ZONE1 + 2 * c], bin[INTEGRAL_ZONE1 + 2 * c + 1]);
        const u64* x = bin + INTEGRAL_WEIGHTED + 3 * c;
        const U192 integral = tb_add192(tb_mul192(opening, length), {x[0], x[1], x[2]});
        row[2 + 2 * c] = tb_lo(opening), row[3 + 2 * c] = tb_hi(opening);
        row[10 + 2 * c] = tb_lo(closing), row[11 + 2 * c] = tb_hi(closing);
        row[18 + 3 * c] = integral.w0, row[19 + 3 * c] = integral.w1, row[20 + 3 * c] = integral.w2;
    }
    row[30] = t_open, row[31] = t_end;
}

// Workgroup b answers request positions [b, b + 1) * QUERY_THREADS (tb_scan_emit_rank).
// out: room for `cap` rows of INTEGRAL_ROW_BYTES.
__global__ __launch_bounds__(QUERY_THREADS) void tb_integral_emit(const u64* ids, u32 n, const u8* accounts, const u32* found,
                                                                  const u32* set, u32 mask, const u64* bins, u64 t_open, u64 t_end,
                                                                  u32 cap, u8* out, u64* res) {
    u32 rank, total;
    const bool have = tb_scan_emit_rank(found, n, rank, total);
    const u32 i = blockIdx.x * QUERY_THREADS + threadIdx.x;
    if ((blockIdx.x + 1) * QUERY_THREADS >= n && threadIdx.x == 0) {  // the last workgroup: every found position
        res[SCAN_RES_MATCHED] = total;
        res[SCAN_RES_ORPHAN] = bins[(u64)n * INTEGRAL_BIN_WORDS];
    }
    if (!have || rank >= cap) return;
    const u64* account = (const u64*)(accounts + (u64)i * 128);
    const u32 index = tb_change_probe(set, mask, ids, account[0], account[1]);  // a found id is in the set
    if (index == CHANGE_NONE) return;
    u64 row[32];
    tb_integral_row(account, bins + (u64)index * INTEGRAL_BIN_WORDS, t_open, t_end, row);
    ulonglong2* dst = (ulonglong2*)(out + (u64)rank * INTEGRAL_ROW_BYTES);
#pragma unroll
    for (u32 q = 0; q < 16; q++) dst[q] = make_ulonglong2(row[2 * q], row[2 * q + 1]);
}
