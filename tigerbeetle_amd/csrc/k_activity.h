// k_activity.h — get_active_accounts (include/tbgpu.h tbgpu_get_active_accounts): for a period
// (t_open, t_close] and an optional ledger and code, one 128-byte row per distinct account x the
// period's records name — what x paid (`debits`) and what it was paid (`credits`) — the first k by x,
// by volume or by record count.
//
// k_counterparties.h groups around one subject: a record is a hit when it names the subject, and it
// has one key.  Here there is no subject: every live record of the period is a hit on both of its
// sides.  The group table, tb_cp_claim, tb_cp_merge, the select's start (k_select.h does the rest) and
// the emit are k_counterparties.h's, unchanged (the slot's `to` half holds `debits`, its `from` half
// `credits`; tb_cp_key has the BY_TRANSFERS key); the new kernel is the scan:
//   tb_activity_scan  the record step of tb_cp_scan's shape — the timestamp plane first, with word 14
//                     (ledger and code) from the sector the timestamp field shares, against the filter;
//                     a whole wave is skipped when no lane is in the period and carries the ledger and
//                     the code; only a lane that passes both probes the id index for liveness
//                     (tb_transfer_find) and, a post, reads its pending transfer's amount.  A live lane
//                     has the same three sums for up to two keys {slot, half}: its debit account's
//                     `debits` and its credit account's `credits`, each found or claimed in the group
//                     table under the tag that names this record's field.
//
// The combine.  A wave holds up to 128 keys.  On a uniform log they are all distinct and
// tb_scan_link's loop — one round a distinct key — is pure cost; on a hot pair they are two, and the
// link turns 128 adds into two.  ACT_COMBINE chooses at compile time:
//   0  the claimed LDS bins alone: every keyed lane adds;
//   1  each side linked (tb_scan_combine), as tb_cp_scan does;
//   2  a side is linked only when a cheap test finds repeats: a lane's key against the next lane's,
//      one shuffle and a ballot; at least ACT_LINK_MIN adjacent repeats link the side.
// Chosen: 2, on this measurement (one MI355X, 16,777,216 transfers, the whole log by id, median of 21,
// ms; profiles/activity/combine_<n>.json):
//                uniform, 1M accounts    Zipf    one pair
//   0                  6.066            16.399    2.118
//   1                  6.416            15.560    1.936
//   2                  5.991            16.499    1.964
// It keeps the uniform log at the bins-alone time and gives the hot pair the linked time; it does not
// fire on the Zipf log and leaves the always-linked variant's 5 % there.
//
// Plain launches: no grid barrier, no spin, no wait on another workgroup; every loop is bounded by the
// workgroup's tiles, the table's slots or the wave's 64 lanes.
#pragma once

#include "k_counterparties.h"

#define ACT_ROWS_MAX 8191u  // TBGPU_ACTIVE_ROWS_MAX
#define ACT_ROW_BYTES CP_ROW_BYTES
#ifndef ACT_COMBINE
#define ACT_COMBINE 2
#endif
#ifndef ACT_LINK_MIN
#define ACT_LINK_MIN 16u
#endif
// The orders of tb_cp_key.
#define ACT_BY_ID CP_ORDER_ID
#define ACT_BY_VOLUME CP_ORDER_VOLUME
#define ACT_BY_TRANSFERS CP_ORDER_TRANSFERS

struct ActFilter {
    u64 t_open, t_close;  // the period; t_close = 0: no upper end
    u64 min_lo, min_hi;   // only accounts at or above
    u64 w14_mask, w14;    // word 14 of a matching record under the mask: {ledger, code}, each all-ones or zero in the mask
    u32 sides;            // CP_SIDE_*
};

// Word 14 of a record is {ledger: 32, code: 16, flags: 16}, least significant first.
__host__ __device__ static inline void tb_activity_w14(u32 ledger, u32 code, u64& mask, u64& want) {
    mask = (ledger ? 0xFFFFFFFFULL : 0) | (code ? 0xFFFFULL << 32 : 0);
    want = (u64)ledger | (u64)(code & 0xFFFFu) << 32;
}

// N.T[self] is the scanned engine, n its log's end.  table: mask + 1 slots, st: the state words — both
// zeroed on the stream before the launch.  Workgroup b scans tiles [b, b + 1) * CHANGE_TILES of
// CHANGE_THREADS positions.
__global__ __launch_bounds__(CHANGE_THREADS) void tb_activity_scan(NodeTablesArgs N, u32 self, u64 n, ActFilter F, u64* table, u32 mask,
                                                                  u64* st) {
    __shared__ u64 s_bins[CP_LDS_BINS * CP_FLOW_WORDS];
    __shared__ u32 s_tags[CP_LDS_BINS];  // the {slot, half} each bin holds
    const Tables& T = N.T[self];
    const u32 lane = threadIdx.x & 63;
    for (u32 i = threadIdx.x; i < CP_LDS_BINS * CP_FLOW_WORDS; i += CHANGE_THREADS) s_bins[i] = 0;
    for (u32 i = threadIdx.x; i < CP_LDS_BINS; i += CHANGE_THREADS) s_tags[i] = CHANGE_NONE;
    __syncthreads();
    for (u32 t = 0; t < CHANGE_TILES; t++) {
        const u64 tile0 = ((u64)blockIdx.x * CHANGE_TILES + t) * CHANGE_THREADS, pos = tile0 + threadIdx.x;
        if (tile0 >= n) break;  // the whole workgroup alike
        const u64* w = (const u64*)&T.xlog[pos < n ? pos : 0];
        // Words 14 and 15 in one 16-byte load: {ledger, code, flags} lies in the 32-byte sector the
        // timestamp is read from, so the word-14 test reads nothing the period test did not.
        const ulonglong2 tail = ((const ulonglong2*)w)[7];
        const u64 w14 = tail.x, ts = pos < n ? tb_log_ts(T, pos, tail.y) : 0;  // the plane: coalesced
        const bool wanted = ts > F.t_open && (F.t_close == 0 || ts <= F.t_close) && (w14 & F.w14_mask) == F.w14;
        if (__ballot(wanted) == 0) continue;  // the whole wave alike: nothing but the plane and that sector was read, and no probe ran
        u32 key[2] = {CHANGE_NONE, CHANGE_NONE};  // slot * 2 + half (0: debits, 1: credits)
        u128 v[3] = {0, 0, 0};                    // {posted, pending_in, pending_out}
        if (wanted) {
            const u64 lo = w[0], hi = w[1];
            if (!tb_id_reserved(lo, hi) && tb_transfer_find(T, lo, hi) == (u32)pos) {
                const u128 amount = tb_u128(w[6], w[7]);
                const u32 tf = (u32)(w14 >> 48);
                u128 p = amount;
                if (tb_effect_is_post(tf) && !tb_pending_amount(N, w[8], w[9], &p)) atomicOr((unsigned long long*)&st[CP_ORPHAN], 1ULL);
                const StatementFlows f = tb_statement_flows(tf, amount, p);
                v[0] = f.posted_in, v[1] = f.pending_in, v[2] = f.pending_out;
#pragma unroll
                for (u32 half = 0; half < 2; half++) {
                    if (!(F.sides & (half ? CP_SIDE_CREDITS : CP_SIDE_DEBITS))) continue;
                    const ulonglong2 x = ((const ulonglong2*)w)[1 + half];  // words 2, 3: the debit account; 4, 5: the credit account
                    if (x.y < F.min_hi || (x.y == F.min_hi && x.x < F.min_lo)) continue;
                    const u32 slot = tb_cp_claim(N, table, mask, tb_cp_tag(self, pos, half), x.x, x.y);
                    if (slot == CHANGE_NONE) {
                        atomicOr((unsigned long long*)&st[CP_OVERFLOW], 1ULL);
                    } else {
                        key[half] = slot * 2 + half;
                    }
                }
            }
        }
        // The adds, a side at a time: a side's lanes never share a key with the other side's.
#pragma unroll
        for (u32 half = 0; half < 2; half++) {
            bool adds = key[half] != CHANGE_NONE;
            if (__ballot(adds) == 0) continue;  // the whole wave alike
            u128 a[3] = {v[0], v[1], v[2]};
            u32 count = adds ? 1 : 0;
#if ACT_COMBINE == 1
            tb_scan_combine<3>(lane, key[half], adds, a, count);
#elif ACT_COMBINE == 2
            const u32 next = __shfl(key[half], (int)((lane + 1) & 63));
            if ((u32)__popcll(__ballot(adds && next == key[half])) >= ACT_LINK_MIN) tb_scan_combine<3>(lane, key[half], adds, a, count);
#endif
            if (adds) {
                const u32 at = tb_change_bin_claim(s_tags, CP_LDS_BINS, key[half]);
                u64* bin = at != CHANGE_NONE ? s_bins + at * CP_FLOW_WORDS
                                             : table + (u64)(key[half] >> 1) * CP_SLOT_WORDS + CP_TO + half * CP_FLOW_WORDS;
                tb_cp_add(bin, a, count);
            }
        }
    }
    // The workgroup's claimed bins go to their slots: a thread per sum and per count.
    __syncthreads();
    for (u32 i = threadIdx.x; i < CP_LDS_BINS * 4; i += CHANGE_THREADS) {
        const u32 b = i / 4, part = i % 4, k = s_tags[b];
        if (k == CHANGE_NONE) continue;
        const u64* src = s_bins + b * CP_FLOW_WORDS;
        u64* dst = table + (u64)(k >> 1) * CP_SLOT_WORDS + CP_TO + (k & 1) * CP_FLOW_WORDS;
        if (part < 3) {
            tb_atomic_add128(dst + 2 * part, tb_u128(src[2 * part], src[2 * part + 1]));
        } else if (src[6]) {
            atomicAdd((unsigned long long*)(dst + 6), (unsigned long long)src[6]);
        }
    }
}
