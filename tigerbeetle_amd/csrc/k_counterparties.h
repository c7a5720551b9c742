// k_counterparties.h — get_account_counterparties (include/tbgpu.h tbgpu_get_account_counterparties):
// for one subject account a and a period (t_open, t_close], one 128-byte row per distinct account x
// that a paid or was paid by — what went a -> x (`to`) and x -> a (`from`) — the first k by x, or by
// volume.
//
// The account-set family (k_account_scan.h) probes a set the request fixed and adds into bins the
// request fixed.  Here the caller bounds nothing: the groups are discovered.  Three steps:
//   tb_cp_scan     the record step of tb_matrix_record's shape — the timestamp plane first, a whole
//                  wave skipped when no lane is in the period — with the subject's id compared
//                  directly against the record's two account words (there is no set); the liveness
//                  probe and the P read run only for a hit.  A hit finds or claims its counterparty's
//                  slot in the group table (tb_cp_claim) and adds its flows there: combined across
//                  the lanes of the wave that share a slot and a direction (tb_scan_combine), into a
//                  workgroup LDS bin claimed by {slot, direction} (tb_change_bin_claim), else into the
//                  slot in HBM;
//   the select     the first k of the occupied slots by a multi-word key — {id} by default, {~volume,
//                  id} under BY_VOLUME, {~count, id} for k_activity.h's BY_TRANSFERS — by k_select.h,
//                  which tb_cp_count and tb_cp_begin start;
//   tb_cp_emit     tb_select_rank, then the rows.
// A node: every shard scans its own log into its own table, then tb_cp_merge folds each peer's table
// into the first shard's (plain loads of the peer's HBM once its stream is idle, the same find-or-claim
// by id, local atomics), and the select and the emit run once there: a group's sums are whole before
// any order is applied.
//
// The group table: open addressing, linear probing, `mask + 1` slots of CP_SLOT_WORDS 64-bit words in
// HBM, zeroed on the stream before the scan:
//   word 0        the tag, 0 while free: 1 + {which shard's log, log position, which of the record's
//                 two account fields} of the record that claimed the slot.  One 64-bit compare-and-swap
//                 publishes it; a later probe learns the slot's id by reading that record, whose bytes
//                 never change during a call, so nothing is ever half-published and no lane waits for
//                 another;
//   word 1        unused;
//   words 2..8    `to`:   {posted, pending_in, pending_out} of two words each, then the transfer count;
//   words 9..15   `from`, likewise.
// Plain launches: no grid barrier, no spin, no wait on another workgroup; every loop is bounded by the
// workgroup's tiles, the table's slots, k or a constant.
#pragma once

#include "k_matrix.h"
#include "k_select.h"

#define CP_ROWS_MAX 8191u  // TBGPU_COUNTERPARTIES_ROWS_MAX
#define CP_ROW_BYTES 128u
#define CP_SLOT_WORDS 16u
#define CP_FLOW_WORDS 7u  // MATRIX_BIN_WORDS: a direction's sums, in the row's order
#define CP_TO 2u          // the first word of `to` in a slot; `from` follows
// The claimed bins: 60 B each with the tag, 30 KB a workgroup, two workgroups a CU.  A bin's key is
// {slot, direction}.
#ifndef CP_LDS_BINS
#define CP_LDS_BINS 512u
#endif
#define CP_SIDE_DEBITS 1u   // TBGPU_FILTER_DEBITS: records whose debit account is the subject
#define CP_SIDE_CREDITS 2u  // TBGPU_FILTER_CREDITS

// The select's key (k_select.h): CP_KEY_WORDS words, most significant first.
#define CP_KEY_WORDS 4u
#define CP_PASSES_MAX (CP_KEY_WORDS * SEL_WORD_PASSES)
#define CP_KEY_STRIDE (CP_KEY_WORDS + 1)  // a collected entry: the key's words, then its slot

// Device state of one call, u64 words: the select's (SEL_TOTAL: the occupied slots, the groups), the
// scan's flags and the key bits tb_cp_count gathers.  Every wave of tb_cp_count ORs into CP_ONES and
// CP_ZEROS, and where those atomics fall among the 128-byte lines decides its time: CP_ONES shares
// the first line with SEL_TOTAL, CP_ZEROS has the second ("The select").
enum : u32 {
    CP_ORPHAN = SEL_CALLER,        // a matching post's pending transfer was not resident
    CP_OVERFLOW = SEL_CALLER + 1,  // a hit found no slot: more groups than the table holds
    CP_ONES = SEL_CALLER + 3,      // [CP_KEY_WORDS] the OR of every key
    CP_ZEROS = SEL_WORDS,          // [CP_KEY_WORDS] the OR of every key's complement
    CP_WORDS = SEL_WORDS + 4,
};
static_assert(CP_ONES + CP_KEY_WORDS == 16 && CP_ZEROS >= 16 && CP_ZEROS + CP_KEY_WORDS <= 32, "the key bits' lines");
#define CP_STATE_BYTES SEL_STATE_BYTES(CP_WORDS, CP_PASSES_MAX)

struct CpFilter {
    u64 a_lo, a_hi;      // the subject
    u64 t_open, t_close; // the period; t_close = 0: no upper end
    u64 min_lo, min_hi;  // only counterparties at or above
    u32 sides;           // CP_SIDE_*
    u32 by_volume;
};

__host__ __device__ static inline u64 tb_cp_tag(u32 shard, u64 pos, u32 field) { return 1 + ((u64)shard << 41 | pos << 1 | field); }

// The id the slot tagged `tag` stands for: account field `field` of the record at `pos` of shard
// `shard`'s log (words 2, 3: the debit account; 4, 5: the credit account).  false: no such record.
__device__ static inline bool tb_cp_tag_id(const NodeTablesArgs& N, u64 tag, u64& lo, u64& hi) {
    const u64 t = tag - 1, pos = (t >> 1) & ((1ULL << 40) - 1);
    const u32 shard = (u32)(t >> 41), field = (u32)t & 1;
    if (tag == 0 || shard >= N.world || pos >= N.T[shard].xlog_cap) return false;
    const ulonglong2 id = ((const ulonglong2*)&N.T[shard].xlog[pos])[1 + field];
    lo = id.x, hi = id.y;
    return true;
}

// The slot of counterparty (lo, hi), found or claimed with `tag` — a record that names it — or
// CHANGE_NONE: every slot holds another id.
__device__ static inline u32 tb_cp_claim(const NodeTablesArgs& N, u64* table, u32 mask, u64 tag, u64 lo, u64 hi) {
    u32 s = (u32)tb_change_hash(lo, hi) & mask;
    for (u32 i = 0; i <= mask; i++) {
        u64* p = table + (u64)s * CP_SLOT_WORDS;
        u64 t = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t == 0) {
            t = atomicCAS((unsigned long long*)p, 0ULL, (unsigned long long)tag);
            if (t == 0) return s;
        }
        u64 xl, xh;
        if (tb_cp_tag_id(N, t, xl, xh) && xl == lo && xh == hi) return s;
        s = (s + 1) & mask;
    }
    return CHANGE_NONE;
}

// dst[0, CP_FLOW_WORDS) += one direction's sums.
__device__ static inline void tb_cp_add(u64* dst, const u128 (&v)[3], u64 count) {
    tb_atomic_add128(dst, v[0]);
    tb_atomic_add128(dst + 2, v[1]);
    tb_atomic_add128(dst + 4, v[2]);
    if (count) atomicAdd((unsigned long long*)(dst + 6), (unsigned long long)count);
}

// N.T[self] is the scanned engine, n its log's end.  table: mask + 1 slots, st: the state words — both
// zeroed on the stream before the launch.  Workgroup b scans tiles [b, b + 1) * CHANGE_TILES of
// CHANGE_THREADS positions.
__global__ __launch_bounds__(CHANGE_THREADS) void tb_cp_scan(NodeTablesArgs N, u32 self, u64 n, CpFilter F, u64* table, u32 mask,
                                                            u64* st) {
    __shared__ u64 s_bins[CP_LDS_BINS * CP_FLOW_WORDS];
    __shared__ u32 s_tags[CP_LDS_BINS];  // the {slot, direction} each bin holds
    const Tables& T = N.T[self];
    const u32 lane = threadIdx.x & 63;
    for (u32 i = threadIdx.x; i < CP_LDS_BINS * CP_FLOW_WORDS; i += CHANGE_THREADS) s_bins[i] = 0;
    for (u32 i = threadIdx.x; i < CP_LDS_BINS; i += CHANGE_THREADS) s_tags[i] = CHANGE_NONE;
    __syncthreads();
    for (u32 t = 0; t < CHANGE_TILES; t++) {
        const u64 tile0 = ((u64)blockIdx.x * CHANGE_TILES + t) * CHANGE_THREADS, pos = tile0 + threadIdx.x;
        if (tile0 >= n) break;  // the whole workgroup alike
        const u64* w = (const u64*)&T.xlog[pos < n ? pos : 0];
        const u64 ts = pos < n ? tb_log_ts(T, pos, w[15]) : 0;  // the plane: coalesced
        const bool wanted = ts > F.t_open && (F.t_close == 0 || ts <= F.t_close);
        if (__ballot(wanted) == 0) continue;  // the whole wave alike: nothing but the plane was read
        u32 key = CHANGE_NONE;  // slot * 2 + direction (0: to, 1: from)
        u128 v[3] = {0, 0, 0};  // {posted, pending_in, pending_out}
        if (wanted) {
            const ulonglong2 d = ((const ulonglong2*)w)[1], c = ((const ulonglong2*)w)[2];
            const bool is_d = (F.sides & CP_SIDE_DEBITS) && d.x == F.a_lo && d.y == F.a_hi;
            const bool is_c = (F.sides & CP_SIDE_CREDITS) && c.x == F.a_lo && c.y == F.a_hi;
            const u64 lo = w[0], hi = w[1];
            if ((is_d || is_c) && !tb_id_reserved(lo, hi) && tb_transfer_find(T, lo, hi) == (u32)pos) {
                const u128 amount = tb_u128(w[6], w[7]);
                const u32 tf = (u32)(w[14] >> 48);
                u128 p = amount;
                if (tb_effect_is_post(tf) && !tb_pending_amount(N, w[8], w[9], &p)) atomicOr((unsigned long long*)&st[CP_ORPHAN], 1ULL);
                const StatementFlows f = tb_statement_flows(tf, amount, p);
                v[0] = f.posted_in, v[1] = f.pending_in, v[2] = f.pending_out;
                // The counterparty: the record's other account, named by its field 1 (credit) for a
                // debit hit and by its field 0 for a credit hit.
                const ulonglong2 x = is_d ? c : d;
                if (x.y > F.min_hi || (x.y == F.min_hi && x.x >= F.min_lo)) {
                    const u32 slot = tb_cp_claim(N, table, mask, tb_cp_tag(self, pos, is_d ? 1 : 0), x.x, x.y);
                    if (slot == CHANGE_NONE) {
                        atomicOr((unsigned long long*)&st[CP_OVERFLOW], 1ULL);
                    } else {
                        key = slot * 2 + (is_d ? 0 : 1);
                        // A loaded record from the subject to itself, both sides wanted: `from` of
                        // its own row too, straight into the slot.
                        if (is_d && is_c) tb_cp_add(table + (u64)slot * CP_SLOT_WORDS + CP_TO + CP_FLOW_WORDS, v, 1);
                    }
                }
            }
        }
        bool adds = key != CHANGE_NONE;
        u32 count = adds ? 1 : 0;
        tb_scan_combine<3>(lane, key, adds, v, count);
        if (!adds) continue;
        const u32 at = tb_change_bin_claim(s_tags, CP_LDS_BINS, key);
        u64* bin = at != CHANGE_NONE ? s_bins + at * CP_FLOW_WORDS
                                     : table + (u64)(key >> 1) * CP_SLOT_WORDS + CP_TO + (key & 1) * CP_FLOW_WORDS;
        tb_cp_add(bin, v, count);
    }
    // The workgroup's claimed bins go to their slots: a thread per sum and per count.
    __syncthreads();
    for (u32 i = threadIdx.x; i < CP_LDS_BINS * 4; i += CHANGE_THREADS) {
        const u32 b = i / 4, part = i % 4, key = s_tags[b];
        if (key == CHANGE_NONE) continue;
        const u64* src = s_bins + b * CP_FLOW_WORDS;
        u64* dst = table + (u64)(key >> 1) * CP_SLOT_WORDS + CP_TO + (key & 1) * CP_FLOW_WORDS;
        if (part < 3) {
            tb_atomic_add128(dst + 2 * part, tb_u128(src[2 * part], src[2 * part + 1]));
        } else if (src[6]) {
            atomicAdd((unsigned long long*)(dst + 6), (unsigned long long)src[6]);
        }
    }
}

// A node's first shard folds a peer's table into its own: a thread per slot of `peer` (as many slots
// as `table`), read with plain loads once the peer's stream is idle; an occupied one finds or claims
// its id's slot here, under the peer's tag — the record lies in the peer's log — and adds its sums.
__global__ __launch_bounds__(QUERY_THREADS) void tb_cp_merge(NodeTablesArgs N, const u64* peer, u64* table, u32 mask, u64* st) {
    const u64 s = (u64)blockIdx.x * QUERY_THREADS + threadIdx.x;
    if (s > mask) return;
    const u64* src = peer + s * CP_SLOT_WORDS;
    const u64 tag = src[0];
    u64 lo, hi;
    if (!tb_cp_tag_id(N, tag, lo, hi)) return;
    const u32 slot = tb_cp_claim(N, table, mask, tag, lo, hi);
    if (slot == CHANGE_NONE) {
        atomicOr((unsigned long long*)&st[CP_OVERFLOW], 1ULL);
        return;
    }
    u64* dst = table + (u64)slot * CP_SLOT_WORDS;
#pragma unroll
    for (u32 dir = 0; dir < 2; dir++) {
        const u64* f = src + CP_TO + dir * CP_FLOW_WORDS;
        const u128 v[3] = {tb_u128(f[0], f[1]), tb_u128(f[2], f[3]), tb_u128(f[4], f[5])};
        tb_cp_add(dst + CP_TO + dir * CP_FLOW_WORDS, v, f[6]);
    }
}

// ---- the select --------------------------------------------------------------------------------------
// The key of slot `slot`, most significant word first, or false: the slot is free.  By id: {id.hi,
// id.lo, 0, 0}.  By volume: {~volume.hi, ~volume.lo, id.hi, id.lo}, volume = to.posted + from.posted
// modulo 2^128, so that ascending keys are descending volumes and equal volumes go by id.  By transfers
// (k_activity.h): {~count, id.hi, id.lo, 0}, count = to.transfers + from.transfers.  `order` is a
// CP_ORDER_*.
#define CP_ORDER_ID 0u
#define CP_ORDER_VOLUME 1u
#define CP_ORDER_TRANSFERS 2u
__host__ __device__ static inline u32 tb_cp_order_words(u32 order) { return order == CP_ORDER_VOLUME ? 4 : order == CP_ORDER_TRANSFERS ? 3 : 2; }
__device__ static inline bool tb_cp_key(const NodeTablesArgs& N, const u64* table, u64 slot, u32 mask, u32 order, u64 (&K)[CP_KEY_WORDS]) {
    if (slot > mask) return false;
    const u64* e = table + slot * CP_SLOT_WORDS;
    u64 lo, hi;
    if (!tb_cp_tag_id(N, e[0], lo, hi)) return false;
    if (order == CP_ORDER_VOLUME) {
        const u128 volume = tb_u128(e[CP_TO], e[CP_TO + 1]) + tb_u128(e[CP_TO + CP_FLOW_WORDS], e[CP_TO + CP_FLOW_WORDS + 1]);
        K[0] = ~tb_hi(volume), K[1] = ~tb_lo(volume), K[2] = hi, K[3] = lo;
    } else if (order == CP_ORDER_TRANSFERS) {
        K[0] = ~(e[CP_TO + 6] + e[CP_TO + CP_FLOW_WORDS + 6]), K[1] = hi, K[2] = lo, K[3] = 0;
    } else {
        K[0] = hi, K[1] = lo, K[2] = 0, K[3] = 0;
    }
    return true;
}

// A tile of QUERY_THREADS slots per workgroup: how many are occupied, into counts[b] and the total, and
// which bits of the keys are ever one and ever zero.
__global__ __launch_bounds__(QUERY_THREADS) void tb_cp_count(NodeTablesArgs N, const u64* table, u32 mask, u32 order, u32* counts,
                                                             u64* st) {
    __shared__ u32 s_cnt[QUERY_WAVES];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 K[CP_KEY_WORDS];
    const bool have = tb_cp_key(N, table, (u64)blockIdx.x * QUERY_THREADS + threadIdx.x, mask, order, K);
    const u64 m = __ballot(have);
    if (lane == 0) s_cnt[wave] = (u32)__popcll(m);
    if (m) {  // the whole wave alike
#pragma unroll
        for (u32 q = 0; q < CP_KEY_WORDS; q++) {
            u64 ones = have ? K[q] : 0, zeros = have ? ~K[q] : 0;
#pragma unroll
            for (u32 off = 32; off > 0; off >>= 1) {
                ones |= __shfl_xor((unsigned long long)ones, off);
                zeros |= __shfl_xor((unsigned long long)zeros, off);
            }
            if (lane == 0) {
                if (ones) atomicOr((unsigned long long*)&st[CP_ONES + q], (unsigned long long)ones);
                if (zeros) atomicOr((unsigned long long*)&st[CP_ZEROS + q], (unsigned long long)zeros);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 c = 0;
        for (u32 w = 0; w < QUERY_WAVES; w++) c += s_cnt[w];
        counts[blockIdx.x] = c;
        if (c) atomicAdd((unsigned long long*)&st[SEL_TOTAL], (unsigned long long)c);
    }
}

// One thread: the select's start.  The prefix begins as the bits every key shares, so a pass whose
// digit no two keys differ in has nothing to decide.
__global__ void tb_cp_begin(u32 k, u64* st) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    st[SEL_RANK] = k;
    for (u32 q = 0; q < CP_KEY_WORDS; q++) {
        st[SEL_PREFIX + q] = st[CP_ONES + q] & ~st[CP_ZEROS + q];
        st[SEL_VARIES + q] = st[CP_ONES + q] & st[CP_ZEROS + q];
    }
}

// The select's key source: tb_cp_key of the group table's slot.
struct CpSource {
    static constexpr u32 WORDS = CP_KEY_WORDS;
    NodeTablesArgs N;
    const u64* table;
    u32 mask, order;
    __device__ bool key(u64 slot, u64 (&K)[WORDS]) const { return tb_cp_key(N, table, slot, mask, order, K); }
};

// out[rank] = the row: the id its tag's record holds, then the slot's sums.
__global__ __launch_bounds__(QUERY_THREADS) void tb_cp_emit(NodeTablesArgs N, const u64* table, u32 mask, u32 k, const u64* st,
                                                            const u64* keys, u8* out) {
    const u32 n = (u32)min((u64)k, st[SEL_NKEYS]);
    if (blockIdx.x * SEL_EMIT_KEYS >= n) return;
    u64 mine[CP_KEY_STRIDE];
    const u32 rank = tb_select_rank<CP_KEY_WORDS>(keys, n, mine);
    const u64 slot = mine[CP_KEY_WORDS];
    if (threadIdx.x % SEL_EMIT_LANES != 0 || slot > mask || rank >= k) return;
    const u64* e = table + slot * CP_SLOT_WORDS;
    u64 lo, hi;
    if (!tb_cp_tag_id(N, e[0], lo, hi)) return;
    ulonglong2* dst = (ulonglong2*)(out + (u64)rank * CP_ROW_BYTES);
    dst[0] = make_ulonglong2(lo, hi);
#pragma unroll
    for (u32 q = 1; q < CP_ROW_BYTES / 16; q++) dst[q] = make_ulonglong2(e[2 * q], e[2 * q + 1]);
}
