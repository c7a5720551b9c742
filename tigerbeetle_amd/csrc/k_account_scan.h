// k_account_scan.h — the account-set scan: what get_change_events' second pass (k_change_events.h),
// lookup_accounts_at (k_asof.h), get_account_statements (k_statement.h),
// get_account_balance_integrals (k_integral.h), get_account_statement_series (k_series.h) and, for
// its combine, get_ledger_balances (k_ledgers.h) have in common.
//
// The family.  A request names accounts; nothing was stored for it at commit.  Its accounts go into
// a hash set, and one scan of the log does the rest:
//   the set      an open-addressing table of 32-bit entries {16-bit tag, account index + 1}; a tag
//                match is confirmed against the full id (tb_change_probe).  Every workgroup copies it
//                into LDS once, as it is or narrowed to 16 bits an entry (tb_change_lds_entry);
//   the record   the timestamp alone first, from the plane: a wave with nothing above the call's lower
//                bound reads nothing else.  Then both ids against the set, and on a hit only the
//                liveness probe (the id index holds this record's id at this position) and, for a post,
//                its pending transfer's amount — the orphan flag where that is not resident
//                (tb_scan_record);
//   the combine  the lanes of the wave that hold the same key are linked into a chain (tb_scan_link)
//                and one pointer-jumping pass of six steps sums every chain into its first lane
//                (tb_scan_chain_sum), so the shuffles do not grow with the number of distinct keys;
//   the bins     every first lane adds at once: into an LDS bin its key claims at first use
//                (tb_change_bin_claim), else into the key's bin in HBM; the workgroup hands each LDS
//                bin it claimed to HBM once, at its end;
//   the answer   one engine ranks the found request positions (tb_scan_emit_rank) and writes the rows
//                on the device; a node mirrors every shard's bins back and its host adds them
//                (account_scan_host.h) and writes the same rows with the same row function.
// What a member owns: its key and bin layout, the body between the record step and the combine that
// turns a record into sums, its flush, its row function — and its __global__ kernels, with their own
// LDS sizes and __launch_bounds__.  query.h's AccountScan describes a member to the one host driver.
// Plain launches: no grid barrier, no spin, no wait on another workgroup; every loop is bounded by
// the workgroup's tiles, the set's slots, a workgroup's share of the found flags or the 64 lanes of a
// wave.
#pragma once

#include "k_balances.h"

#define CHANGE_NONE 0xFFFFFFFFu
// 512 positions a tile (two of k_query.h's) and 16 tiles a workgroup: a workgroup of eight waves
// spreads its copy of the set and its LDS bins over 8,192 records, and two such workgroups fit a CU's
// LDS at the largest set, sixteen waves a CU; 256 threads would leave eight.
#define CHANGE_THREADS 512
#define CHANGE_TILES 16
// What an emit kernel leaves in `res`: {0: found positions (rows), 1: a post's pending transfer was not resident}.
#define SCAN_RES_MATCHED 0
#define SCAN_RES_ORPHAN 1
#define SCAN_RES_WORDS 2

// The set's hash of an account id: the low bits pick the slot, the top 16 the tag.  Independent of
// tb_home's bits and of the account table's position bits by a second mix.
__host__ __device__ static inline u64 tb_change_hash(u64 lo, u64 hi) { return tb_mix64(tb_hash_id(lo, hi) ^ 0x9e3779b97f4a7c15ULL); }
__host__ __device__ static inline u32 tb_change_entry(u64 h, u32 index) { return (u32)(h >> 48) << 16 | (index + 1); }

// The index of account (lo, hi) in the set, or CHANGE_NONE.  s_set: the workgroup's copy of the
// entries; ids: the accounts' ids by index (lo, hi), read on a tag match only.
__device__ static inline u32 tb_change_probe(const u32* s_set, u32 mask, const u64* ids, u64 lo, u64 hi) {
    const u64 h = tb_change_hash(lo, hi);
    const u32 tag = (u32)(h >> 48);
    u32 s = (u32)h & mask;
    for (u32 i = 0; i <= mask; i++) {
        const u32 e = s_set[s];
        if (e == 0) return CHANGE_NONE;
        if ((e >> 16) == tag) {
            const u32 index = (e & 0xFFFFu) - 1;
            if (ids[2 * (u64)index] == lo && ids[2 * (u64)index + 1] == hi) return index;
        }
        s = (s + 1) & mask;
    }
    return CHANGE_NONE;
}

// The same over a workgroup's narrowed copy of the entries (tb_change_lds_entry): {3-bit tag, index + 1}
// in 16 bits, for sets whose indices stay below 8,191.  One occupied slot in eight passes the tag and
// pays the read of the full id.
__device__ static inline u32 tb_change_probe(const u16* s_set, u32 mask, const u64* ids, u64 lo, u64 hi) {
    const u64 h = tb_change_hash(lo, hi);
    const u32 tag = (u32)(h >> 61);
    u32 s = (u32)h & mask;
    for (u32 i = 0; i <= mask; i++) {
        const u32 e = s_set[s];
        if (e == 0) return CHANGE_NONE;
        if ((e >> 13) == tag) {
            const u32 index = (e & 0x1FFFu) - 1;
            if (ids[2 * (u64)index] == lo && ids[2 * (u64)index + 1] == hi) return index;
        }
        s = (s + 1) & mask;
    }
    return CHANGE_NONE;
}

// An entry of the set as a workgroup keeps it in LDS: as it is, or narrowed to the top three bits of
// its tag and its index + 1 (at most 8,191, never zero for an entry that is not).
template <typename ENTRY>
__device__ static inline ENTRY tb_change_lds_entry(u32 e) {
    if (sizeof(ENTRY) == 4) return (ENTRY)e;
    return (ENTRY)(e ? (e >> 29) << 13 | (e & 0x1FFFu) : 0);
}

// The LDS bin that holds `key`'s sums in this workgroup, claimed at its first add — one of the two
// slots the key hashes to — or CHANGE_NONE when other keys hold both (the add goes to HBM).
// tags: [bins] the key each LDS bin holds, CHANGE_NONE while free.
__device__ static inline u32 tb_change_bin_claim(u32* tags, u32 bins, u32 index) {
    u32 s = index % bins;
#pragma unroll
    for (u32 k = 0; k < 2; k++) {
        const u32 old = atomicCAS(&tags[s], CHANGE_NONE, index);
        if (old == CHANGE_NONE || old == index) return s;
        s = ((index * 0x9E3779B1u) >> 7) % bins;
    }
    return CHANGE_NONE;
}

// Lane `from`'s value (any lane's own when `from` is itself).
__device__ static inline u128 tb_shfl128(u128 v, u32 from) {
    const u64 lo = __shfl((unsigned long long)tb_lo(v), (int)from);
    const u64 hi = __shfl((unsigned long long)tb_hi(v), (int)from);
    return tb_u128(lo, hi);
}

// A scan's LDS before its first tile, by a workgroup of CHANGE_THREADS: the set's mask + 1 entries
// copied, `words` words of bins zeroed, `tags` tags freed.  The caller's __syncthreads() follows.
template <typename ENTRY>
__device__ static inline void tb_scan_lds_init(ENTRY* s_set, const u32* set, u32 mask, u64* s_bins, u32 words, u32* s_tags,
                                               u32 tags) {
    for (u32 i = threadIdx.x; i <= mask; i += CHANGE_THREADS) s_set[i] = tb_change_lds_entry<ENTRY>(set[i]);
    for (u32 i = threadIdx.x; i < words; i += CHANGE_THREADS) s_bins[i] = 0;
    for (u32 i = threadIdx.x; i < tags; i += CHANGE_THREADS) s_tags[i] = CHANGE_NONE;
}

// One lane's record of a tile.
struct ScanRecord {
    u64 ts;       // its timestamp; 0 past the log's end
    bool wanted;  // above the lower bound
    u32 idx[2];   // the debit and the credit account's index, CHANGE_NONE: not a member, or the record is not live
};

// The record step.  N.T[self] is the scanned engine, n its log's end.  Returns the wave's ballot of
// `wanted`: 0 — the whole wave alike — and the caller skips the tile, nothing but the timestamp plane
// was read (every tile of an ordered log's prefix).  Otherwise the ids are read where wanted, and on
// a set hit only the liveness probe runs: the id index holds this record's id at this position
// (tb_query_hit's test).  A live hit calls body(tf, amount, p) — the transfer's flags, its amount, and
// its pending transfer's amount (a post; its own otherwise, and where that is not resident, with
// *orphan raised) — there and not after the call, so that the three die where the member's sums are
// born: handed back in `r` they stayed live across the join and cost every scan 5 to 9 VGPRs.
template <typename ENTRY, typename BODY>
__device__ static inline u64 tb_scan_record(const NodeTablesArgs& N, u32 self, u64 pos, u64 n, u64 t_lower, const ENTRY* s_set,
                                            u32 mask, const u64* ids, u64* orphan, ScanRecord& r, BODY body) {
    const Tables& T = N.T[self];
    const u64* w = (const u64*)&T.xlog[pos < n ? pos : 0];
    r.ts = pos < n ? tb_log_ts(T, pos, w[15]) : 0;  // the plane: coalesced, beside chunk 7
    r.wanted = r.ts > t_lower;
    r.idx[0] = r.idx[1] = CHANGE_NONE;
    const u64 any = __ballot(r.wanted);
    if (any == 0) return 0;
    if (r.wanted) {
        const ulonglong2 d = ((const ulonglong2*)w)[1], c = ((const ulonglong2*)w)[2];
        r.idx[0] = tb_change_probe(s_set, mask, ids, d.x, d.y);
        r.idx[1] = tb_change_probe(s_set, mask, ids, c.x, c.y);
    }
    if ((r.idx[0] & r.idx[1]) != CHANGE_NONE) {
        const u64 lo = w[0], hi = w[1];
        if (tb_id_reserved(lo, hi) || tb_transfer_find(T, lo, hi) != (u32)pos) {
            r.idx[0] = r.idx[1] = CHANGE_NONE;
        } else {
            const u128 amount = tb_u128(w[6], w[7]);
            const u32 tf = (u32)(w[14] >> 48);
            u128 p = amount;
            if (tb_effect_is_post(tf) && !tb_pending_amount(N, w[8], w[9], &p)) atomicOr((unsigned long long*)orphan, 1ULL);
            body(tf, amount, p);
        }
    }
    return any;
}

// The combine's first part.  The lanes with `adds` that hold the same key `my` are linked into a
// chain: each learns the next lane of its group (nxt; itself: none), and `adds` stays true in the
// first lane of each group only.  The loop visits each distinct key once.  Returns whether any group
// has more than one lane — the whole wave alike.  A lane without `adds` joins no group, whatever
// its `my`.
__device__ static inline bool tb_scan_link(u32 lane, u32 my, bool& adds, u32& nxt) {
    const u32 key = adds ? my : CHANGE_NONE;  // (no leader's: a leader adds, and CHANGE_NONE is no key)
    bool chains = false;
    nxt = lane;
    u64 todo = __ballot(adds);
    while (todo) {  // at most 64 rounds: every round clears its leader's bit
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const u32 b = __shfl(key, leader);
        const bool mine = key == b;
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
    return chains;
}

// The combine's second part: v[0, NV) and count become the sums of the chain from this lane on — after
// step s they cover 2^(s+1) lanes — so a chain's first lane ends with its group's.
template <u32 NV>
__device__ static inline void tb_scan_chain_sum(u32 lane, u32 nxt, u128 (&v)[NV], u32& count) {
#pragma unroll
    for (u32 s = 0; s < 6; s++) {
        const bool has = nxt != lane;
        u128 o[NV];
#pragma unroll
        for (u32 c = 0; c < NV; c++) o[c] = tb_shfl128(v[c], nxt);
        const u32 oc = __shfl(count, nxt);
        const u32 nn = __shfl(nxt, nxt);
        if (has) {
#pragma unroll
            for (u32 c = 0; c < NV; c++) v[c] += o[c];
            count += oc;
            nxt = nn == nxt ? lane : nn;
        }
    }
}

// Both parts: afterwards `adds` is true in one lane of each group, whose v[0, NV) and count hold the
// group's sums.  A caller without a count passes a zero it never reads.
template <u32 NV>
__device__ static inline void tb_scan_combine(u32 lane, u32 my, bool& adds, u128 (&v)[NV], u32& count) {
    u32 nxt;
    if (tb_scan_link(lane, my, adds, nxt)) tb_scan_chain_sum<NV>(lane, nxt, v, count);
}

// An emit kernel's ranking, by a workgroup of QUERY_THREADS that answers request positions
// [b, b + 1) * QUERY_THREADS: whether this thread's position is found, its rank among the request's
// found positions, and `total`, the found positions up to the workgroup's last — in the last workgroup,
// all of them.  The base — the found positions before the workgroup's first — is a sum over
// found[0, b * QUERY_THREADS), at most 32 flags a thread, so no workgroup waits for another.
__device__ static inline bool tb_scan_emit_rank(const u32* found, u32 n, u32& rank, u32& total) {
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
    rank = (u32)__popcll(mine & ((1ULL << lane) - 1));
    total = 0;
    for (u32 w = 0; w < QUERY_WAVES; w++) {
        rank += s_part[w];
        if (w < wave) rank += s_wave[w];
        total += s_part[w] + s_wave[w];
    }
    return have;
}
