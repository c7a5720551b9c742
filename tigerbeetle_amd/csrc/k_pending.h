// k_pending.h — get_pending_transfers (include/tbgpu.h tbgpu_get_pending_transfers): the two-phase
// transfers of a window, each with its state — open, expired at a clock the caller names, posted or
// voided — and, for a posted or voided one, the record that resolved it.
//
// Nothing is stored for it at commit.  The log holds every pending record with its timeout, and
// T.xposted[pos] holds what became of the pending transfer at log position pos, so
//   the selection  is k_query.h's scan under a third predicate, QueryPendingFilter (defined there,
//                  beside the other two): count -> scan -> scatter on an ordered log, the keyed rounds
//                  on one out of timestamp order.  It reads chunks 6 and 7 of every record (32 B), the
//                  account ids of a pending record in the window only when an account is named, and
//                  the posted byte only for a pending record that passed so far.  The kernel that
//                  writes a kept row writes its state beside it: tb_query_scatter, or, behind the
//                  keyed rounds, tb_pending_gather below;
//   the join       tb_pending_resolutions, only when a kept row is posted or voided: the host builds
//                  the set of those rows' ids (k_change_events.h's open-addressing table: 32-bit
//                  entries {16-bit tag, index + 1}), a workgroup copies it into LDS once, and every
//                  record with the post or the void flag that is newer than the oldest such row probes
//                  it with its pending_id.  A hit that is live (k_query.h's probe) stores its 128 bytes
//                  into slot `index`.  Commits resolve a pending transfer at most once, so at most one
//                  live record hits a slot: plain vector stores, no atomics.
// The set: at most 4,095 ids take 8,192 slots, 32 KB of LDS as 32-bit entries.  The ids themselves
// stay in HBM and are read on a tag match only, so nothing needs narrowing: four workgroups fit a
// compute unit's 160 KB at the largest set.
// Plain launches: no grid barrier, no spin, no wait on another workgroup; every loop is bounded by
// the workgroup's tiles or the set's slots.
#pragma once

#include "k_change_events.h"

#define PENDING_ROWS_MAX 4095u  // TBGPU_PENDING_ROWS_MAX
// 256 positions a tile (k_query.h's) and 16 tiles a workgroup: its copy of the set, 1 KB to 32 KB,
// is spread over 4,096 records.
#define PENDING_THREADS 256
#define PENDING_TILES 16

// Behind the keyed rounds: the records at m chosen log positions, in that order, each with its state.
__global__ __launch_bounds__(QUERY_THREADS) void tb_pending_gather(Tables T, QueryPendingFilter flt, const u64* positions, u32 m,
                                                                   u64 n, u8* out) {
    const u32 i = blockIdx.x * QUERY_THREADS + threadIdx.x;
    if (i >= m) return;
    const u64 pos = positions[i];
    if (pos >= n) return;
    const ulonglong2* c = (const ulonglong2*)&T.xlog[pos];
    const ulonglong2 b = c[6], d = c[7];
    const QueryPendingFields f{tb_log_ts(T, pos, d.y), (u32)(b.y >> 32), (u32)(d.x >> 48)};
    *(Transfer*)(out + (u64)i * 128) = tb_log_load(T, pos);
    flt.states[i] = (u8)flt.state(f, T.xposted, pos);
}

// set: mask + 1 entries over ids[0, count) (lo, hi), count <= PENDING_ROWS_MAX; slots: [count] 128-B
// records, zeroed on the stream before the launch.  Workgroup b scans tiles [b, b + 1) * PENDING_TILES
// of PENDING_THREADS positions of the log's n records.  Dynamic LDS: the set's mask + 1 entries.
// A record at or below ts_floor — the oldest kept resolved row's timestamp — resolves none of them.
__global__ __launch_bounds__(PENDING_THREADS) void tb_pending_resolutions(Tables T, u64 n, u64 ts_floor, const u32* set, u32 mask,
                                                                         const u64* ids, u8* slots) {
    extern __shared__ __attribute__((aligned(16))) u8 s_lds[];
    u32* s_set = (u32*)s_lds;
    for (u32 i = threadIdx.x; i <= mask; i += PENDING_THREADS) s_set[i] = set[i];
    __syncthreads();
    for (u32 t = 0; t < PENDING_TILES; t++) {
        const u64 tile0 = ((u64)blockIdx.x * PENDING_TILES + t) * PENDING_THREADS, pos = tile0 + threadIdx.x;
        if (tile0 >= n) break;  // the whole workgroup alike
        if (pos >= n) continue;
        // Chunk 7 first: the flags and the timestamp decide whether chunk 4, the pending_id, is read.
        const ulonglong2* c = (const ulonglong2*)&T.xlog[pos];
        const ulonglong2 d = c[7];
        const u32 tf = (u32)(d.x >> 48);
        // A post / void's record is always written whole (its field holds its timestamp): a zero
        // field is a create's or a dead position's, which the flags drop.
        if (!(tf & (TF_POST | TF_VOID)) || (tf & TF_PENDING) || tb_log_ts(T, pos, d.y) <= ts_floor) continue;
        const ulonglong2 p = c[4];
        const u32 index = tb_change_probe(s_set, mask, ids, p.x, p.y);
        if (index == CHANGE_NONE) continue;
        // Live: the id index holds this record's id at this position (tb_query_hit's test).
        const ulonglong2 id = c[0];
        if (tb_id_reserved(id.x, id.y) || tb_transfer_find(T, id.x, id.y) != (u32)pos) continue;
        *(Transfer*)(slots + (u64)index * 128) = tb_log_load(T, pos);
    }
}
