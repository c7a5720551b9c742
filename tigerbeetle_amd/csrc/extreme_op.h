// extreme_op.h — the ordered aggregate's operator (k_extremes.h): a segment of one account's steps in
// log order as an element, the composition of two neighbouring segments, and the row written from a
// period's element.  Written once for the kernel's chains, bins and cells, tb_extreme_emit's fold, the
// host's exact path (query.h) and tests/extremes_host_check.cpp, which runs it under sanitizers on a
// machine without a GPU: plain C++ there, __host__ __device__ in a device build.  The next ordered
// aggregate — the first time below a threshold, the longest run below zero — is another element type
// with its own compose; the chain pass, the bins and the fold take any.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define TB_OP_HD __host__ __device__
#else
// Outside a device build k_integral.h is not there: the 192-bit value and its add as it has them.
#define TB_OP_HD
struct U192 {
    uint64_t w0, w1, w2;
};
static inline U192 tb_add192(U192 a, U192 b) {
    const unsigned __int128 lo = (unsigned __int128)a.w0 + b.w0;
    const unsigned __int128 mid = (unsigned __int128)a.w1 + b.w1 + (uint64_t)(lo >> 64);
    return {(uint64_t)lo, (uint64_t)mid, a.w2 + b.w2 + (uint64_t)(mid >> 64)};
}
static inline U192 tb_neg192(U192 a) { return tb_add192({~a.w0, ~a.w1, ~a.w2}, {1, 0, 0}); }
#endif

// Signed 192-bit values are U192s read as two's complement.
TB_OP_HD static inline bool tb_less192(U192 a, U192 b) {
    if (a.w2 != b.w2) return (int64_t)a.w2 < (int64_t)b.w2;
    if (a.w1 != b.w1) return a.w1 < b.w1;
    return a.w0 < b.w0;
}
TB_OP_HD static inline U192 tb_sub192(U192 a, U192 b) { return tb_add192(a, tb_neg192(b)); }

// A segment of one account's steps in log order.  count == 0: the empty segment, the identity.
struct ExtremeElem {
    U192 sum;             // the segment's net step
    U192 lo, hi;          // the minimum and maximum over its non-empty prefixes, relative to its start
    uint64_t t_lo, t_hi;       // where each is first reached
    uint64_t count;            // its records
    uint64_t first_ts, last_ts;
};
TB_OP_HD static inline ExtremeElem tb_extreme_empty() { return ExtremeElem{{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, 0, 0, 0, 0, 0}; }
TB_OP_HD static inline ExtremeElem tb_extreme_leaf(U192 step, uint64_t ts) { return ExtremeElem{step, step, step, ts, ts, 1, ts, ts}; }

// A then B.  Ties go to A: `first reached`.  *unordered is raised when B does not start after A ends.
TB_OP_HD static inline ExtremeElem tb_extreme_compose(const ExtremeElem& A, const ExtremeElem& B, bool* unordered) {
    if (B.count == 0) return A;
    if (A.count == 0) return B;
    if (B.first_ts <= A.last_ts) *unordered = true;
    ExtremeElem R = A;
    R.sum = tb_add192(A.sum, B.sum);
    const U192 lo = tb_add192(A.sum, B.lo), hi = tb_add192(A.sum, B.hi);
    if (tb_less192(lo, A.lo)) R.lo = lo, R.t_lo = B.t_lo;
    if (tb_less192(A.hi, hi)) R.hi = hi, R.t_hi = B.t_hi;
    R.count = A.count + B.count;
    R.last_ts = B.last_ts;
    return R;
}

TB_OP_HD static inline void tb_extreme_store(uint64_t* w, const ExtremeElem& e) {
    w[0] = e.sum.w0, w[1] = e.sum.w1, w[2] = e.sum.w2, w[3] = e.lo.w0, w[4] = e.lo.w1, w[5] = e.lo.w2;
    w[6] = e.hi.w0, w[7] = e.hi.w1, w[8] = e.hi.w2, w[9] = e.t_lo, w[10] = e.t_hi, w[11] = e.count;
    w[12] = e.first_ts, w[13] = e.last_ts;
}
TB_OP_HD static inline ExtremeElem tb_extreme_load(const uint64_t* w) {
    return ExtremeElem{{w[0], w[1], w[2]}, {w[3], w[4], w[5]}, {w[6], w[7], w[8]}, w[9], w[10], w[11], w[12], w[13]};
}

// One row from an account's id, the measure at t_open and the period's element: 24 words {id,
// opening[3], closing[3], low[3], high[3], t_low, t_high, records, t_open, t_end, measure, 0 x 4}.
// Device and host alike: the exact path writes its rows with it.
TB_OP_HD static inline void tb_extreme_row(uint64_t id_lo, uint64_t id_hi, U192 opening, const ExtremeElem& e, uint64_t t_open, uint64_t t_end,
                                                      uint64_t measure, uint64_t* row) {
    const ExtremeElem start{{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, t_open, t_open, 1, 0, 0};  // v_0: the opening itself, first of all
    bool ignored = false;
    ExtremeElem all = start;
    if (e.count) {
        ExtremeElem rest = e;
        if (rest.first_ts == 0) rest.first_ts = 1;  // (no record has timestamp 0; `start` ends at 0)
        all = tb_extreme_compose(start, rest, &ignored);
    }
    const U192 closing = tb_add192(opening, e.sum), low = tb_add192(opening, all.lo), high = tb_add192(opening, all.hi);
    row[0] = id_lo, row[1] = id_hi;
    row[2] = opening.w0, row[3] = opening.w1, row[4] = opening.w2;
    row[5] = closing.w0, row[6] = closing.w1, row[7] = closing.w2;
    row[8] = low.w0, row[9] = low.w1, row[10] = low.w2;
    row[11] = high.w0, row[12] = high.w1, row[13] = high.w2;
    row[14] = all.t_lo, row[15] = all.t_hi, row[16] = e.count, row[17] = t_open, row[18] = t_end, row[19] = measure;
    row[20] = row[21] = row[22] = row[23] = 0;
}

