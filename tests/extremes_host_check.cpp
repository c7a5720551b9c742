// extremes_host_check.cpp — get_account_balance_extremes' operator (csrc/extreme_op.h) as the kernel's
// chains, bins and cells, the emit's fold and the host's exact path compose it: its identity, its
// associativity, its tie rule, the signed 192-bit compare and the carries of its sums across the 64-
// and the 128-bit border, against a walk of the same steps in __int128 limbs.  Random sequences are
// folded whole and split at every cut point and as balanced trees, and the kernel's six-step chain pass
// is replayed on 64 lanes kept in arrays: it must keep lane order.  A
// program of its own so that it can run under -fsanitize=address,undefined on a machine without a GPU
// (tests/test_extremes_host.py builds and runs it).  Exit status 0: every check held.
#include "../tigerbeetle_amd/csrc/extreme_op.h"

#include <cstdio>
#include <cstring>
#include <vector>

typedef unsigned __int128 u128;
static int failures = 0;
#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) failures++, printf("line %d: %s\n", __LINE__, #x); \
    } while (0)

static uint64_t rng_state = 0x243F6A8885A308D3ULL;
static uint64_t rng() {  // xorshift64*: a fixed sequence
    rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1DULL;
}

// A signed 192-bit reference value in limbs the operator does not use: a signed top of 64 bits over an
// unsigned 128-bit bottom.
struct Ref {
    int64_t top;
    u128 low;
};
static Ref ref_of(U192 v) { return {(int64_t)v.w2, (u128)v.w1 << 64 | v.w0}; }
static Ref ref_add(Ref a, Ref b) {
    const u128 low = a.low + b.low;
    return {(int64_t)((uint64_t)a.top + (uint64_t)b.top + (uint64_t)(low < a.low)), low};
}
static bool ref_less(Ref a, Ref b) { return a.top != b.top ? a.top < b.top : a.low < b.low; }
static bool ref_same(Ref a, U192 v) { return a.top == (int64_t)v.w2 && a.low == ((u128)v.w1 << 64 | v.w0); }

static bool same(const ExtremeElem& a, const ExtremeElem& b) {
    uint64_t x[14], y[14];
    tb_extreme_store(x, a), tb_extreme_store(y, b);
    return memcmp(x, y, sizeof x) == 0;
}

// A step below 2^130 in magnitude, with words on the borders: +-(2^64 - 1), +-2^64, +-2^127, +-(2^128 - 1), small ones.
static U192 edge_step() {
    U192 v = {0, 0, 0};
    switch (rng() % 8) {
        case 0: v = {~0ULL, 0, 0}; break;
        case 1: v = {0, 1, 0}; break;
        case 2: v = {0, 1ULL << 63, 0}; break;
        case 3: v = {~0ULL, ~0ULL, 0}; break;
        case 4: v = {~0ULL, ~0ULL, 1}; break;
        case 5: v = {rng() % 7, 0, 0}; break;  // small, often equal: ties
        default: v = {rng(), rng(), rng() % 2}; break;
    }
    return rng() % 2 ? tb_neg192(v) : v;
}

// The definition: walk the steps, keep the least and the greatest prefix sum and the first timestamp of each.
static ExtremeElem walk(const std::vector<U192>& steps, uint64_t ts0) {
    ExtremeElem e = tb_extreme_empty();
    Ref sum = {0, 0}, lo = {0, 0}, hi = {0, 0};
    for (size_t i = 0; i < steps.size(); i++) {
        sum = ref_add(sum, ref_of(steps[i]));
        const uint64_t ts = ts0 + 3 * i;
        if (i == 0 || ref_less(sum, lo)) lo = sum, e.t_lo = ts;
        if (i == 0 || ref_less(hi, sum)) hi = sum, e.t_hi = ts;
        if (i == 0) e.first_ts = ts;
        e.last_ts = ts, e.count++;
    }
    e.sum = {(uint64_t)sum.low, (uint64_t)(sum.low >> 64), (uint64_t)sum.top};
    e.lo = {(uint64_t)lo.low, (uint64_t)(lo.low >> 64), (uint64_t)lo.top};
    e.hi = {(uint64_t)hi.low, (uint64_t)(hi.low >> 64), (uint64_t)hi.top};
    return e;
}

static ExtremeElem fold(const std::vector<U192>& steps, size_t from, size_t to, uint64_t ts0, bool* unordered) {
    ExtremeElem e = tb_extreme_empty();
    for (size_t i = from; i < to; i++) e = tb_extreme_compose(e, tb_extreme_leaf(steps[i], ts0 + 3 * i), unordered);
    return e;
}

// The composition as a balanced tree, the shape of a chain pass: halves of halves.
static ExtremeElem tree(const std::vector<U192>& steps, size_t from, size_t to, uint64_t ts0, bool* unordered) {
    if (to - from == 0) return tb_extreme_empty();
    if (to - from == 1) return tb_extreme_leaf(steps[from], ts0 + 3 * from);
    const size_t mid = from + (to - from + 1) / 2;
    return tb_extreme_compose(tree(steps, from, mid, ts0, unordered), tree(steps, mid, to, ts0, unordered), unordered);
}

static void check_compare_and_carries() {
    const U192 zero = {0, 0, 0}, one = {1, 0, 0}, minus_one = {~0ULL, ~0ULL, ~0ULL};
    const U192 low_border = {~0ULL, 0, 0}, mid_border = {~0ULL, ~0ULL, 0}, least = {0, 0, 1ULL << 63}, most = {~0ULL, ~0ULL, ~0ULL >> 1};
    CHECK(tb_less192(minus_one, zero) && !tb_less192(zero, minus_one) && !tb_less192(zero, zero));
    CHECK(tb_less192(least, minus_one) && tb_less192(minus_one, one) && tb_less192(one, most) && tb_less192(least, most));
    CHECK(tb_less192(low_border, {0, 1, 0}) && tb_less192(mid_border, {0, 0, 1}) && tb_less192({0, 0, 1}, most));
    CHECK(tb_less192(tb_neg192({0, 0, 1}), tb_neg192(mid_border)));  // -2^128 < -(2^128 - 1)
    // Carries across both borders, and back.
    U192 v = tb_add192(low_border, one);
    CHECK(v.w0 == 0 && v.w1 == 1 && v.w2 == 0);
    v = tb_add192(mid_border, one);
    CHECK(v.w0 == 0 && v.w1 == 0 && v.w2 == 1);
    v = tb_sub192({0, 0, 1}, one);
    CHECK(v.w0 == ~0ULL && v.w1 == ~0ULL && v.w2 == 0);
    v = tb_sub192(zero, one);
    CHECK(v.w0 == ~0ULL && v.w1 == ~0ULL && v.w2 == ~0ULL);
    for (int i = 0; i < 20000; i++) {
        const U192 a = edge_step(), b = edge_step();
        CHECK(ref_same(ref_add(ref_of(a), ref_of(b)), tb_add192(a, b)));
        CHECK(tb_less192(a, b) == ref_less(ref_of(a), ref_of(b)));
        const U192 d = tb_sub192(a, b);
        CHECK(ref_same(ref_add(ref_of(d), ref_of(b)), a));
    }
}

static void check_identity_and_ties() {
    bool unordered = false;
    const ExtremeElem empty = tb_extreme_empty();
    const ExtremeElem a = tb_extreme_leaf({5, 0, 0}, 10), b = tb_extreme_leaf(tb_neg192({5, 0, 0}), 20), c = tb_extreme_leaf({5, 0, 0}, 30);
    CHECK(same(tb_extreme_compose(empty, a, &unordered), a) && same(tb_extreme_compose(a, empty, &unordered), a));
    CHECK(same(tb_extreme_compose(empty, empty, &unordered), empty) && !unordered);
    // +5, -5, +5: the high of 5 is first reached at 10, and the low of 0... the least prefix is 0 at 20.
    const ExtremeElem abc = tb_extreme_compose(tb_extreme_compose(a, b, &unordered), c, &unordered);
    CHECK(abc.t_hi == 10 && abc.hi.w0 == 5 && abc.t_lo == 20 && abc.lo.w0 == 0 && abc.lo.w2 == 0 && abc.count == 3 && !unordered);
    CHECK(same(abc, tb_extreme_compose(a, tb_extreme_compose(b, c, &unordered), &unordered)));
    // Zero steps: every prefix ties, the first timestamp stays on both sides.
    const ExtremeElem z = tb_extreme_compose(tb_extreme_leaf({0, 0, 0}, 7), tb_extreme_leaf({0, 0, 0}, 8), &unordered);
    CHECK(z.t_lo == 7 && z.t_hi == 7 && !unordered);
    // Order is checked where it is used.
    bool bad = false;
    tb_extreme_compose(c, a, &bad);
    CHECK(bad);
    bad = false;
    tb_extreme_compose(a, a, &bad);  // the same timestamp twice is no order either
    CHECK(bad);
    // The row: the opening is v_0 at t_open and wins every tie.
    uint64_t row[24];
    tb_extreme_row(3, 4, {100, 0, 0}, abc, 9, 40, 0x01FF00FF, row);
    CHECK(row[0] == 3 && row[1] == 4 && row[2] == 100 && row[5] == 105 && row[8] == 100 && row[14] == 9 && row[11] == 105 && row[15] == 10);
    CHECK(row[16] == 3 && row[17] == 9 && row[18] == 40 && row[19] == 0x01FF00FF && row[20] == 0 && row[23] == 0);
    tb_extreme_row(3, 4, tb_neg192({100, 0, 0}), empty, 9, 40, 1, row);
    CHECK(row[2] == (uint64_t)-100 && row[4] == ~0ULL && row[7] == ~0ULL && row[8] == row[2] && row[11] == row[2] && row[14] == 9 && row[15] == 9 && row[16] == 0);
}

static void check_splits() {
    for (int round = 0; round < 300; round++) {
        const size_t n = 1 + rng() % 70;
        std::vector<U192> steps(n);  // exactly sized: a read past it is the sanitizer's to find
        for (U192& s : steps) s = edge_step();
        const uint64_t ts0 = 1 + rng() % 1000;
        bool unordered = false;
        const ExtremeElem whole = fold(steps, 0, n, ts0, &unordered);
        CHECK(same(whole, walk(steps, ts0)));
        CHECK(same(whole, tree(steps, 0, n, ts0, &unordered)));
        for (size_t cut = 0; cut <= n; cut++) {
            const ExtremeElem left = fold(steps, 0, cut, ts0, &unordered), right = tree(steps, cut, n, ts0, &unordered);
            CHECK(same(tb_extreme_compose(left, right, &unordered), whole));
            // Three parts, grouped both ways.
            const size_t cut2 = cut + (n - cut) / 2;
            const ExtremeElem mid = fold(steps, cut, cut2, ts0, &unordered), tail = fold(steps, cut2, n, ts0, &unordered);
            const ExtremeElem l = tb_extreme_compose(tb_extreme_compose(left, mid, &unordered), tail, &unordered);
            const ExtremeElem r = tb_extreme_compose(left, tb_extreme_compose(mid, tail, &unordered), &unordered);
            CHECK(same(l, whole) && same(r, whole));
            // Through memory, as a bin or a cell holds it.
            uint64_t words[14];
            tb_extreme_store(words, left);
            CHECK(same(tb_extreme_load(words), left));
        }
        CHECK(!unordered);
    }
}

// The kernel's chain pass (k_extremes.h tb_extreme_chain) on 64 lanes kept in arrays: every lane reads
// its successor's element and successor at once, then composes its own element in front.  Lanes of
// random groups are linked as tb_scan_link links them (each to the next lane of its group, the last to
// itself); after six steps a group's first lane must hold the group's fold in lane order — the lower
// lane always the left operand.
static void check_chain_pass() {
    for (int round = 0; round < 400; round++) {
        const uint32_t groups = 1 + rng() % (round % 4 == 0 ? 1 : 9);
        uint32_t key[64], nxt[64];
        ExtremeElem e[64];
        std::vector<U192> steps(64);
        for (uint32_t l = 0; l < 64; l++) {
            key[l] = rng() % 5 == 0 ? ~0u : (uint32_t)(rng() % groups);  // some lanes hold nothing
            steps[l] = edge_step();
            e[l] = key[l] == ~0u ? tb_extreme_empty() : tb_extreme_leaf(steps[l], 100 + 3 * l);
        }
        for (uint32_t l = 0; l < 64; l++) {
            nxt[l] = l;
            for (uint32_t m = l + 1; m < 64 && key[l] != ~0u; m++) {
                if (key[m] == key[l]) {
                    nxt[l] = m;
                    break;
                }
            }
        }
        bool unordered = false;
        for (int s = 0; s < 6; s++) {
            ExtremeElem o[64];
            uint32_t nn[64];
            for (uint32_t l = 0; l < 64; l++) o[l] = e[nxt[l]], nn[l] = nxt[nxt[l]];
            for (uint32_t l = 0; l < 64; l++) {
                if (nxt[l] == l) continue;
                e[l] = tb_extreme_compose(e[l], o[l], &unordered);
                nxt[l] = nn[l] == nxt[l] ? l : nn[l];
            }
        }
        CHECK(!unordered);
        for (uint32_t g = 0; g < groups; g++) {
            ExtremeElem want = tb_extreme_empty();
            uint32_t first = 64;
            for (uint32_t l = 0; l < 64; l++) {
                if (key[l] != g) continue;
                if (first == 64) first = l;
                want = tb_extreme_compose(want, tb_extreme_leaf(steps[l], 100 + 3 * l), &unordered);
            }
            if (first != 64) CHECK(same(e[first], want) && nxt[first] == first);
        }
    }
}

int main() {
    check_chain_pass();
    check_compare_and_carries();
    check_identity_and_ties();
    check_splits();
    printf("extremes_host_check: %d failures\n", failures);
    return failures != 0;
}
