// account_scan_host_check.cpp — csrc/account_scan_host.h (a node's index of request positions and its
// sum of the shards' bins) against unsigned __int128 arithmetic, as a program of its own so that it
// can run under -fsanitize=address,undefined on a machine without a GPU
// (tests/test_account_scan_host.py builds and runs it).  Exit status 0: every check held.
#include "../tigerbeetle_amd/csrc/account_scan_host.h"

#include <cstdio>
#include <cstring>

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
// A word that makes carries common: all ones, zero, one, a high bit, or random.
static uint64_t edge_word() {
    switch (rng() % 6) {
        case 0: return ~0ULL;
        case 1: return 0;
        case 2: return 1;
        case 3: return 1ULL << 63;
        default: return rng();
    }
}

// a + b modulo 2^(64 * words), words <= 3, by 128-bit arithmetic a word at a time.
static void reference_add(const uint64_t* a, const uint64_t* b, uint32_t words, uint64_t* out) {
    u128 carry = 0;
    for (uint32_t w = 0; w < words; w++) {
        const u128 s = (u128)a[w] + b[w] + carry;
        out[w] = (uint64_t)s;
        carry = s >> 64;
    }
}

static void check_layout(const ScanBinRun* runs, uint32_t n_runs, uint32_t repeat, uint32_t shards) {
    const uint32_t words = scan_bin_words(runs, n_runs) * repeat;
    std::vector<uint64_t> sum(words + 2, 0xA5A5A5A5A5A5A5A5ULL), want(words, 0);  // a guard word either side
    std::fill(sum.begin() + 1, sum.end() - 1, 0);
    for (uint32_t d = 0; d < shards; d++) {
        std::vector<uint64_t> src(words);  // exactly sized: a read past it is the sanitizer's to find
        for (auto& w : src) w = edge_word();
        scan_bins_add(sum.data() + 1, src.data(), runs, n_runs, repeat);
        uint32_t at = 0;
        for (uint32_t k = 0; k < repeat; k++) {
            for (uint32_t r = 0; r < n_runs; r++) {
                for (uint32_t c = 0; c < runs[r].count; c++, at += runs[r].words) {
                    uint64_t out[3];
                    reference_add(want.data() + at, src.data() + at, runs[r].words, out);
                    memcpy(want.data() + at, out, runs[r].words * 8);
                }
            }
        }
        CHECK(at == words);
    }
    CHECK(memcmp(sum.data() + 1, want.data(), (size_t)words * 8) == 0);
    CHECK(sum.front() == 0xA5A5A5A5A5A5A5A5ULL && sum.back() == 0xA5A5A5A5A5A5A5A5ULL);
}

int main() {
    // The four layouts of csrc/query.h, and one run of each width alone.
    const ScanBinRun asof[] = {{2, 4}}, statement[] = {{2, 4}, {2, 3}, {1, 1}, {2, 3}, {1, 1}}, integral[] = {{2, 8}, {3, 4}},
                     series[] = {{2, 3}, {1, 1}, {2, 3}, {1, 1}}, w1[] = {{1, 1}}, w2[] = {{2, 1}}, w3[] = {{3, 1}};
    CHECK(scan_bin_words(asof, 1) == 8 && scan_bin_words(statement, 5) == 22 && scan_bin_words(integral, 2) == 28 &&
          scan_bin_words(series, 4) == 14);
    for (uint32_t round = 0; round < 200; round++) {
        check_layout(asof, 1, 1, 1 + round % 3);
        check_layout(statement, 5, 1, 1 + round % 3);
        check_layout(integral, 2, 1, 1 + round % 3);
        check_layout(series, 4, 1 + round % 9, 1 + round % 3);
        check_layout(w1, 1, 1, 2), check_layout(w2, 1, 1, 2), check_layout(w3, 1, 1, 2);
    }
    // Hand-made carries: across 64 bits, across 128 bits (a 192-bit sum), out of the top word
    // (dropped), and a count beside a sum that wraps — the count takes no carry.
    {
        uint64_t sum[3] = {~0ULL, ~0ULL, 7}, one[3] = {1, 0, 0};
        scan_bins_add(sum, one, w3, 1, 1);
        CHECK(sum[0] == 0 && sum[1] == 0 && sum[2] == 8);
        uint64_t top[3] = {~0ULL, ~0ULL, ~0ULL};
        scan_bins_add(top, one, w3, 1, 1);
        CHECK(top[0] == 0 && top[1] == 0 && top[2] == 0);
        uint64_t mid[3] = {1, ~0ULL, 0}, all[3] = {~0ULL, ~0ULL, 0};  // the middle word wraps by itself and by the carry
        scan_bins_add(mid, all, w3, 1, 1);
        CHECK(mid[0] == 0 && mid[1] == ~0ULL && mid[2] == 1);
        const ScanBinRun pair_count[] = {{2, 1}, {1, 1}};
        uint64_t bin[3] = {~0ULL, ~0ULL, 5}, add[3] = {1, 0, 2};
        scan_bins_add(bin, add, pair_count, 2, 1);
        CHECK(bin[0] == 0 && bin[1] == 0 && bin[2] == 7);
        uint64_t lo[2] = {~0ULL, 3}, inc[2] = {2, 0};
        scan_bins_add(lo, inc, w2, 1, 1);
        CHECK(lo[0] == 1 && lo[1] == 4);
    }
    // The index: the smallest position that names the id, ids that differ in one word only, repeats.
    {
        const uint64_t ids[] = {5, 0, 5, 1, 7, 0, 5, 0, 0, 5, 7, 0, 5, 1, 5, 0};  // (lo, hi) x 8
        const std::vector<uint32_t> index = scan_first_positions(ids, 8);
        const uint32_t want[] = {0, 1, 2, 0, 4, 2, 1, 0};
        CHECK(index.size() == 8 && memcmp(index.data(), want, sizeof want) == 0);
        CHECK(scan_first_positions(ids, 0).empty());
        CHECK(scan_first_positions(ids, 1) == std::vector<uint32_t>{0});
    }
    for (uint32_t round = 0; round < 50; round++) {
        const uint32_t n = 1 + (uint32_t)(rng() % 300);
        std::vector<uint64_t> ids(2 * (size_t)n);  // exactly sized
        for (uint32_t i = 0; i < n; i++) ids[2 * i] = rng() % 9, ids[2 * i + 1] = rng() % 3 ? 0 : ~0ULL;
        const std::vector<uint32_t> index = scan_first_positions(ids.data(), n);
        for (uint32_t i = 0; i < n; i++) {
            uint32_t first = 0;
            while (ids[2 * first] != ids[2 * i] || ids[2 * first + 1] != ids[2 * i + 1]) first++;
            CHECK(index[i] == first);
        }
    }
    printf("account_scan_host_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
