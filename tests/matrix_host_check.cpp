// matrix_host_check.cpp — what a node's host does for get_account_flow_matrix with
// csrc/account_scan_host.h: the two maps from the request's ids (scan_pair_maps over
// scan_first_positions) and the sum of the shards' bins of one key on the matrix's layout
// {{2, 3}, {1, 1}}, against a brute-force search and unsigned __int128 arithmetic.  A program of its own
// so that it can run under -fsanitize=address,undefined on a machine without a GPU
// (tests/test_matrix_host.py builds and runs it).  Exit status 0: every check held.
#include "../tigerbeetle_amd/csrc/account_scan_host.h"

#include <cstdio>
#include <cstring>

typedef unsigned __int128 u128;
static int failures = 0;
#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) failures++, printf("line %d: %s\n", __LINE__, #x); \
    } while (0)

static uint64_t rng_state = 0x13198A2E03707344ULL;
static uint64_t rng() {  // xorshift64*: a fixed sequence
    rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1DULL;
}
static uint64_t edge_word() {
    switch (rng() % 6) {
        case 0: return ~0ULL;
        case 1: return 0;
        case 2: return 1;
        case 3: return 1ULL << 63;
        default: return rng();
    }
}

static const ScanBinRun MATRIX[] = {{2, 3}, {1, 1}};
static const uint32_t WORDS = 7;

static bool same(const std::vector<uint64_t>& ids, uint32_t a, uint32_t b) { return ids[2 * a] == ids[2 * b] && ids[2 * a + 1] == ids[2 * b + 1]; }

// The maps of `ids` (n_debit debit ids, then n_credit credit ids) against a search of each list: for
// every position, the maps at its id's index name the first position of each list that holds the id.
static void check_maps(const std::vector<uint64_t>& ids, uint32_t n_debit, uint32_t n_credit) {
    const uint32_t n = n_debit + n_credit;
    const std::vector<uint32_t> first = scan_first_positions(ids.data(), n);
    std::vector<uint16_t> row_of(n), col_of(n);  // exactly sized: a write past them is the sanitizer's to find
    scan_pair_maps(first, n_debit, n_credit, row_of.data(), col_of.data());
    std::vector<bool> is_index(n, false);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t row = SCAN_PAIR_NONE, col = SCAN_PAIR_NONE, index = 0;
        while (!same(ids, index, i)) index++;
        for (uint32_t r = n_debit; r-- > 0;) row = same(ids, r, i) ? r : row;
        for (uint32_t q = n_credit; q-- > 0;) col = same(ids, n_debit + q, i) ? q : col;
        CHECK(first[i] == index && row_of[index] == row && col_of[index] == col);
        CHECK(i < n_debit ? row != SCAN_PAIR_NONE : col != SCAN_PAIR_NONE);
        CHECK((row == SCAN_PAIR_NONE || row < n_debit) && (col == SCAN_PAIR_NONE || col < n_credit));
        is_index[index] = true;
    }
    for (uint32_t i = 0; i < n; i++) {
        if (!is_index[i]) CHECK(row_of[i] == SCAN_PAIR_NONE && col_of[i] == SCAN_PAIR_NONE);
    }
}

// `shards` sets of bins of n_keys keys, exactly sized, summed key by key as query.h's row loop does.
static void check_sums(uint32_t n_keys, uint32_t shards) {
    std::vector<std::vector<uint64_t>> bins(shards, std::vector<uint64_t>((size_t)n_keys * WORDS));
    for (auto& shard : bins) {
        for (auto& w : shard) w = edge_word();
    }
    for (uint32_t key = 0; key < n_keys; key += 1 + key / 8) {  // the first keys, then ever fewer, and the last
        for (uint32_t pass = 0; pass < 2; pass++) {
            const uint32_t k = pass ? n_keys - 1 - key : key;
            uint64_t sum[WORDS + 2] = {0xA5A5A5A5A5A5A5A5ULL, 0, 0, 0, 0, 0, 0, 0, 0xA5A5A5A5A5A5A5A5ULL};
            for (uint32_t d = 0; d < shards; d++) scan_bins_add(sum + 1, bins[d].data() + (size_t)k * WORDS, MATRIX, 2, 1);
            for (uint32_t c = 0; c < 3; c++) {
                u128 want = 0;
                for (uint32_t d = 0; d < shards; d++) want += (u128)bins[d][(size_t)k * WORDS + 2 * c] | (u128)bins[d][(size_t)k * WORDS + 2 * c + 1] << 64;
                CHECK(sum[1 + 2 * c] == (uint64_t)want && sum[2 + 2 * c] == (uint64_t)(want >> 64));
            }
            uint64_t count = 0;
            for (uint32_t d = 0; d < shards; d++) count += bins[d][(size_t)k * WORDS + 6];
            CHECK(sum[7] == count && sum[0] == 0xA5A5A5A5A5A5A5A5ULL && sum[8] == 0xA5A5A5A5A5A5A5A5ULL);
        }
    }
}

int main() {
    CHECK(scan_bin_words(MATRIX, 2) == WORDS);
    // By hand: an id in both lists, repeats in either, ids that differ in one word only.
    {
        //                             debit: 5, 7, 5, (5,1)          credit: 7, 9, 7, 5, 9
        const std::vector<uint64_t> ids = {5, 0, 7, 0, 5, 0, 5, 1, 7, 0, 9, 0, 7, 0, 5, 0, 9, 0};
        const std::vector<uint32_t> first = scan_first_positions(ids.data(), 9);
        const uint32_t want_first[] = {0, 1, 0, 3, 1, 5, 1, 0, 5};
        CHECK(memcmp(first.data(), want_first, sizeof want_first) == 0);
        uint16_t row_of[9], col_of[9];
        scan_pair_maps(first, 4, 5, row_of, col_of);
        const uint16_t N = SCAN_PAIR_NONE;
        const uint16_t want_row[] = {0, 1, N, 3, N, N, N, N, N}, want_col[] = {3, 0, N, N, N, 1, N, N, N};
        CHECK(memcmp(row_of, want_row, sizeof want_row) == 0 && memcmp(col_of, want_col, sizeof want_col) == 0);
        check_maps(ids, 4, 5);
        check_maps(ids, 9, 0), check_maps(ids, 0, 9), check_maps(ids, 1, 8), check_maps(ids, 8, 1);
    }
    // The widest shapes: 1 x 4,095 and 4,095 x 1, distinct ids, then the one id repeated on the long side.
    for (uint32_t shape = 0; shape < 4; shape++) {
        const uint32_t n_debit = shape & 1 ? 4095 : 1, n_credit = shape & 1 ? 1 : 4095;
        std::vector<uint64_t> ids(2 * 4096);  // exactly sized
        for (uint32_t i = 0; i < 4096; i++) ids[2 * i] = shape & 2 ? 1 + i % 3 : 1 + i, ids[2 * i + 1] = i % 2 ? 0 : ~0ULL;
        check_maps(ids, n_debit, n_credit);
    }
    // Random lists over few ids: both lists the same, rectangular, disjoint.
    for (uint32_t round = 0; round < 60; round++) {
        const uint32_t n_debit = 1 + (uint32_t)(rng() % 63), n_credit = round % 3 == 0 ? n_debit : 1 + (uint32_t)(rng() % 65);
        std::vector<uint64_t> ids(2 * (size_t)(n_debit + n_credit));
        for (uint32_t i = 0; i < n_debit + n_credit; i++) {
            ids[2 * i] = rng() % 40 + (round % 3 == 2 && i >= n_debit ? 100 : 0), ids[2 * i + 1] = rng() % 4 ? 0 : ~0ULL;
        }
        if (round % 3 == 0) memcpy(ids.data() + 2 * (size_t)n_debit, ids.data(), (size_t)n_debit * 16);
        check_maps(ids, n_debit, n_credit);
    }
    // The adder on the matrix's layout: every key of the largest request and of small ones, 1 to 3 shards.
    for (uint32_t shards = 1; shards <= 3; shards++) check_sums(4095, shards), check_sums(1, shards), check_sums(63 * 7, shards);
    // Hand-made carries: across 64 bits into a sum's high word, out of 128 bits (dropped, and never
    // into the next sum), and the count beside them takes none.
    {
        uint64_t bin[7] = {~0ULL, 3, ~0ULL, ~0ULL, 5, 0, 9}, add[7] = {1, 0, 1, 0, 0, 0, 2};
        scan_bins_add(bin, add, MATRIX, 2, 1);
        const uint64_t want[7] = {0, 4, 0, 0, 5, 0, 11};
        CHECK(memcmp(bin, want, sizeof want) == 0);
        uint64_t top[7] = {0, 0, 0, 0, ~0ULL, ~0ULL, ~0ULL}, one[7] = {0, 0, 0, 0, 1, 0, 1};
        scan_bins_add(top, one, MATRIX, 2, 1);
        const uint64_t wrapped[7] = {0, 0, 0, 0, 0, 0, 0};
        CHECK(memcmp(top, wrapped, sizeof wrapped) == 0);
    }
    printf("matrix_host_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
