// account_scan_host.h — what a node's host does with the account-set scan's bins (k_account_scan.h):
// which bin a request position reads, and the sum of the shards' bins.  Plain C++, no device code and
// no runtime: query.h includes it, and tests/account_scan_host_check.cpp runs it under sanitizers.
#pragma once

#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

// index[i] = the smallest request position that names position i's id — the index tb_asof_gather's set
// gives the id on the device.  ids: n ids (lo, hi).
static inline std::vector<uint32_t> scan_first_positions(const uint64_t* ids, uint32_t n) {
    std::vector<uint32_t> index(n), order(n);
    std::iota(order.begin(), order.end(), 0u);
    auto same = [&](uint32_t a, uint32_t b) { return ids[2 * (uint64_t)a] == ids[2 * (uint64_t)b] && ids[2 * (uint64_t)a + 1] == ids[2 * (uint64_t)b + 1]; };
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        if (ids[2 * (uint64_t)a + 1] != ids[2 * (uint64_t)b + 1]) return ids[2 * (uint64_t)a + 1] < ids[2 * (uint64_t)b + 1];
        if (ids[2 * (uint64_t)a] != ids[2 * (uint64_t)b]) return ids[2 * (uint64_t)a] < ids[2 * (uint64_t)b];
        return a < b;
    });
    for (uint32_t j = 0; j < n; j++) index[order[j]] = j && same(order[j - 1], order[j]) ? index[order[j - 1]] : order[j];
    return index;
}

// The flow matrix's maps (k_matrix.h).  The request is two lists laid end to end, n_debit debit ids and
// then n_credit credit ids, and `first` is scan_first_positions over all of them.  row_of[index] = the
// first debit position that names the id whose index is `index`, col_of[index] = its first credit
// position (counted from the credit list's start), SCAN_PAIR_NONE where that list does not name it.
// Entries of positions that are no id's index stay SCAN_PAIR_NONE.  row_of, col_of: n_debit + n_credit
// entries each.
static constexpr uint16_t SCAN_PAIR_NONE = 0xFFFFu;
static inline void scan_pair_maps(const std::vector<uint32_t>& first, uint32_t n_debit, uint32_t n_credit, uint16_t* row_of,
                                  uint16_t* col_of) {
    const uint32_t n = n_debit + n_credit;
    std::fill(row_of, row_of + n, SCAN_PAIR_NONE);
    std::fill(col_of, col_of + n, SCAN_PAIR_NONE);
    for (uint32_t i = 0; i < n_debit; i++) {
        if (first[i] == i) row_of[i] = (uint16_t)i;  // (a debit position's first is a debit position)
    }
    for (uint32_t i = n_debit; i < n; i++) {  // ascending: the first credit position stays
        if (col_of[first[i]] == SCAN_PAIR_NONE) col_of[first[i]] = (uint16_t)(i - n_debit);
    }
}

// A bin's layout: runs of `count` sums of `words` 64-bit words each, low word first — 2: a 128-bit
// sum, 3: a 192-bit sum, 1: a plain count.
struct ScanBinRun {
    uint32_t words, count;
};
static constexpr uint32_t scan_bin_words(const ScanBinRun* runs, uint32_t n_runs) {
    uint32_t words = 0;
    for (uint32_t r = 0; r < n_runs; r++) words += runs[r].words * runs[r].count;
    return words;
}

// sum += src over `repeat` consecutive bins of the layout, as the device added them: every sum modulo
// 2^(64 * words), its carries across its own word borders and never into its neighbour.
static inline void scan_bins_add(uint64_t* sum, const uint64_t* src, const ScanBinRun* runs, uint32_t n_runs, uint32_t repeat) {
    for (uint32_t k = 0; k < repeat; k++) {
        for (uint32_t r = 0; r < n_runs; r++) {
            for (uint32_t c = 0; c < runs[r].count; c++) {
                uint64_t carry = 0;
                for (uint32_t w = 0; w < runs[r].words; w++, sum++, src++) {
                    const uint64_t a = *sum + *src, b = a + carry;
                    carry = (uint64_t)(a < *src) | (uint64_t)(b < a);  // (never both)
                    *sum = b;
                }
            }
        }
    }
}
