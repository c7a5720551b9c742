// index_home.cpp — the transfer index's home function and probe step (csrc/tb_device.h tb_xi_home,
// tb_xi_next), on the host, for tests (tests/test_index_home.py, tests/test_gpu_index_locality.py).
// Compiled host-only; it never touches a GPU.
//
//   index_home group                      the group size G
//   index_home homes <cap>                ids "hi lo" (hex) on stdin -> "home" per line (decimal)
//   index_home cycle <cap> <start>        tb_xi_steps(cap - 1), then every entry from <start> on,
//                                         one tb_xi_next at a time, until steps + 1 entries are out
//   index_home family <name> <n> <cap>    ids k = 0..n-1 of a family -> the G slot-class counts,
//                                         then the number of segments no id's home fell into
// families: sequential (id = k + 1), reversed (maxInt - (k + 1)), shl3 (k << 3), shl16 (k << 16),
// hi (lo constant, hi = k), scramble (lo = a 64-bit bijective mix of k).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tigerbeetle_amd/csrc/tb_device.h"

static void family_id(const char* name, u64 k, u64* lo, u64* hi) {
    *hi = 0;
    if (!strcmp(name, "sequential")) {
        *lo = k + 1;
    } else if (!strcmp(name, "reversed")) {
        *lo = ~0ULL - (k + 1);
        *hi = ~0ULL;
    } else if (!strcmp(name, "shl3")) {
        *lo = k << 3;
    } else if (!strcmp(name, "shl16")) {
        *lo = k << 16;
    } else if (!strcmp(name, "hi")) {
        *lo = 0x1234567;
        *hi = k;
    } else if (!strcmp(name, "scramble")) {
        *lo = tb_mix64(k + 0x9e3779b97f4a7c15ULL);
    } else {
        fprintf(stderr, "unknown family %s\n", name);
        exit(2);
    }
}

int main(int argc, char** argv) {
    if (argc >= 2 && !strcmp(argv[1], "group")) {
        printf("%llu\n", (unsigned long long)XI_GROUP);
        return 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "homes")) {
        const u64 mask = strtoull(argv[2], nullptr, 0) - 1;
        u64 hi, lo;
        while (scanf("%" SCNx64 " %" SCNx64, &hi, &lo) == 2) printf("%" PRIu64 "\n", tb_xi_home(lo, hi, mask));
        return 0;
    }
    if (argc >= 4 && !strcmp(argv[1], "cycle")) {
        const u64 mask = strtoull(argv[2], nullptr, 0) - 1;
        u64 p = strtoull(argv[3], nullptr, 0);
        const u64 steps = tb_xi_steps(mask);
        printf("%" PRIu64 "\n", steps);
        for (u64 n = 0; n <= steps; n++) {
            printf("%" PRIu64 "\n", p);
            p = tb_xi_next(p, mask);
        }
        return 0;
    }
    if (argc >= 5 && !strcmp(argv[1], "family")) {
        const u64 n = strtoull(argv[3], nullptr, 0), cap = strtoull(argv[4], nullptr, 0), mask = cap - 1;
        std::vector<u64> classes(XI_GROUP, 0);
        std::vector<u8> hit(cap >> XI_GROUP_LOG2, 0);
        for (u64 k = 0; k < n; k++) {
            u64 lo, hi;
            family_id(argv[2], k, &lo, &hi);
            const u64 home = tb_xi_home(lo, hi, mask);
            classes[home & (XI_GROUP - 1)]++;
            hit[home >> XI_GROUP_LOG2] = 1;
        }
        for (u64 c : classes) printf("%" PRIu64 "\n", c);
        u64 empty = 0;
        for (u8 h : hit) empty += !h;
        printf("%" PRIu64 "\n", empty);
        return 0;
    }
    fprintf(stderr, "usage: index_home group | homes <cap> | cycle <cap> <start> | family <name> <n> <cap>\n");
    return 2;
}
