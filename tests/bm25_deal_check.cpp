// Host check of csrc/ls_bm25_deal.h (compiled and run by tests/test_bm25_subset_cpu.py): enumerate every
// (workgroup, thread, step, u) the BM25 score kernel enumerates and check that every position of [0, m) is
// visited exactly once by a valid lane and that no invalid lane reports a position < m.
#include <cstdio>
#include <vector>

#include "ls_bm25_deal.h"

static const int U = 4;  // LS_BM25_U: the kernel evaluates steps s0 .. s0 + U - 1 of every batch

int main() {
    std::vector<long long> ms;
    for (long long m = 0; m < 70; ++m) ms.push_back(m);
    for (long long m : {255, 256, 257, 1023, 2047, 2049, 2305, 4097, 20000, 65537}) ms.push_back(m);
    const long long Bs[] = {1, 2, 3, 5, 7, 8, 16, 24, 72, 256};
    long long cases = 0;
    for (long long m : ms)
        for (long long B : Bs) {
            std::vector<int> seen((size_t)m, 0);
            for (long long block = 0; block < B; ++block) {
                const ls_bm25_deal d = ls_bm25_deal_make(m, B, block);
                for (long long s0 = 0; s0 < d.steps; s0 += U)
                    for (int u = 0; u < U; ++u)
                        for (int t = 0; t < 256; ++t) {
                            const long long row = ls_bm25_deal_row(d, s0 + u, t);
                            if (row < 0) {
                                std::printf("m=%lld B=%lld: negative position %lld\n", m, B, row);
                                return 1;
                            }
                            if (ls_bm25_deal_valid(d, s0 + u, row)) {
                                if (row >= m) {
                                    std::printf("m=%lld B=%lld: valid lane at position %lld\n", m, B, row);
                                    return 1;
                                }
                                seen[(size_t)row]++;
                            } else if (row < m) {
                                std::printf("m=%lld B=%lld: invalid lane reports position %lld\n", m, B, row);
                                return 1;
                            }
                        }
            }
            for (long long r = 0; r < m; ++r)
                if (seen[(size_t)r] != 1) {
                    std::printf("m=%lld B=%lld: position %lld visited %d times\n", m, B, r, seen[(size_t)r]);
                    return 1;
                }
            ++cases;
        }
    std::printf("OK %lld cases\n", cases);
    return 0;
}
