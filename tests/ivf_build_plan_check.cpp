// Host check of csrc/ls_ivf_build_plan.h (compiled with AddressSanitizer + UndefinedBehaviorSanitizer and run by
// tests/test_ivf_build_cpu.py): enumerate every (workgroup, wave, tile, slot, centroid batch, entry) that
// ls_ivf_assign_kernel enumerates and check that every (row, centroid) pair is scored exactly once, that no load
// leaves [0, n) x [0, nlist) (the kernel relies on no pad row), and that the workgroup count follows the scan's rule
// (at least 4 tiles per wave unless one workgroup, at most 2 workgroups per CU). The means kernel's steps likewise.
#include <cstdio>
#include <vector>

#include "ls_ivf_build_plan.h"

static const int GEOMS[8][2] = {{16, 1}, {16, 2}, {16, 3}, {16, 4}, {32, 3}, {32, 4}, {64, 3}, {64, 4}};

#define FAIL(...)                 \
    do {                          \
        std::printf(__VA_ARGS__); \
        std::printf("\n");        \
        return 1;                 \
    } while (0)

int main() {
    const long long ns[] = {0, 1, 63, 64, 2307, 20011};
    const int nlists[] = {1, 7, 37, 300, 8191};
    const int cus[] = {8, 256};
    long long cases = 0;
    for (auto& gm : GEOMS)
        for (long long n : ns)
            for (int nlist : nlists)
                for (int n_cu : cus) {
                    const int L = gm[0], V = gm[1], CB = ls_ivfb_cent_batch(V), U = scan_unroll(V);
                    const int blocks = ls_ivfb_blocks(n, L, V, n_cu);
                    const ls_ivfb_deal dl = ls_ivfb_deal_make(n, L, V, blocks);
                    if (dl.TR != U * (LS_WAVE / L) || dl.TR > LS_WAVE) FAIL("L=%d V=%d: tile of %d rows", L, V, dl.TR);
                    if (blocks < 1 || blocks > 2 * n_cu) FAIL("n=%lld n_cu=%d: %d workgroups", n, n_cu, blocks);
                    if (blocks > 1 && dl.NT < (long long)(blocks - 1) * LS_SCAN_WAVES * 4 + 1)
                        FAIL("n=%lld L=%d V=%d n_cu=%d: %d workgroups for %lld tiles (< 4 tiles per wave)", n, L, V, n_cu,
                             blocks, dl.NT);
                    // the centroid walk of one tile (the same for every tile)
                    std::vector<int> cseen((size_t)nlist, 0);
                    for (int b = 0; b < ls_ivfb_cent_batches(nlist, CB); ++b)
                        for (int j = 0; j < CB; ++j) {
                            const int c = ls_ivfb_cent(b, CB, j), cl = ls_ivfb_cent_load(c, nlist);
                            if (cl < 0 || cl >= nlist) FAIL("nlist=%d: centroid load %d", nlist, cl);
                            if (ls_ivfb_cent_valid(c, nlist)) {
                                if (c != cl) FAIL("nlist=%d: centroid %d loads %d", nlist, c, cl);
                                cseen[(size_t)c]++;
                            }
                        }
                    for (int c = 0; c < nlist; ++c)
                        if (cseen[(size_t)c] != 1) FAIL("nlist=%d: centroid %d walked %d times", nlist, c, cseen[(size_t)c]);
                    // the tile deal
                    const bool pairs = n * nlist <= (1ll << 22);  // the full (row, centroid) matrix where it is small
                    std::vector<int> rseen((size_t)n, 0);
                    std::vector<unsigned char> pseen(pairs ? (size_t)(n * nlist) : 0, 0);
                    for (long long gw = 0; gw < dl.W; ++gw)
                        for (long long step = 0;; ++step) {
                            const long long t = ls_ivfb_tile(dl.W, gw, step);
                            if (t >= dl.NT) break;
                            if (step > dl.NT) FAIL("n=%lld: wave %lld does not stop", n, gw);
                            for (int u = 0; u < U; ++u)
                                for (int grp = 0; grp < dl.R; ++grp) {
                                    const long long r = ls_ivfb_row(t, dl.TR, dl.R, u, grp);
                                    const long long rl = ls_ivfb_row_load(r, n);
                                    if (rl < 0 || rl >= n) FAIL("n=%lld: slot loads row %lld", n, rl);
                                    if (!ls_ivfb_row_valid(r, n)) continue;
                                    if (r != rl) FAIL("n=%lld: row %lld loads %lld", n, r, rl);
                                    rseen[(size_t)r]++;
                                    if (pairs)
                                        for (int b = 0; b < ls_ivfb_cent_batches(nlist, CB); ++b)
                                            for (int j = 0; j < CB; ++j) {
                                                const int c = ls_ivfb_cent(b, CB, j);
                                                if (ls_ivfb_cent_valid(c, nlist)) pseen[(size_t)(r * nlist + c)]++;
                                            }
                                }
                        }
                    for (long long r = 0; r < n; ++r)
                        if (rseen[(size_t)r] != 1) FAIL("n=%lld L=%d V=%d: row %lld visited %d times", n, L, V, r, rseen[(size_t)r]);
                    for (size_t i = 0; i < pseen.size(); ++i)
                        if (pseen[i] != 1) FAIL("n=%lld nlist=%d: pair %zu scored %d times", n, nlist, i, (int)pseen[i]);
                    // the means kernel's steps
                    std::vector<int> mseen((size_t)n, 0);
                    for (long long s = 0; s < ls_ivfb_means_steps(n); ++s)
                        for (int tid = 0; tid < LS_IVFB_MEANS_BLOCK; ++tid) {
                            const long long r = ls_ivfb_means_row(s, tid);
                            if (r < n) mseen[(size_t)r]++;
                        }
                    for (long long r = 0; r < n; ++r)
                        if (mseen[(size_t)r] != 1) FAIL("n=%lld: means row %lld visited %d times", n, r, mseen[(size_t)r]);
                    ++cases;
                }
    std::printf("OK %lld cases\n", cases);
    return 0;
}
