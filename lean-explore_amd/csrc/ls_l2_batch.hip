// ls_l2_batch.hip — several L2 queries per corpus pass (include/leansearch_l2_batch.h): the scan
// kernel's L2 instantiations at NQ = 4 and 8 (plain scan, f32 and fp16 rows, the eight shared geometries less the four
// fp16 shapes declined at NQ = 8, never SMALL); the header's switch is ls_switch.hip's. A translation unit of its own:
// the build stays parallel and ls_l2_scan.hip's single-query kernels keep their code.
#include "ls_scan_launch.h"

int ls_launch_scan_l2_batch(const void* d_corpus, int64_t n, const ls_geom& g, const ls_scan_args& a, hipStream_t s) {
    if ((a.nq != 4 && a.nq != 8) || g.elem == 1) {
        ls_set_error("ls_launch_scan: an L2 group launch serves 4 or 8 queries over f32 or fp16 rows (nq %d, %d-byte elements)", a.nq,
                     g.elem);
        return LS_ERR_INVALID_ARG;
    }
    return ls_geom_dispatch<false, true>("ls_launch_scan", g, [&](auto L, auto V) -> int {
        if (a.nq == 8) {
            if (g.elem != 2) return ls_scan_launch<false, L(), V(), 8>(d_corpus, n, g, a, s, ls_l2_arg{});
            // (fp16 rows of 4-chunk lanes and of 16 lanes x 2 chunks at 8 queries: not built - DESIGN.md 4.11b;
            // ls_scan_l2_declines8 never plans them)
            if constexpr (V() == 4 || (L() == 16 && V() == 2)) {
                ls_set_error("ls_launch_scan: no 8-query L2 kernel for fp16 rows of %d chunks (planned as groups of 4)", g.chunks);
                return LS_ERR_INVALID_ARG;
            } else {
                return ls_scan_launch<true, L(), V(), 8>(d_corpus, n, g, a, s, ls_l2_arg{});
            }
        }
        return g.elem == 2 ? ls_scan_launch<true, L(), V(), 4>(d_corpus, n, g, a, s, ls_l2_arg{})
                           : ls_scan_launch<false, L(), V(), 4>(d_corpus, n, g, a, s, ls_l2_arg{});
    });
}
