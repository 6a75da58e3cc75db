// ls_sq8_ivf.hip — the probed-list scan (ls_ivf.hip) over sq8 rows: ls_ivf_scan_kernel with QuerySq8, ten geometries.
// The same dot / group_sum as the sq8 scan of ls_sq8_scan.hip, so every score is bit-identical to the flat scan's.
#include "ls_ivf_kernel.h"

template <int L, int V>
static int sq8_ivf_launch_lv(const ls_geom& g, const ivf_launch& a, hipStream_t s) {
    constexpr int U = scan_unroll(V);
    hipLaunchKernelGGL((ls_ivf_scan_kernel<false, L, V, U, ls_sq8_arg>), dim3(a.blocks), dim3(LS_SCAN_THREADS), 0, s,
                       (const f32x4*)a.corpus, g.chunks, a.ids, a.off, a.probe, a.nprobe, a.q, g.d, a.normalize ? 1 : 0,
                       a.S, a.cand, a.bound, a.kprime, ls_sq8_arg{a.step});
    LS_HIP(hipGetLastError());
    return LS_OK;
}

int ls_ivf_launch_scan_sq8(const ls_geom& g, const ivf_launch& a, hipStream_t s) {
    if (!a.step) {
        ls_set_error("ls_ivf_search: an sq8 launch needs the step");
        return LS_ERR_INVALID_ARG;
    }
#define LS_CASE(LL, VV) \
    if (g.L == LL && g.V == VV) return sq8_ivf_launch_lv<LL, VV>(g, a, s);
    LS_GEOM_CASES_SQ8
#undef LS_CASE
    ls_set_error("ls_ivf_search: unsupported sq8 row geometry L=%d V=%d", g.L, g.V);
    return LS_ERR_INVALID_ARG;
}
