// ls_sq8_ivf_subset.hip — the probed-list scan over an IVF subset (ls_ivf_subset.hip) of sq8 rows: ls_ivf_scan_kernel
// with a row list and QuerySq8. An IVF index has at most 1024 dimensions (its centroids are an f32 index), i.e. at most
// 64 chunks of 16 codes: the six geometries below; the four that begin past d = 1024 cannot be reached and are not built.
#include "ls_ivf_kernel.h"

template <int L, int V>
static int sq8_ivf_subset_launch_lv(const ls_geom& g, const ivf_launch& a, hipStream_t s) {
    constexpr int U = scan_unroll(V);
    hipLaunchKernelGGL((ls_ivf_scan_kernel<false, L, V, U, const u32*, ls_sq8_arg>), dim3(a.blocks),
                       dim3(LS_SCAN_THREADS), 0, s, (const f32x4*)a.corpus, g.chunks, a.ids, a.off, a.probe, a.nprobe,
                       a.q, g.d, a.normalize ? 1 : 0, a.S, a.cand, a.bound, a.kprime, a.srow, ls_sq8_arg{a.step});
    LS_HIP(hipGetLastError());
    return LS_OK;
}

int ls_ivf_launch_scan_subset_sq8(const ls_geom& g, const ivf_launch& a, hipStream_t s) {
    if (!a.step || !a.srow) {
        ls_set_error("ls_ivf_search_subset: an sq8 launch needs the step and the row list");
        return LS_ERR_INVALID_ARG;
    }
#define LS_CASE(LL, VV) \
    if (g.L == LL && g.V == VV) return sq8_ivf_subset_launch_lv<LL, VV>(g, a, s);
    LS_CASE(8, 1) LS_CASE(8, 3) LS_CASE(16, 1) LS_CASE(16, 2) LS_CASE(16, 3) LS_CASE(16, 4)
#undef LS_CASE
    ls_set_error("ls_ivf_search_subset: unsupported sq8 row geometry L=%d V=%d", g.L, g.V);
    return LS_ERR_INVALID_ARG;
}
