// ls_ivf_subset.hip — the probed-list scan (ls_ivf.hip) over an IVF subset (include/leansearch_ivf_subset.h):
// ls_ivf_scan_kernel with a row list, f32 / fp16, eight geometries each. The prefix runs over the subset's soff, a
// position resolves to an index of the compacted arrays, and the row loads fetch srow[x]; dot / group_sum / keys are
// the plain kernel's, so every score is bit-identical to the flat scan's of that row. The sq8 instantiations live in
// ls_sq8_ivf_subset.hip; the subset object and the orchestration in ls_ivf.hip.
#include "ls_ivf_kernel.h"

template <bool F16, int L, int V>
static int ivf_subset_launch_lv(const ls_geom& g, const ivf_launch& a, hipStream_t s) {
    constexpr int U = scan_unroll(V);
    hipLaunchKernelGGL((ls_ivf_scan_kernel<F16, L, V, U, const u32*>), dim3(a.blocks), dim3(LS_SCAN_THREADS), 0, s,
                       (const f32x4*)a.corpus, g.chunks, a.ids, a.off, a.probe, a.nprobe, a.q, g.d,
                       a.normalize ? 1 : 0, a.S, a.cand, a.bound, a.kprime, a.srow);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

template <bool F16>
static int ivf_subset_launch_dt(const ls_geom& g, const ivf_launch& a, hipStream_t s) {
#define LS_CASE(LL, VV) \
    if (g.L == LL && g.V == VV) return ivf_subset_launch_lv<F16, LL, VV>(g, a, s);
    LS_GEOM_CASES
#undef LS_CASE
    ls_set_error("ls_ivf_search_subset: unsupported row geometry L=%d V=%d", g.L, g.V);
    return LS_ERR_INVALID_ARG;
}

int ls_ivf_launch_scan_subset(const ls_geom& g, const ivf_launch& a, hipStream_t s) {
    if (!a.srow || !a.ids || !a.off) {
        ls_set_error("ls_ivf_search_subset: a subset launch needs the subset's three arrays");
        return LS_ERR_INVALID_ARG;
    }
    if (g.elem == 1) return ls_ivf_launch_scan_subset_sq8(g, a, s);
    return g.elem == 2 ? ivf_subset_launch_dt<true>(g, a, s) : ivf_subset_launch_dt<false>(g, a, s);
}
