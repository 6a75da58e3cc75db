// ls_ivf_subset.hip — the probed-list scan (ls_ivf.hip) over an IVF subset (include/leansearch_ivf_subset.h):
// ls_ivf_scan_kernel with a row list, f32 / fp16, eight geometries each. The prefix runs over the subset's soff, a
// position resolves to an index of the compacted arrays, and the row loads fetch srow[x]; dot / group_sum / keys are
// the plain kernel's, so every score is bit-identical to the flat scan's of that row. The sq8 instantiations live in
// ls_sq8_ivf_subset.hip; the subset object and the orchestration in ls_ivf.hip.
#include "ls_scan_launch.h"

template <bool F16>
static int ivf_subset_launch_dt(const ls_geom& g, const ivf_launch& a, hipStream_t s) {
    return ls_geom_dispatch<false, true>("ls_ivf_search_subset", g, [&](auto L, auto V) -> int {
        return ls_ivf_scan_launch<F16, L(), V()>(g, a, s, a.srow);
    });
}

int ls_ivf_launch_scan_subset(const ls_geom& g, const ivf_launch& a, hipStream_t s) {
    if (!a.srow || !a.ids || !a.off) {
        ls_set_error("ls_ivf_search_subset: a subset launch needs the subset's three arrays");
        return LS_ERR_INVALID_ARG;
    }
    if (g.bf16) return ls_ivf_launch_scan_bf16(g, a, s);  // (ls_bf16_ivf.hip)
    if (g.elem == 1) return ls_ivf_launch_scan_subset_sq8(g, a, s);
    return g.elem == 2 ? ivf_subset_launch_dt<true>(g, a, s) : ivf_subset_launch_dt<false>(g, a, s);
}
