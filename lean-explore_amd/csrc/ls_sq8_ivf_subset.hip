// ls_sq8_ivf_subset.hip — the probed-list scan over an IVF subset (ls_ivf_subset.hip) of sq8 rows: ls_ivf_scan_kernel
// with a row list and QuerySq8. An IVF index has at most 1024 dimensions (its centroids are an f32 index), i.e. at most
// 64 chunks of 16 codes: six geometries; the four that begin past d = 1024 cannot be reached and are not built.
#include "ls_scan_launch.h"

int ls_ivf_launch_scan_subset_sq8(const ls_geom& g, const ivf_launch& a, hipStream_t s) {
    if (!a.step || !a.srow) {
        ls_set_error("ls_ivf_search_subset: an sq8 launch needs the step and the row list");
        return LS_ERR_INVALID_ARG;
    }
    return ls_geom_dispatch<true, false>("ls_ivf_search_subset", g, [&](auto L, auto V) -> int {
        return ls_ivf_scan_launch<false, L(), V()>(g, a, s, a.srow, ls_sq8_arg{a.step});
    });
}
