// ls_sq8_ivf.hip — the probed-list scan (ls_ivf.hip) over sq8 rows: ls_ivf_scan_kernel with QuerySq8, ten geometries.
// The same dot / group_sum as the sq8 scan of ls_sq8_scan.hip, so every score is bit-identical to the flat scan's.
#include "ls_scan_launch.h"

int ls_ivf_launch_scan_sq8(const ls_geom& g, const ivf_launch& a, hipStream_t s) {
    if (!a.step) {
        ls_set_error("ls_ivf_search: an sq8 launch needs the step");
        return LS_ERR_INVALID_ARG;
    }
    return ls_geom_dispatch<true, true>("ls_ivf_search", g, [&](auto L, auto V) -> int {
        return ls_ivf_scan_launch<false, L(), V()>(g, a, s, ls_sq8_arg{a.step});
    });
}
