// ls_bf16_ivf.hip — the probed-list scan (ls_ivf.hip) over bf16 rows (include/leansearch_bf16.h):
// ls_ivf_scan_kernel with the ls_bf16_arg tag at the end of its pack, the eight 2-byte geometries, in plain and row-list
// (IVF subset) form. The tag selects QueryBf16 (ls_scan_dev.h): the same dot / group_sum as the bf16 scan of
// ls_bf16_scan.hip, so every score is bit-identical to the flat scan's of that row; prefix, fetch, keys and the merge are
// the kernel's own. A translation unit of its own: ls_ivf.hip's and ls_ivf_subset.hip's instantiations keep their code.
#include "ls_scan_launch.h"
#include "ls_ivf_state.h"

#include "../../include/leansearch_bf16.h"

int ls_ivf_launch_scan_bf16(const ls_geom& g, const ivf_launch& a, hipStream_t s) {
    if (!g.bf16 || a.l2 || !a.ids || !a.off) {
        ls_set_error("ls_ivf_search: a bf16 launch serves the inner product over bf16 rows and needs the lists' ids and offsets");
        return LS_ERR_INVALID_ARG;
    }
    return ls_geom_dispatch<false, true>("ls_ivf_search", g, [&](auto L, auto V) -> int {
        return a.srow ? ls_ivf_scan_launch<false, L(), V()>(g, a, s, a.srow, ls_bf16_arg{})
                      : ls_ivf_scan_launch<false, L(), V()>(g, a, s, ls_bf16_arg{});
    });
}

extern "C" {

int ls_ivf_bf16_inexact(ls_ivf* v, int64_t* out) {
    if (!v || v->dtype != LS_DTYPE_BF16) {
        ls_set_error("ls_ivf_bf16_inexact: not a bf16 IVF index");
        return LS_ERR_INVALID_ARG;
    }
    if (!out) {
        ls_set_error("ls_ivf_bf16_inexact: out is null");
        return LS_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lk(v->mu);
    *out = v->bf16_inexact;
    return LS_OK;
}

}  // extern "C"
