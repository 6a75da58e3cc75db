// ls_l2_scan.hip — LS_METRIC_L2 (include/leansearch_l2.h): the scan kernel's L2 instantiations (plain and
// row-list scan, NQ = 1, f32 and fp16 rows, the eight shared geometries, SMALL and not) and the three entry points of the
// header. A translation unit of its own: the build stays parallel and ls_scan.hip's instantiations keep their code.
#include "ls_scan_launch.h"

#include "ls_index.h"
#include "../../include/leansearch_l2.h"

// ---- scan launches -------------------------------------------------------------------------------------------------
int ls_launch_scan_l2(const void* d_corpus, int64_t n, const ls_geom& g, const ls_scan_args& a, hipStream_t s) {
    if (a.nq == 4 || a.nq == 8) return ls_launch_scan_l2_batch(d_corpus, n, g, a, s);  // (ls_l2_batch.hip)
    if (a.nq != 1 || g.elem == 1) {
        ls_set_error("ls_launch_scan: an L2 launch serves one query over f32 or fp16 rows (nq %d, %d-byte elements)", a.nq, g.elem);
        return LS_ERR_INVALID_ARG;
    }
    return ls_geom_dispatch<false, true>("ls_launch_scan", g, [&](auto L, auto V) -> int {
        return g.elem == 2 ? ls_scan_launch<true, L(), V(), 1>(d_corpus, n, g, a, s, ls_l2_arg{})
                           : ls_scan_launch<false, L(), V(), 1>(d_corpus, n, g, a, s, ls_l2_arg{});
    });
}

int ls_launch_scan_subset_l2(const void* d_corpus, const u32* d_list, int64_t m, const ls_geom& g, const ls_scan_args& a,
                             hipStream_t s) {
    if (g.elem == 1) {
        ls_set_error("ls_launch_scan_subset: an L2 launch scans f32 or fp16 rows");
        return LS_ERR_INVALID_ARG;
    }
    return ls_geom_dispatch<false, true>("ls_launch_scan_subset", g, [&](auto L, auto V) -> int {
        return g.elem == 2 ? ls_scan_launch<true, L(), V(), 1>(d_corpus, m, g, a, s, d_list, ls_l2_arg{})
                           : ls_scan_launch<false, L(), V(), 1>(d_corpus, m, g, a, s, d_list, ls_l2_arg{});
    });
}

// ---- include/leansearch_l2.h -----------------------------------------------------------------------------------------
static int l2_create(ls_index** out, const float* corpus, bool on_device, int64_t n, int32_t d, int32_t dtype, int32_t device,
                     const char* who) {
    if (dtype == LS_DTYPE_SQ8) {  // (before any device check)
        if (out) *out = nullptr;
        ls_set_error("%s: an L2 index stores fp32 or fp16 rows (LS_DTYPE_SQ8 serves the inner product only)", who);
        return LS_ERR_INVALID_ARG;
    }
    if (dtype == LS_DTYPE_BF16) {  // (likewise)
        if (out) *out = nullptr;
        ls_set_error("%s: an L2 index stores fp32 or fp16 rows (bf16 rows, LS_DTYPE_BF16, serve the inner product only)", who);
        return LS_ERR_INVALID_ARG;
    }
    return ls_i_create(out, corpus, on_device, n, d, dtype, nullptr, device, who, LS_METRIC_L2);
}

extern "C" {

int ls_create_l2(ls_index** out, const float* corpus, int64_t n, int32_t d, int32_t dtype, int32_t device) {
    return l2_create(out, corpus, false, n, d, dtype, device, "ls_create_l2");
}

int ls_create_l2_from_device(ls_index** out, const void* d_corpus, int64_t n, int32_t d, int32_t dtype, int32_t device) {
    return l2_create(out, (const float*)d_corpus, true, n, d, dtype, device, "ls_create_l2_from_device");
}

int32_t ls_metric(const ls_index* ix) { return ix ? ix->metric : -1; }

}  // extern "C"
