// ls_l2_ivf.hip — the probed-list scan (ls_ivf.hip) of an L2 IVF handle (include/leansearch_ivf_l2.h):
// ls_ivf_scan_kernel with the ls_l2_arg tag at the end of its pack, f32 / fp16 rows, the eight shared geometries, in plain
// and row-list form. The tag selects QueryL2 (ls_scan_dev.h) and the row's sum is negated once behind group_sum, so every
// score is -distance with the distance of the flat L2 scan of that row, bit for bit; prefix, fetch, keys and the merge
// are the inner-product kernel's. A translation unit of its own: ls_ivf.hip's and ls_ivf_subset.hip's instantiations
// keep their code. The L2 form of the assignment kernel (ls_ivf_assign_kernel.h: default assignment, ls_ivf_assign_l2,
// the L2 trainer) lives here too, with its launcher.
#include "ls_ivf_assign_kernel.h"
#include "ls_scan_launch.h"

template <bool F16>
static int ivf_l2_launch_dt(const ls_geom& g, const ivf_launch& a, hipStream_t s) {
    return ls_geom_dispatch<false, true>("ls_ivf_search", g, [&](auto L, auto V) -> int {
        return a.srow ? ls_ivf_scan_launch<F16, L(), V()>(g, a, s, a.srow, ls_l2_arg{})
                      : ls_ivf_scan_launch<F16, L(), V()>(g, a, s, ls_l2_arg{});
    });
}

int ls_ivf_launch_scan_l2(const ls_geom& g, const ivf_launch& a, hipStream_t s) {
    if (g.elem == 1) {
        ls_set_error("ls_ivf_search: an L2 launch scans f32 or fp16 rows");
        return LS_ERR_INVALID_ARG;
    }
    if (!a.ids || !a.off) {
        ls_set_error("ls_ivf_search: an L2 launch needs the lists' ids and offsets");
        return LS_ERR_INVALID_ARG;
    }
    return g.elem == 2 ? ivf_l2_launch_dt<true>(g, a, s) : ivf_l2_launch_dt<false>(g, a, s);
}

// ---- assignment ---------------------------------------------------------------------------------------------------------
template <int L, int V, int U>
__global__ __launch_bounds__(LS_SCAN_THREADS) void ls_ivf_assign_l2_kernel(const f32x4* __restrict__ rows, long long n,
                                                                            const f32x4* __restrict__ cent, int nlist,
                                                                            int* __restrict__ assign) {
    ls_ivf_assign_body<L, V, U, true>(rows, n, cent, nlist, assign);
}

int ls_ivf_launch_assign_l2(const ls_geom& g, const void* d_rows, int64_t n, const void* d_cent, int32_t nlist,
                            int32_t* d_assign, int32_t n_cu, hipStream_t s) {
    if (n <= 0) return LS_OK;
    if (g.elem != 4 || nlist < 1 || nlist > LS_IVFB_MAX_NLIST) {
        ls_set_error("ls_ivf_assign_l2: fp32 rows and 1 <= nlist < %d (%d-byte elements, nlist %d)", LS_IVFB_MAX_NLIST + 1,
                     g.elem, nlist);
        return LS_ERR_INVALID_ARG;
    }
    return ls_geom_dispatch<false, true>("ls_ivf_assign_l2", g, [&](auto L, auto V) -> int {
        const int blocks = ls_ivfb_blocks(n, L(), V(), n_cu);
        hipLaunchKernelGGL((ls_ivf_assign_l2_kernel<L(), V(), scan_unroll(V())>), dim3(blocks), dim3(LS_SCAN_THREADS), 0, s,
                           (const f32x4*)d_rows, (long long)n, (const f32x4*)d_cent, nlist, d_assign);
        LS_HIP(hipGetLastError());
        return LS_OK;
    });
}
