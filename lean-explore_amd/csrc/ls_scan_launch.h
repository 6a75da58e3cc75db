// ls_scan_launch.h — the host side of every row-scan launch: one launcher per kernel template (ls_scan_kernel,
// ls_ivf_scan_kernel). The translation units that instantiate the kernels (ls_scan.hip, ls_sq8_scan.hip, ls_ivf.hip,
// ls_sq8_ivf.hip, ls_ivf_subset.hip, ls_sq8_ivf_subset.hip) are an entry point each: their argument checks, then
// ls_geom_dispatch (the table of row geometries: ls_common.h) with a launcher. The trailing arguments of a launcher are
// the kernel's pack: nothing, the row list, ls_sq8_arg{step}, or the list and then the step; ls_l2_arg{} in the step's
// place on an L2 handle (ls_l2_scan.hip), ls_bf16_arg{} on a bf16 handle (ls_bf16_scan.hip, ls_bf16_ivf.hip).
#pragma once
#include "ls_ivf_kernel.h"
#include "ls_scan_kernel.h"

#ifndef LS_SCAN_S  // (ls_scan.hip: the LS_SCAN_ABL_NOS timing ablation passes no score vectors)
#define LS_SCAN_S(x) (x)
#endif

// One launch of ls_scan_kernel<F16, L, V, ., NQ, ., Tail...> over `rows` rows (with a row list: positions of the list;
// a.blocks and a.kprime are the caller's, planned from that count). The SMALL variant where the plan says so. The
// instantiations without a row list carry the previous launch's selection jobs (a.nfin; a row-list launch has none:
// ls_launch_scan_subset refuses them) and may use the LDS those need.
template <bool F16, int L, int V, int NQ, typename... Tail>
static int ls_scan_launch(const void* corpus, int64_t rows, const ls_geom& g, const ls_scan_args& a, hipStream_t s,
                          Tail... tail) {
    constexpr bool SQ8 = ls_pack_sq8<Tail...>::value;
    constexpr bool LIST = sizeof...(Tail) == (SQ8 || ls_pack_l2<Tail...>::value || ls_pack_bf16<Tail...>::value ? 2 : 1);
    constexpr int US = ls_scan_small_unroll(V, SQ8 && LIST);
    size_t smem = 0;
    if (a.nfin > 0) {
        const ls_fin_params& fp = a.fin.p0;
        const int keff = (int)((long long)fp.k < fp.n ? fp.k : fp.n);
        smem = ls_fin_lds_bytes(fp.keys_cap, keff);
    }
    const int nfw = std::min(a.nfin, LS_FIN_WG_MAX);  // selection workgroups (jobs nfw.. are second rounds)
    auto launch = [&](auto small) -> int {
        constexpr bool SM = decltype(small)::value;
        auto kern = ls_scan_kernel<F16, L, V, SM ? US : scan_unroll(V), NQ, SM, Tail...>;
        if constexpr (!LIST) {
            static ls_attr_once once;  // (one per instantiation of this lambda's body, i.e. per kernel)
            if (int rc = ls_set_max_dynamic_lds(once, (const void*)kern, LS_PIGGY_LDS_MAX)) return rc;
        }
        hipLaunchKernelGGL(kern, dim3(a.blocks + nfw), dim3(LS_SCAN_THREADS), smem, s, (const f32x4*)corpus,
                           (long long)rows, g.chunks, a.d_q, g.d, a.normalize ? 1 : 0, a.reverse ? 1 : 0,
                           LS_SCAN_S(a.d_S), (long long)a.s_stride, a.d_cand, (long long)a.c_stride, a.d_bound,
                           (long long)a.b_stride, a.kprime, nfw, a.fin, a.d_gran, (long long)a.g_stride, a.tag,
                           a.d_qkeep, tail...);
        LS_HIP(hipGetLastError());
        return LS_OK;
    };
    if constexpr (NQ == 1) {
        if (ls_scan_is_small(rows, a.blocks, ls_scan_tile_rows(L, US), NQ)) return launch(std::true_type{});
    }
    return launch(std::false_type{});
}

// One launch of ls_ivf_scan_kernel<F16, L, V, ., Tail...>
template <bool F16, int L, int V, typename... Tail>
static int ls_ivf_scan_launch(const ls_geom& g, const ivf_launch& a, hipStream_t s, Tail... tail) {
    hipLaunchKernelGGL((ls_ivf_scan_kernel<F16, L, V, scan_unroll(V), Tail...>), dim3(a.blocks), dim3(LS_SCAN_THREADS), 0,
                       s, (const f32x4*)a.corpus, g.chunks, a.ids, a.off, a.probe, a.nprobe, a.q, g.d,
                       a.normalize ? 1 : 0, a.S, a.cand, a.bound, a.kprime, tail...);
    LS_HIP(hipGetLastError());
    return LS_OK;
}
