// ls_mq_launch.h — the host side of every small-batch launch (ls_mq.hip, ls_mq16.hip, ls_mq8.hip, ls_mq_subset.hip):
// the argument check, the dispatch over keys per lane and query blocks, and the launch itself. A translation unit is
// its kernels and an entry point: the check with its own error text, ls_geom_dispatch (ls_common.h), ls_mq_dispatch,
// then ls_mq_launch with the kernel, its LDS bytes and ceiling, and the kernel's trailing pack: nothing, a.d_step, or
// the row list.
#pragma once
#include "ls_mq_dev.h"

#include <algorithm>

// What every small-batch kernel relies on: `elem` bytes per element, 1..nq_max queries, workgroups of `waves` waves that
// rank waves x keys keys and emit k' + 1 of them into candidate blocks c_stride keys and bound vectors b_stride apart.
static inline bool ls_mq_args_ok(const ls_geom& g, const ls_scan_args& a, int elem, int nq_max, int waves) {
    return g.elem == elem && a.nq >= 1 && a.nq <= nq_max && a.blocks >= 1 && a.kprime >= 1 &&
           a.kprime + 1 <= LS_MQ_KP_MAX && (a.mq_keys == 3 || a.mq_keys == 5 || a.mq_keys == 8) &&
           a.kprime + 1 <= waves * a.mq_keys && (long long)a.blocks * a.kprime <= a.c_stride && a.blocks <= a.b_stride;
}

// f(M, NB) with the keys per lane (3, 5 or 8) and the query blocks (1; 2 for 17..32 queries where the kernel has that
// form: NB2) as std::integral_constant
template <bool NB2, class F>
static int ls_mq_dispatch(const ls_scan_args& a, F&& f) {
    auto blocks = [&](auto m) -> int {
        if constexpr (NB2)
            if (a.nq > LS_MQ_NQ) return f(m, std::integral_constant<int, 2>{});
        return f(m, std::integral_constant<int, 1>{});
    };
    return a.mq_keys == 3   ? blocks(std::integral_constant<int, 3>{})
           : a.mq_keys == 5 ? blocks(std::integral_constant<int, 5>{})
                            : blocks(std::integral_constant<int, 8>{});
}

// One launch of KERN (workgroups of `waves` waves, `smem` bytes of LDS of its own) over n rows - or n positions of a
// row list. It carries the previous launch's selection jobs (a.nfin) and may use the LDS those need, `lds_max` at most:
// LS_PIGGY_LDS_MAX keeps two workgroups per CU, a two-block kernel takes its CU alone (which the block count allows for).
// The kernel is a template VALUE: hipFuncSetAttribute is remembered per kernel and device.
template <auto KERN, class Row, typename... Tail>
static int ls_mq_launch(const char* who, int waves, size_t smem, int lds_max, const Row* corpus, int64_t n,
                        const ls_geom& g, const ls_scan_args& a, hipStream_t s, Tail... tail) {
    if (a.nfin > 0) {
        const ls_fin_params& fp = a.fin.p0;
        const int keff = (int)((long long)fp.k < fp.n ? fp.k : fp.n);
        smem = std::max(smem, ls_fin_lds_bytes(fp.keys_cap, keff));
    }
    const int nfw = std::min(a.nfin, LS_FIN_WG_MAX);  // selection workgroups (jobs nfw.. are second rounds)
    static ls_attr_once once;
    if (smem > (size_t)lds_max) {
        ls_set_error("%s: %zu bytes of LDS for %d-chunk rows, %d queries", who, smem, g.chunks, a.nq);
        return LS_ERR_INVALID_ARG;
    }
    if (int rc = ls_set_max_dynamic_lds(once, (const void*)KERN, lds_max)) return rc;
    hipLaunchKernelGGL(KERN, dim3(a.blocks + nfw), dim3(64 * waves), smem, s, corpus, (long long)n, a.d_q, g.d, a.nq,
                       a.normalize ? 1 : 0, a.d_S, (long long)a.s_stride, a.d_cand, (long long)a.c_stride, a.d_bound,
                       (long long)a.b_stride, a.kprime, nfw, a.fin, a.d_gran, (long long)a.g_stride, a.tag, a.d_qkeep,
                       tail...);
    LS_HIP(hipGetLastError());
    return LS_OK;
}
