// ls_mq_subset.hip — subset search, small batches on an fp32 index (opt-in: ls_set_subset_small_batch): 2..16 queries
// share ONE pass over the m selected rows of a subset (ls_subset.hip), with the inner products on the f32 matrix cores
// and BIT-IDENTICAL to the single-query row-list scan.
//
// Replaces faiss `index.search(X, k, params=SearchParameters(sel=...))` with more than one row in X (the reference's
// own call is src/lean_explore/search/engine.py:238-250 with one query and no selector), which the subset path served
// with one row-list scan launch and one finalize launch per query: the selected rows were read once per query.
//
// Roofline: HBM over the selected rows. One pass reads m * d * 4 bytes of rows and m * 4 bytes of list once, for up to
// 16 queries; the matrix work is ls_mq.hip's (m * d / 64 v_mfma_f32_16x16x4_f32 of 32 cycles: a third of the HBM time at
// every row length). Small subsets are bound by the launch floor instead. Measured (tools/subset_small_batch_time.py,
// DESIGN.md 4.7b; pass + the group's finalize launch, 16 queries, N = 200 k): all rows 61.8 us at d = 384 / 180.9 us at
// d = 1024 (16 launch pairs: 899 / 2171 us; a plain 16-query ls_mq call with score vectors + its finalize: 66.5 / 183.1);
// a random 10 % subset 21.5 / 44.2 us (336 / 539).
//
// The kernel is ls_mq_kernel (ls_mq_kernel.h) with a row list: one B block, four waves, the eight fp32 row geometries x
// 3 / 5 / 8 keys per lane. It works in list POSITIONS, as the row-list scan does: a tile is 16
// consecutive positions of [0, m), lane (li, kq) loads chunk cb + kq of row list[t * 16 + li], and the score vectors,
// keys, bounds and the selection see an index of m rows. The list is ascending, so ties stay row-ascending. The lane
// transpose, the chain and group order, the add tree, the key lists and the query staging are the plain pass's text:
// ls_mq's scores are the scan kernel's bits, the row-list scan's are the plain scan's, and so these are.
//
// Its own translation unit: ls_mq.hip's 48 instantiations keep their code, and the 24 kernels here
// build beside them.
#include "ls_mq_kernel.h"

#include <algorithm>

#ifndef LS_MQS_KERNEL_ONLY  // (scratch builds that instantiate a kernel or two and look at their resources / ISA)
template <int L, int V, int M>
static int mqs_launch(const void* corpus, const u32* list, int64_t m, const ls_geom& g, const ls_scan_args& a,
                      hipStream_t s) {
    const size_t smem = mq_lds_bytes(g.chunks, M, 1, LS_MQ_WAVES);
    auto kern = ls_mq_kernel<L, V, M, 1, LS_MQ_WAVES, const u32*>;
    static ls_attr_once once;
    // (16 queries of 4 KB rows + their key lists stay under LS_PIGGY_LDS_MAX: two workgroups per CU)
    if (smem > (size_t)LS_PIGGY_LDS_MAX) {
        ls_set_error("ls_launch_mq_subset: %zu bytes of LDS for %d-chunk rows", smem, g.chunks);
        return LS_ERR_INVALID_ARG;
    }
    if (int rc = ls_set_max_dynamic_lds(once, (const void*)kern, LS_PIGGY_LDS_MAX)) return rc;
    hipLaunchKernelGGL(kern, dim3(a.blocks), dim3(64 * LS_MQ_WAVES), smem, s, (const mq_f32x4*)corpus, (long long)m,
                       a.d_q, g.d, a.nq, a.normalize ? 1 : 0, a.d_S, (long long)a.s_stride, a.d_cand,
                       (long long)a.c_stride, a.d_bound, (long long)a.b_stride, a.kprime, 0, ls_fin_batch{},
                       (void*)nullptr, 0ll, 0u, (float*)nullptr, list);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// a.nq = the real query count (1..16) over the m rows of the ascending list d_list; a.mq_keys = 3, 5 or 8
// (ls_mq_subset_plan.h); score vectors are always written (a.d_S set, m <= a.s_stride); no riding selection jobs
int ls_launch_mq_subset(const void* d_corpus, const u32* d_list, int64_t m, const ls_geom& g, const ls_scan_args& a,
                        hipStream_t s) {
    if (m <= 0) return LS_OK;
    if (g.elem != 4 || !d_corpus || !d_list || !a.d_q || !a.d_S || !a.d_cand || !a.d_bound || a.nq < 1 ||
        a.nq > LS_MQ_NQ || a.nfin != 0 || a.d_gran || a.blocks < 1 || a.kprime < 1 || a.kprime + 1 > LS_MQ_KP_MAX ||
        (a.mq_keys != 3 && a.mq_keys != 5 && a.mq_keys != 8) || a.kprime + 1 > LS_MQ_WAVES * a.mq_keys ||
        (long long)a.blocks * a.kprime > a.c_stride || a.blocks > a.b_stride || m > a.s_stride || m > 0xffffffffll) {
        ls_set_error("ls_launch_mq_subset: bad arguments (elem %d nq %d rows %lld blocks %d kprime %d keys %d)", g.elem,
                     a.nq, (long long)m, a.blocks, a.kprime, a.mq_keys);
        return LS_ERR_INVALID_ARG;
    }
#define LS_CASE(LL, VV)                                                                   \
    if (g.L == LL && g.V == VV)                                                           \
        return a.mq_keys == 3 ? mqs_launch<LL, VV, 3>(d_corpus, d_list, m, g, a, s)       \
             : a.mq_keys == 5 ? mqs_launch<LL, VV, 5>(d_corpus, d_list, m, g, a, s)       \
                              : mqs_launch<LL, VV, 8>(d_corpus, d_list, m, g, a, s);
    LS_CASE(16, 1) LS_CASE(16, 2) LS_CASE(16, 3) LS_CASE(16, 4)
    LS_CASE(32, 3) LS_CASE(32, 4)
    LS_CASE(64, 3) LS_CASE(64, 4)
#undef LS_CASE
    ls_set_error("ls_launch_mq_subset: unsupported row geometry L=%d V=%d", g.L, g.V);
    return LS_ERR_INVALID_ARG;
}
#else
#ifndef LS_MQS_ONLY_L
#define LS_MQS_ONLY_L 16
#endif
#ifndef LS_MQS_ONLY_V
#define LS_MQS_ONLY_V 3
#endif
template __global__ void ls_mq_kernel<LS_MQS_ONLY_L, LS_MQS_ONLY_V, 3, 1, LS_MQ_WAVES, const u32*>(
    const mq_f32x4*, long long, const float*, int, int, int, float*, long long, u64*, long long, u64*, long long, int, int,
    ls_fin_batch, void*, long long, u32, float*, const u32*);
template __global__ void ls_mq_kernel<LS_MQS_ONLY_L, LS_MQS_ONLY_V, 8, 1, LS_MQ_WAVES, const u32*>(
    const mq_f32x4*, long long, const float*, int, int, int, float*, long long, u64*, long long, u64*, long long, int, int,
    ls_fin_batch, void*, long long, u32, float*, const u32*);
#endif  // LS_MQS_KERNEL_ONLY
