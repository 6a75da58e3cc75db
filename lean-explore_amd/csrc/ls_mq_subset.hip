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

#ifndef LS_MQS_KERNEL_ONLY  // (scratch builds that instantiate a kernel or two and look at their resources / ISA)
#include "ls_mq_launch.h"
// a.nq = the real query count (1..16) over the m rows of the ascending list d_list; a.blocks / a.kprime / a.mq_keys:
// ls_mq_make_plan (LS_MQ_ROWLIST); score vectors are always written (a.d_S set, m <= a.s_stride); no riding selection
// jobs. 16 queries of 4 KB rows + their key lists stay under LS_PIGGY_LDS_MAX: two workgroups per CU.
int ls_launch_mq_subset(const void* d_corpus, const u32* d_list, int64_t m, const ls_geom& g, const ls_scan_args& a,
                        hipStream_t s) {
    if (m <= 0) return LS_OK;
    if (!ls_mq_args_ok(g, a, 4, LS_MQ_NQ, LS_MQ_WAVES) || !d_corpus || !d_list || !a.d_q || !a.d_S || !a.d_cand ||
        !a.d_bound || a.nfin != 0 || a.d_gran || m > a.s_stride || m > 0xffffffffll) {
        ls_set_error("ls_launch_mq_subset: bad arguments (elem %d nq %d rows %lld blocks %d kprime %d keys %d)", g.elem,
                     a.nq, (long long)m, a.blocks, a.kprime, a.mq_keys);
        return LS_ERR_INVALID_ARG;
    }
    ls_scan_args b{};  // (no jobs, no granules, no tag, no kept queries: the kernel's other arguments are zeros)
    b.d_q = a.d_q, b.nq = a.nq, b.normalize = a.normalize;
    b.d_S = a.d_S, b.s_stride = a.s_stride, b.d_cand = a.d_cand, b.c_stride = a.c_stride;
    b.d_bound = a.d_bound, b.b_stride = a.b_stride, b.blocks = a.blocks, b.kprime = a.kprime, b.mq_keys = a.mq_keys;
    return ls_geom_dispatch<false, true>("ls_launch_mq_subset", g, [&](auto l, auto v) {
        return ls_mq_dispatch<false>(b, [&](auto mk, auto) {
            constexpr int L = decltype(l)::value, V = decltype(v)::value, M = decltype(mk)::value;
            return ls_mq_launch<ls_mq_kernel<L, V, M, 1, LS_MQ_WAVES, const u32*>>(
                "ls_launch_mq_subset", LS_MQ_WAVES, mq_lds_bytes(g.chunks, M, 1, LS_MQ_WAVES), LS_PIGGY_LDS_MAX,
                (const mq_f32x4*)d_corpus, m, g, b, s, d_list);
        });
    });
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
