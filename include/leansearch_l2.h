/*
 * leansearch_l2.h — the L2 metric of libleansearch.so: exact squared-distance top-k and range search on the flat index.
 *
 * Stands in for faiss's `IndexFlatL2(d)` (METRIC_L2, file fourcc IxF2): `index.search(x, k)` returns SQUARED Euclidean
 * distances, smallest first. An L2 handle is an ordinary `ls_index` whose metric is fixed at creation; its storage is
 * LS_DTYPE_F32 or LS_DTYPE_F16. ls_search, ls_search_subset, ls_range_search(_subset), ls_add, ls_remove,
 * ls_reconstruct, ls_subset_create, ls_set_base, ls_ntotal and the other accessors work on it as on any handle.
 *
 * Definitions (tests/l2_ref.c restates the distance)
 *   distance  of query q to stored row x, in the scan's geometry: the row is chunks = L * V chunks of 16 bytes, and lane
 *             `sub` of the row's L lanes takes chunks sub, sub + L, .. (as for the inner product).
 *             f32: each lane runs ONE chain from 0 over its 4 * V elements in memory order: t = x_i - q_i (one rounded
 *               float32 subtraction), then acc = fmaf(t, t, acc). q_i is the query element after the optional
 *               LS_FLAG_NORMALIZE scaling: q_i * inv rounded to float32 BEFORE the subtraction.
 *             f16: the row elements are the stored fp16 values; the query is scaled, then rounded to fp16, as
 *               LS_DTYPE_F16 does for the inner product; both are converted to float32 exactly and the chain is the
 *               f32 one, over 8 * V elements.
 *             The L partial sums are combined by the balanced xor tree (lane ^ 1, ^ 2, ^ 4, ..). Padding elements are
 *             zero in both operands and add exactly 0.
 *   score     the kernels work on s = -dist; the caller receives 0.0f - s, so an exact match returns +0.0.
 *   order     distance ascending, then row ascending. Slots past the valid rows hold index -1 and distance +FLT_MAX
 *             (faiss's max-heap neutral value: the mirror image of leansearch.h's padding). Rows whose distance is NaN
 *             or >= FLT_MAX are never returned. k, LS_MAX_K, ls_set_base and the subset rules are leansearch.h's.
 *   range     row r belongs to query i iff dist(i, r) < radius (strict, as faiss does for L2); rows ascending inside a
 *             segment, the scores of the result are distances. radius = +inf returns every valid row; radius <= 0, -inf
 *             or NaN returns nothing.
 *   A query's bits depend neither on the other queries of the call nor on the entry point (ls_search,
 *   ls_search_subset, the range calls): every query is served alone by the scan path, one launch per query - or, with
 *   ls_set_l2_small_batch (leansearch_l2_batch.h, off by default), in groups of 8 / 4 / 1 per corpus pass: the same bits.
 *
 * Refused with LS_ERR_INVALID_ARG and a message that names L2 (argument errors come before any device check):
 * LS_DTYPE_SQ8 at creation; on an L2 handle ls_search_device (any flags), ls_set_f16_small_batch,
 * ls_set_sq8_small_batch, ls_set_subset_small_batch and ls_export_flags. There are no sharded or replicated L2 creators.
 * The IVF creators of leansearch_ivf.h build inner-product indexes; an L2 IVF index is leansearch_ivf_l2.h's.
 */
#ifndef LEANSEARCH_L2_H
#define LEANSEARCH_L2_H

#include "leansearch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LS_METRIC_INNER_PRODUCT 0
#define LS_METRIC_L2 1

/* corpus: host float32 [n, d]; dtype LS_DTYPE_F32 or LS_DTYPE_F16. n == 0 is allowed. */
int ls_create_l2(ls_index** out, const float* corpus, int64_t n, int32_t d, int32_t dtype, int32_t device);
/* ... with the rows already in HBM on `device`, row-major float32 [n, d] */
int ls_create_l2_from_device(ls_index** out, const void* d_corpus, int64_t n, int32_t d, int32_t dtype, int32_t device);
/* LS_METRIC_* of any handle: LS_METRIC_INNER_PRODUCT for every other creator's; -1 for NULL */
int32_t ls_metric(const ls_index* index);

#ifdef __cplusplus
}
#endif
#endif /* LEANSEARCH_L2_H */
