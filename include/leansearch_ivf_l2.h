/*
 * leansearch_ivf_l2.h — the L2 metric on the IVF-flat index of libleansearch.so: probe, scan, build, add and remove
 * under squared Euclidean distance.
 *
 * Stands in for faiss's `IndexIVFFlat(IndexFlatL2(d), d, nlist)` (METRIC_L2). An L2 IVF handle is an ordinary `ls_ivf`
 * whose metric is fixed at creation: nlist float32 centroids, an assignment row -> list, and the rows as LS_DTYPE_F32 or
 * LS_DTYPE_F16, stored list after list. ls_ivf_search, ls_ivf_search_subset, ls_ivf_range_search(_subset), ls_ivf_add,
 * ls_ivf_remove, ls_ivf_reconstruct, ls_ivf_subset_*, the accessors and the profiling calls work on it as on any handle.
 *
 * Definitions (the distance is leansearch_l2.h's, restated by tests/l2_ref.c)
 *   probe     the probed lists of a query are the top min(nprobe, nlist) rows of ls_search over an ls_create_l2 float32
 *             index of the centroids, bit for bit: distance ascending, then list number ascending. A centroid whose
 *             distance is NaN or >= FLT_MAX is never probed (its probe entry stays -1).
 *   result    what ls_search_subset returns on a flat L2 index of the same rows and dtype for the bitmap of the probed
 *             lists' rows: (distance ascending, original row ascending), padding (+FLT_MAX, -1), every distance
 *             bit-identical to the flat L2 scan's distance for that row. LS_FLAG_NORMALIZE is applied once and both
 *             stages see the same scaled query; with fp16 rows the fine stage rounds the scaled query to fp16 (as the
 *             flat index does) and the coarse stage stays f32. nprobe >= nlist equals ls_search on the flat L2 index. A
 *             query's bits do not depend on its company in the call.
 *   assign    (assign == NULL, at create and at ls_ivf_add) row r goes to the list that the k = 1 L2 search of the
 *             centroid index returns for it: the smallest distance in the scan order with t = centroid_i - row_i (the row
 *             plays the query's role), ties to the lowest list, a row with no valid distance to list 0.
 *   range     row r of a probed list belongs to query i iff dist < radius, strictly; rows ascending inside a segment;
 *             the scores of the result are distances; the radius rules are leansearch_l2.h's.
 *   An index with no probable row (n == 0, or only empty lists can be probed) returns padding only: (+FLT_MAX, -1). The
 *   same holds for the slots past a small subset's rows.
 *
 * Refused with LS_ERR_INVALID_ARG and a message that names L2, before any device check: LS_DTYPE_SQ8 at creation, and
 * ls_ivf_set_small_batch(handle, 1) on an L2 handle. As for every IVF index, d beyond an f32 row geometry (1024) is
 * refused by the centroid index.
 */
#ifndef LEANSEARCH_IVF_L2_H
#define LEANSEARCH_IVF_L2_H

#include "leansearch_ivf_build.h"
#include "leansearch_l2.h"

#ifdef __cplusplus
extern "C" {
#endif

/* As ls_ivf_create, under LS_METRIC_L2; dtype LS_DTYPE_F32 or LS_DTYPE_F16. */
int ls_ivf_create_l2(ls_ivf** out, const float* corpus, int64_t n, int32_t d, int32_t dtype,
                     const float* centroids, int32_t nlist, const int32_t* assign, int32_t device);
int32_t ls_ivf_metric(const ls_ivf* ivf);   /* LS_METRIC_*; -1 for NULL */
/* As ls_ivf_assign, under L2: the default assignment above, one kernel launch per upload step. 1 <= nlist < 8192. */
int ls_ivf_assign_l2(const float* rows, int64_t n, int32_t d, const float* centroids, int32_t nlist,
                     int32_t* out_assign, int32_t device);
/* As ls_ivf_trainer_create; ls_ivf_trainer_assign on this trainer assigns under L2 (the means do not depend on it). */
int ls_ivf_trainer_create_l2(ls_ivf_trainer** out, const float* rows, int64_t n, int32_t d,
                             int32_t nlist, int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* LEANSEARCH_IVF_L2_H */
