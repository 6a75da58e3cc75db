/*
 * leansearch_ivf_subset.h — IVF-flat search over a subset of the rows (libleansearch.so): the IVF form of
 * ls_search_subset / faiss's IDSelector, e.g. "the rows of these packages, among the probed lists".
 *
 * Definitions
 *   - an IVF subset is a set of ORIGINAL rows of one ls_ivf handle (leansearch_ivf.h), given as a bitmap in
 *     ls_subset_create's layout: row r is selected iff (bitmap[r >> 3] >> (r & 7)) & 1; bits at r >= ntotal are ignored;
 *     rows past a short bitmap are not selected. It is compacted once, list after list (inside a list original-row
 *     ascending), and owned by its handle under an int32 id. It covers the rows that existed at its creation:
 *     ls_ivf_add (leansearch_ivf_add.h) keeps it valid and does not extend it, and after ls_ivf_remove
 *     (leansearch_ivf_remove.h) it covers exactly its surviving rows under their new numbers, so a subset never goes stale;
 *     ls_ivf_subset_destroy or ls_ivf_destroy frees it.
 *   - ls_ivf_search_subset returns, per query, what ls_search_subset returns on a flat index of the same rows and dtype
 *     for the bitmap (rows of the probed lists) AND (selected rows).
 *   - the probed lists are chosen exactly as ls_ivf_search chooses them: the top min(nprobe, nlist) centroids over ALL
 *     lists, whatever the selection (faiss, too, applies a selector while it scans lists, not while it probes).
 *   - order: (score descending, original row ascending); padding (-FLT_MAX, -1); NaN / <= -FLT_MAX rows are never
 *     returned; every returned score is bit-identical to the unfiltered single-query scan's score of that row (f32, f16
 *     and sq8); LS_FLAG_NORMALIZE is the only flag, applied once: both stages use that query.
 *   - hence: the all-ones subset equals ls_ivf_search; nprobe >= nlist equals ls_search_subset on the flat index; a
 *     query's result does not depend on the other queries of the call.
 *   - with m selected rows, min(k, m) > LS_MAX_K is LS_ERR_K_TOO_LARGE. m == 0, or no selected row in any list that can
 *     be probed: all padding, nothing is launched.
 * Conventions are leansearch_ivf.h's. Every argument is checked before any device call; calls share the handle's mutex
 * and stream with ls_ivf_search, and ls_ivf_last_kernel_ms reports a subset search like any other.
 */
#ifndef LEANSEARCH_IVF_SUBSET_H
#define LEANSEARCH_IVF_SUBSET_H

#include "leansearch_ivf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bitmap: host bytes [nbytes] (nbytes == 0: nothing selected). *out_id: the subset's id on this handle (>= 1);
 * *out_rows (may be NULL): selected rows m. Costs 8 m + 4 (nlist + 1) bytes of device memory. */
int ls_ivf_subset_create(ls_ivf* ivf, const uint8_t* bitmap, int64_t nbytes, int32_t* out_id, int64_t* out_rows);
int ls_ivf_subset_destroy(ls_ivf* ivf, int32_t subset);

/* selected rows of every list of the handle: out int64 [nlist] */
int ls_ivf_subset_list_sizes(ls_ivf* ivf, int32_t subset, int64_t* out);

/* As ls_ivf_search, over the selected rows of the probed lists. q host float32 [nq, d]; out_scores host float32
 * [nq, k]; out_rows host int64 [nq, k] (original row numbers). nprobe >= 1; min(nprobe, nlist) <= LS_MAX_K.
 * Synchronous. */
int ls_ivf_search_subset(ls_ivf* ivf, int32_t subset, const float* q, int64_t nq, int32_t k, int32_t nprobe,
                         uint32_t flags, float* out_scores, int64_t* out_rows);

#ifdef __cplusplus
}
#endif
#endif /* LEANSEARCH_IVF_SUBSET_H */
