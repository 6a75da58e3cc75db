/*
 * leansearch_range.h — range search of libleansearch.so: every row whose score exceeds a radius, on flat and IVF
 * handles and their row subsets.
 *
 * Stands in for faiss's `index.range_search(x, radius)` -> (lims, D, I) under METRIC_INNER_PRODUCT on the index kinds
 * this library serves (IndexFlatIP, IndexScalarQuantizer, IndexIVFFlat).
 *
 * Definitions (faiss leaves the order inside a query's segment open; this library fixes it)
 *   - the result of query i is the set of rows r with  s(i, r) > radius  (strict, as faiss does for inner product),
 *     s not NaN, and s > -FLT_MAX (the library's "never returned" rule).
 *   - s(i, r) is the score the SINGLE-QUERY scan path gives that row, bit for bit: the scores ls_search returns on an
 *     f32 or sq8 index, and the option-off scan kernel's on an f16 index. ls_search_subset stays on that kernel when
 *     ls_set_f16_small_batch is on; range search does the same, so an f16 handle's range result does not depend on the
 *     option. LS_FLAG_NORMALIZE is applied once, inside the scan (and, on an IVF handle, to both stages).
 *   - flat subset: only the selected rows. IVF: only rows of the probed lists, which are chosen exactly as
 *     ls_ivf_search chooses them (the same coarse search, min(nprobe, nlist) lists). IVF subset: probed AND selected.
 *   - inside a query's segment the rows are ORIGINAL ROW ASCENDING. A flat handle's base (ls_set_base) is added, as
 *     ls_search adds it.
 *   - lims is int64 [nq + 1] with lims[0] = 0; query i owns [lims[i], lims[i + 1]) of scores (float32) and rows (int64).
 *   - one radius applies to all queries of the call. radius = -inf returns every valid row, radius = +inf or NaN
 *     returns nothing: plain comparison semantics, no special case and no error.
 *   - nq = 0 is legal (lims = [0]). An empty index, an empty subset, or no probeable row launches nothing.
 *   - a query's result does not depend on the other queries of the call. There is no cap on the result size.
 * Consequences: for any k <= LS_MAX_K with at least as many slots as hits, the range result equals the ls_search (or
 * ls_search_subset / ls_ivf_search / ls_ivf_search_subset) result filtered by score > radius and re-sorted by row; and
 * an IVF handle with nprobe >= nlist equals the flat range search of the same rows.
 *
 * On an L2 handle (leansearch_l2.h) the result of query i is the set of rows with dist(i, r) < radius, the scores are distances
 * and the radius rules mirror: +inf returns every valid row; <= 0, -inf or NaN nothing. Everything else above holds.
 *
 * Conventions are leansearch.h's: LS_OK or a negative LS_ERR_* code, thread-local message in ls_last_error(), no CPU
 * fallback (LS_ERR_NO_DEVICE without a GPU). Every entry point is synchronous, takes host pointers, checks every
 * argument before any device call and is all or nothing: on an error *out stays NULL and nothing leaks. The flat entry
 * points wait until no synchronous host search is in flight and take the handle, as ls_search_subset does; the IVF
 * entry points share the handle's mutex and stream with ls_ivf_search. flags: LS_FLAG_NORMALIZE only - any other flag
 * is LS_ERR_INVALID_ARG. Sharded and replicated flat handles are refused (LS_ERR_INVALID_ARG, before any device is
 * touched).
 */
#ifndef LEANSEARCH_RANGE_H
#define LEANSEARCH_RANGE_H

#include "leansearch.h"
#include "leansearch_ivf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ls_range_result ls_range_result; /* host memory, owned by the library until ls_range_free */

/* q host float32 [nq, d]. */
int ls_range_search(ls_index* index, const float* q, int64_t nq, float radius, uint32_t flags, ls_range_result** out);
/* ... over the rows of `subset` (ls_subset_create) only */
int ls_range_search_subset(ls_index* index, int32_t subset, const float* q, int64_t nq, float radius, uint32_t flags,
                           ls_range_result** out);
/* nprobe >= 1; min(nprobe, nlist) <= LS_MAX_K. Rows are original row numbers. */
int ls_ivf_range_search(ls_ivf* ivf, const float* q, int64_t nq, float radius, int32_t nprobe, uint32_t flags,
                        ls_range_result** out);
/* ... over the rows of `subset` (ls_ivf_subset_create) in the probed lists only */
int ls_ivf_range_search_subset(ls_ivf* ivf, int32_t subset, const float* q, int64_t nq, float radius, int32_t nprobe,
                               uint32_t flags, ls_range_result** out);

int64_t ls_range_nq(const ls_range_result* r);
const int64_t* ls_range_lims(const ls_range_result* r);  /* [nq + 1] */
const float* ls_range_scores(const ls_range_result* r);  /* [lims[nq]] (may be NULL when that is 0) */
const int64_t* ls_range_rows(const ls_range_result* r);  /* [lims[nq]] (may be NULL when that is 0) */
/* Kernel timing: with profiling on (ls_set_profiling / ls_ivf_set_profiling) the hipEvent time of the call's count,
 * offsets and emit launches alone, summed over its groups of queries, in ms; 0 otherwise. */
float ls_range_kernel_ms(const ls_range_result* r);
void ls_range_free(ls_range_result* r); /* NULL is fine */

#ifdef __cplusplus
}
#endif
#endif /* LEANSEARCH_RANGE_H */
