/*
 * leansearch_ivf.h — IVF-flat search of libleansearch.so: probe `nprobe` inverted lists, scan only their rows.
 *
 * Stands in for `faiss.IndexIVFFlat(IndexFlatIP(d), d, nlist, METRIC_INNER_PRODUCT)` searched with `index.nprobe = 64`,
 * which is the index the reference ships and searches (reference src/lean_explore/extract/index.py:95-116,
 * search/engine.py:247-250). Opt-in: the exact flat search of leansearch.h stays the default and is untouched.
 *
 * Definitions (faiss leaves tie and summation order open; this library fixes them, DESIGN.md sections 1 and 4.8)
 *   - an index is `nlist` centroids (float32 [nlist, d]), an assignment row -> list, and the rows (LS_DTYPE_*).
 *   - probe: the probed lists of a query are the top min(nprobe, nlist) rows of ls_search over a float32 index of the
 *     centroids, bit for bit (order: score descending, list number ascending).
 *   - result: what ls_search_subset returns on a flat index of the same rows and dtype for the bitmap of the probed
 *     lists' rows: (score descending, ORIGINAL row ascending), (-FLT_MAX, -1) padding, NaN / <= -FLT_MAX rows never
 *     returned, every score bit-identical to the unfiltered single-query scan's, LS_FLAG_NORMALIZE applied once (both
 *     stages use the same normalised query). nprobe >= nlist therefore equals ls_search on the flat index.
 *   - a query's result does not depend on the other queries of the call. Empty lists are legal.
 * This is a subset-search result by definition; it is NOT claimed to match faiss bit for bit.
 *
 * Conventions are leansearch.h's: LS_OK or a negative LS_ERR_* code, thread-local message in ls_last_error(), no CPU
 * fallback (LS_ERR_NO_DEVICE without a GPU). Calls on one handle are serialised inside; the handle has its own stream.
 */
#ifndef LEANSEARCH_IVF_H
#define LEANSEARCH_IVF_H

#include "leansearch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ls_ivf ls_ivf; /* opaque; single device */

/* corpus: host float32 [n, d] (n == 0 allowed); centroids: host float32 [nlist, d], nlist >= 1; assign: host int32 [n],
 * the list of every row (0 <= assign[r] < nlist), or NULL: row r goes to the list whose centroid has the largest inner
 * product with the float32 row, ties to the lowest list number, computed by the library's own exact k = 1 search (a row
 * no centroid scores - NaN - goes to list 0). The rows are stored list after list, ascending by original row inside a
 * list: one copy of the corpus in HBM. */
int ls_ivf_create(ls_ivf** out, const float* corpus, int64_t n, int32_t d, int32_t dtype, const float* centroids,
                  int32_t nlist, const int32_t* assign, int32_t device);

/* q host float32 [nq, d]; out_scores host float32 [nq, k]; out_rows host int64 [nq, k] (original row numbers).
 * nprobe >= 1; min(nprobe, nlist) <= LS_MAX_K. flags: LS_FLAG_NORMALIZE only. LS_ERR_K_TOO_LARGE when
 * min(k, rows of the index) exceeds LS_MAX_K. Synchronous. */
int ls_ivf_search(ls_ivf* ivf, const float* q, int64_t nq, int32_t k, int32_t nprobe, uint32_t flags, float* out_scores,
                  int64_t* out_rows);

int64_t ls_ivf_ntotal(const ls_ivf* ivf);
int32_t ls_ivf_dim(const ls_ivf* ivf);
int32_t ls_ivf_nlist(const ls_ivf* ivf);
int ls_ivf_list_sizes(const ls_ivf* ivf, int64_t* out /* [nlist] */);
int ls_ivf_assignment(const ls_ivf* ivf, int32_t* out /* [ntotal]: the list of every row */);
void ls_ivf_destroy(ls_ivf* ivf);

/* Kernel timing (hipEvents on the handle's stream, off by default): with profiling on, every query of a search records
 * coarse = the centroid search, fine = the probed-list scan + its selection. ls_ivf_last_kernel_ms returns the sums over
 * the queries of the most recent search (up to 64 of them) and, optionally, how many of its queries needed the second,
 * always-exact launch. */
int ls_ivf_set_profiling(ls_ivf* ivf, int32_t enabled);
int ls_ivf_last_kernel_ms(ls_ivf* ivf, float* coarse_ms, float* fine_ms, int32_t* rescued);

#ifdef __cplusplus
}
#endif
#endif /* LEANSEARCH_IVF_H */
