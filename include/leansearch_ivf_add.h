/*
 * leansearch_ivf_add.h — adding rows to a built IVF-flat handle of libleansearch.so: the other half of the reference's
 * build pair `index.train(x); index.add(x)` (reference src/lean_explore/extract/index.py:110-116). The lists are merged
 * in HBM: the stored rows never return to the host and are never re-encoded.
 *
 * Definition. After a successful ls_ivf_add the handle is, in everything observable, the handle
 * ls_ivf_create would have made from the old rows followed by the new rows, with the same centroids and the
 * concatenated assignment: ls_ivf_ntotal, ls_ivf_list_sizes, ls_ivf_assignment, ls_ivf_reconstruct, every ls_ivf_search
 * result, ls_ivf_search_subset on subsets created afterwards, the small-batch pass and its ls_ivf_last_passes. New rows
 * get the original row numbers ntotal .. ntotal + n_add - 1; rows stay stored list after list, ascending by original
 * row inside a list, so every list is its old rows followed by its new rows in call order.
 *   - storage: fp16 rows are rounded as ls_create rounds them; sq8 rows are encoded with the handle's existing step,
 *     which is fixed for the life of the handle (leansearch_sq8.h) and never retrained. The stored bytes of the old rows
 *     are moved, not encoded again.
 *   - assign_or_null == NULL: the lists are computed by ls_ivf_create(assign = NULL)'s rule, bit for bit, the same way
 *     (the library's exact k = 1 search over the centroids on the float32 row, ties to the lowest list, a row no
 *     centroid scores to list 0). As leansearch_ivf_build.h remarks, that search is single-valued only below 8192 lists.
 *   - existing subsets of the handle (leansearch_ivf_subset.h) stay valid and keep covering the rows that existed at
 *     their creation - the flat index's rule ("ls_add does not extend it", leansearch.h). ls_ivf_set_small_batch and
 *     ls_ivf_set_profiling keep their values.
 *   - all or nothing: the new storage is built BESIDE the old one and swapped in under the handle's mutex only when it
 *     is complete. On any failure, out of device memory included, the handle is unchanged and still searchable. The
 *     price is a transient second copy in HBM: for the length of the call the device holds the old stored rows, the new
 *     rows (a flat index of them) and the merged storage of both.
 *   - every argument is checked before any device call. n_add == 0 returns LS_OK and touches nothing;
 *     ntotal + n_add must stay below 2^32 - 1; an assign entry outside [0, nlist) is LS_ERR_INVALID_ARG with its index
 *     in the message, as ls_ivf_create reports it.
 * Conventions are leansearch.h's. Synchronous; serialised with the handle's other calls.
 */
#ifndef LEANSEARCH_IVF_ADD_H
#define LEANSEARCH_IVF_ADD_H

#include "leansearch_ivf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rows: host float32 [n_add, d]; assign_or_null: host int32 [n_add] (0 <= assign[j] < nlist) or NULL. */
int ls_ivf_add(ls_ivf* ivf, const float* rows, int64_t n_add, const int32_t* assign_or_null);

/* With ls_ivf_set_profiling on: the time of the most recent ls_ivf_add's merge kernel (hipEvents on the handle's
 * stream) and the bytes it moved (every stored row read once and written once); zeros when none was timed. Either
 * pointer may be NULL. */
int ls_ivf_add_last_kernel_ms(ls_ivf* ivf, float* merge_ms, int64_t* merge_bytes);

#ifdef __cplusplus
}
#endif
#endif /* LEANSEARCH_IVF_ADD_H */
