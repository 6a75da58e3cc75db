/*
 * leansearch_ivf_remove.h — removing rows from a built IVF-flat handle of libleansearch.so: the counterpart of
 * leansearch_ivf_add.h, and faiss's `index.remove_ids(sel)`. With it an update of the index is ls_ivf_remove(stale)
 * followed by ls_ivf_add(fresh) on rows that never leave HBM. The lists are compacted in HBM: the stored rows never
 * return to the host and are never decoded or re-encoded.
 *
 * Definition. After a successful ls_ivf_remove the handle is, in everything observable, the
 * handle ls_ivf_create would have made from the surviving rows in their order, with the same centroids and the
 * surviving assignment: ls_ivf_ntotal, ls_ivf_list_sizes, ls_ivf_assignment, ls_ivf_reconstruct, every ls_ivf_search
 * result (scores and rows bit for bit), the small-batch pass and its ls_ivf_last_passes, ls_ivf_search_subset on
 * subsets created afterwards, and a later ls_ivf_add.
 *   - numbering: survivors are renumbered densely. Old row r becomes r - (removed rows below r), as faiss's
 *     IndexFlat.remove_ids renumbers - NOT faiss's IVF rule of keeping the ids: every structure of this library equates
 *     "id" with "row < ntotal". A caller that keeps a positional id map deletes the same positions from it.
 *   - storage: rows stay stored list after list, ascending by original row inside a list (the renumbering is monotone,
 *     so the order inside a list is kept). Stored bytes are moved: fp16 and sq8 rows keep their bytes, and the sq8 step
 *     stays as it is (it is fixed for the life of the handle, leansearch_sq8.h, and never retrained).
 *   - existing subsets of the handle (leansearch_ivf_subset.h) stay valid: each afterwards covers exactly its surviving
 *     rows under their new numbers, list after list, ascending inside a list. A subset may become empty; a search of it
 *     returns all padding. ls_ivf_subset_list_sizes reports the new sizes.
 *   - all or nothing: the compacted storage, its row ids and offsets and the new arrays of every existing subset are
 *     built BESIDE the handle under its mutex and swapped in only when complete; the swap allocates nothing. On any
 *     failure, out of device memory included, the handle and its subsets are unchanged and searchable. The price is a
 *     transient second copy in HBM: the old stored rows plus the surviving stored rows at the peak.
 *     ls_ivf_set_small_batch and ls_ivf_set_profiling keep their values.
 *   - nothing selected below ntotal: LS_OK, nothing touched, 0 removed. Everything selected: ntotal == 0; the handle
 *     is searchable (every result is padding) and takes ls_ivf_add afterwards.
 *   - every argument is checked before any device call: a null handle, nbytes < 0 and a null bitmap with nbytes > 0 are
 *     LS_ERR_INVALID_ARG with the function's name in the message.
 * Conventions are leansearch.h's. Synchronous; serialised with the handle's other calls.
 */
#ifndef LEANSEARCH_IVF_REMOVE_H
#define LEANSEARCH_IVF_REMOVE_H

#include "leansearch_ivf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bitmap: ls_subset_create's layout over ORIGINAL rows: row r is removed iff (bitmap[r >> 3] >> (r & 7)) & 1. Bits at
 * r >= ntotal are ignored; rows past a short bitmap are kept. *out_removed (may be NULL): the rows removed. */
int ls_ivf_remove(ls_ivf* ivf, const uint8_t* bitmap, int64_t nbytes, int64_t* out_removed);

/* With ls_ivf_set_profiling on: the time of the most recent ls_ivf_remove's row-compaction kernel (hipEvents on the
 * handle's stream) and the bytes it moved (every surviving stored row read once and written once); zeros when none was
 * timed. Either pointer may be NULL. */
int ls_ivf_remove_last_kernel_ms(ls_ivf* ivf, float* compact_ms, int64_t* compact_bytes);

#ifdef __cplusplus
}
#endif
#endif /* LEANSEARCH_IVF_REMOVE_H */
