/*
 * leansearch_remove.h — removing rows from a built flat handle (ls_index) of libleansearch.so: the counterpart of
 * ls_add, and faiss's `IndexFlat.remove_ids(sel)`. With it an update of the index is ls_remove(stale) followed by
 * ls_add(fresh) on rows that never leave HBM. The corpus is compacted IN PLACE through a bounded staging buffer: no
 * second copy of the stored rows exists at any time, so a handle that fills the card can still lose rows.
 *
 * Definition. After a successful ls_remove the handle is, in everything observable, the
 * handle ls_create (ls_create_sq8, ls_create_sharded, ls_create_replicated) would have made from the surviving rows
 * in their order, with the same dtype, ls_set_base and switches: ls_ntotal and ls_reconstruct, ls_sq8_codes and
 * ls_sq8_step, every search result (scores and rows bit for bit) through every path - host, device, pipelined, the
 * small-batch passes, the batched passes -, ls_search_subset on subsets created afterwards, and a later ls_add.
 *   - bitmap: ls_subset_create's layout. Row r is removed iff (bitmap[r >> 3] >> (r & 7)) & 1; rows are numbered
 *     without the ls_set_base offset. Bits at r >= ntotal are ignored; rows past a short bitmap are kept.
 *   - numbering: survivors are renumbered densely, as faiss's IndexFlat.remove_ids and ls_ivf_remove renumber. Old row
 *     r becomes r - (removed rows below r). A caller that keeps a positional id map deletes the same positions from it.
 *   - storage: stored bytes are moved, never decoded or re-encoded: fp16 and sq8 rows keep their bytes, and the sq8
 *     step stays as it is (it is fixed for the life of the handle, leansearch_sq8.h, and never retrained).
 *   - existing subsets of the handle (ls_subset_create) stay valid: each afterwards covers exactly its surviving rows
 *     under their new numbers, ascending. ls_subset_rows reports the new size. A subset may become empty; a search of
 *     it returns all padding.
 *   - pending work: before a row is touched the call does what ls_add does - it waits for the synchronous host calls
 *     in flight, drains the scan lanes, repairs the unchecked batched calls and synchronises the device. Pipelined
 *     device calls queued before the removal therefore get their final results from the index as it was.
 *   - failure: every argument is checked before any device call: a null handle, nbytes < 0 and a null bitmap with
 *     nbytes > 0 are LS_ERR_INVALID_ARG with the function's name and the offending argument in the message. The whole
 *     plan, every allocation and every existing subset's new list (device and host copies) are made BEFORE the first
 *     row moves: a failure up to that point, out of device memory included, leaves the handle and its subsets unchanged
 *     and searchable. From there on only kernel launches and device-to-device copies on the handle's stream remain; a
 *     HIP error from those returns LS_ERR_HIP and leaves the handle fit only for ls_destroy.
 *   - nothing selected below ntotal: LS_OK, nothing touched, 0 removed. Everything selected: ntotal == 0; the handle
 *     is searchable (every result is padding) and takes ls_add afterwards.
 *   - the row capacity, the score vectors and the scratch are kept: ls_remove(stale) followed by ls_add(fresh) of no
 *     more rows allocates nothing for the corpus.
 *   - group handles: every member (shard / replica) is prepared first, and rows move only when all are. A replicated
 *     handle hands every replica the same bitmap (and refuses when an earlier add left the replicas inconsistent); a
 *     sharded handle hands shard g its own bits, and the shards' row blocks are contiguous again afterwards (a shard
 *     may end with 0 rows).
 * Conventions are leansearch.h's. Synchronous; serialised with the handle's other calls.
 */
#ifndef LEANSEARCH_REMOVE_H
#define LEANSEARCH_REMOVE_H

#include "leansearch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* *out_removed (may be NULL): the rows removed. */
int ls_remove(ls_index* index, const uint8_t* bitmap, int64_t nbytes, int64_t* out_removed);

/* Rows subset `subset` of the handle (ls_subset_create) covers now. */
int ls_subset_rows(ls_index* index, int32_t subset, int64_t* out_rows);

/* Test / tuning hook: rows per staging slab of the following ls_remove calls; 0 = automatic (as many stored rows as
 * fit 256 MiB, at most the rows that move). */
int ls_remove_set_slab_rows(ls_index* index, int64_t rows);

/* The most recent ls_remove on this handle (any pointer may be NULL): rows that changed place, staging slabs used,
 * and - with ls_set_profiling on - the time from the first to the last of the row-moving kernels and copies (hipEvents
 * on the handle's stream; they run back to back) and the bytes they read + wrote. Group handles: sums. */
int ls_remove_last(ls_index* index, int64_t* moved_rows, int64_t* slabs, float* move_ms, int64_t* move_bytes);

#ifdef __cplusplus
}
#endif
#endif /* LEANSEARCH_REMOVE_H */
