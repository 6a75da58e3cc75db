/*
 * leansearch_subset_batch.h — opt-in: the queries of a subset search share one pass over the selected rows (DESIGN.md
 * section 4.7b).
 *
 * By default ls_search_subset (leansearch.h) serves every query of a call with a scan launch and a selection launch of
 * its own: a call of 16 queries reads the selected rows 16 times. With this option on, groups of 2..16 queries of one
 * call share ONE pass on the f32 matrix cores, followed by one selection launch for the group (17 and more queries:
 * passes of 16; a lone rest is served as before). The scores are the single-query path's, bit for bit: a query's
 * results do not depend on the option or on its company.
 *
 * Served this way: an fp32 index on one device, subsets of at least 4096 selected rows, for k small enough for the
 * per-lane key lists (the rule of the fp32 small-batch kernel). Every other subset call - and every call with the option
 * off - is served exactly as before. ls_search and the IVF calls are not affected.
 */
#ifndef LEANSEARCH_SUBSET_BATCH_H
#define LEANSEARCH_SUBSET_BATCH_H

#include "leansearch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* enable != 0: on. Off by default; enable == 0 is always allowed. LS_ERR_INVALID_ARG for a null handle, and for
 * enable != 0 on an fp16 or sq8 index or on a sharded / replicated handle (their subset searches stay as they are). */
int ls_set_subset_small_batch(ls_index* index, int32_t enable);

#ifdef __cplusplus
}
#endif
#endif /* LEANSEARCH_SUBSET_BATCH_H */
