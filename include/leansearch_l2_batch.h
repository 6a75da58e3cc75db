/*
 * leansearch_l2_batch.h — opt-in: 2..8 queries on an L2 index share one pass over the corpus.
 *
 * By default an L2 index (leansearch_l2.h) serves every query with a scan launch of its own. With this option on, the
 * queries that reach the scan path together - an explicit batch of ls_search, concurrent ls_search callers combined into
 * one call - go out in groups of 8, 4 or 1 (5 or more left: 8; 2 to 4 left: 4; the last real query repeated as padding),
 * and a group shares ONE pass of the scan kernel on the vector ALU. The distance is the one leansearch_l2.h defines, bit
 * for bit: a query's results depend neither on the option, nor on its company, nor on its place in a group. A lone
 * query and every retry stay on the single-query L2 scan.
 *
 * Served in groups of 4 / 1 only: fp16 rows of 17..32 chunks (129 <= d <= 256), whose 8-query kernel is not
 * built, and fp16 rows of 4-chunk lanes (49..64, 97..128, 193..256 chunks), where two launches of 4 measured faster than one
 * of 8. The results are the same bits either way.
 *
 * Not affected: ls_search_subset, ls_range_search(_subset), ls_add, ls_remove, every IVF handle. ls_search_device stays
 * refused on an L2 handle.
 */
#ifndef LEANSEARCH_L2_BATCH_H
#define LEANSEARCH_L2_BATCH_H

#include "leansearch_l2.h"

#ifdef __cplusplus
extern "C" {
#endif

/* enable != 0: on. Off by default. LS_ERR_INVALID_ARG (before any device check) for a null handle, for a handle whose
 * ls_metric is not LS_METRIC_L2 and for a sharded or replicated handle. Waits for the handle's queued work, which
 * finishes under the old setting. */
int ls_set_l2_small_batch(ls_index* index, int32_t enable);
/* 1 if the option is on, else 0 (a null handle, any other handle: 0) */
int32_t ls_l2_small_batch(const ls_index* index);

#ifdef __cplusplus
}
#endif
#endif /* LEANSEARCH_L2_BATCH_H */
