/*
 * leansearch_sq8_batch.h — opt-in: small batches on an sq8 index share one pass over the codes.
 *
 * By default an sq8 index (leansearch_sq8.h) serves every query with a scan launch of its own. With this option on,
 * 2..16 queries that reach the scan path together - an explicit batch, concurrent ls_search callers combined into one
 * call, a pipelined device call - share ONE pass on the f32 matrix cores (17..32 queries: two passes). The score is
 * the one leansearch_sq8.h defines, bit for bit: a query's results do not depend on the option, on its company or on
 * the entry point. A lone query, every retry and every repair stay on the scan kernel.
 *
 * Served this way: rows of at most 64 chunks (d <= 1024) on a handle of at least 4096 rows, for k small enough for the
 * per-lane key lists (the rule of the fp32 small-batch kernel). Every other call is served exactly as with the option
 * off. ls_search_subset and the IVF calls are not affected.
 */
#ifndef LEANSEARCH_SQ8_BATCH_H
#define LEANSEARCH_SQ8_BATCH_H

#include "leansearch_sq8.h"

#ifdef __cplusplus
extern "C" {
#endif

/* enable != 0: on. Off by default. LS_ERR_INVALID_ARG for a null handle and for a handle that is not an sq8 index.
 * Waits for the handle's queued work, which finishes under the old setting. */
int ls_set_sq8_small_batch(ls_index* index, int32_t enable);

#ifdef __cplusplus
}
#endif
#endif /* LEANSEARCH_SQ8_BATCH_H */
