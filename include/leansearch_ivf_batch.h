/*
 * leansearch_ivf_batch.h — opt-in: the queries of an IVF search share one pass over the lists they probe (DESIGN.md
 * section 4.8d).
 *
 * By default ls_ivf_search (leansearch_ivf.h) serves every query of a call with a chain of its own - centroid search,
 * probed-list scan, selection - and reads every probed row once per query that probes it. With this option on, groups of
 * 2..16 queries of one call share ONE centroid search, ONE pass on the f32 matrix cores over the union of the lists the
 * group probes, and one selection launch (17 and more queries: groups of 16; a lone rest is served as before). Nothing
 * about the result changes: probe lists, scores, order and padding are leansearch_ivf.h's, bit for bit - a query's
 * result does not depend on the option or on its company.
 *
 * Served this way: fp32 rows, calls without a subset, at most 4096 lists, groups whose row bound (the rows of the
 * handle's nprobe largest lists, times the group, at most the index) reaches 4096, for k small enough for the per-lane
 * key lists (the rule of the fp32 small-batch kernel). Every other call - ls_ivf_search_subset always, and every call
 * with the option off - is served exactly as before.
 */
#ifndef LEANSEARCH_IVF_BATCH_H
#define LEANSEARCH_IVF_BATCH_H

#include "leansearch_ivf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* enable != 0: on. Off by default; enable == 0 is always allowed. LS_ERR_INVALID_ARG for a null handle, and for
 * enable != 0 on a handle of fp16 or sq8 rows (refused before any device call). Switching it on sizes the handle's
 * scratch for 16 queries; nothing is allocated by a search afterwards that the option-off search would not allocate. */
int ls_ivf_set_small_batch(ls_ivf* ivf, int32_t enable);

/* The most recent ls_ivf_search / ls_ivf_search_subset of the handle: passes = union passes it launched (one per group
 * of 2..16 queries served this way; 0 with the option off), union_rows = the sum of their union sizes (rows read by the
 * passes). Either pointer may be NULL. */
int ls_ivf_last_passes(ls_ivf* ivf, int32_t* passes, int64_t* union_rows);

#ifdef __cplusplus
}
#endif
#endif /* LEANSEARCH_IVF_BATCH_H */
