/*
 * leansearch_ivf_build.h — building an IVF-flat index on the GPU (libleansearch.so): the two steps of a Lloyd
 * iteration (list of every row, float64 mean of every list), the list assignment of a corpus, and the read-back of a
 * built handle's rows in original order. Opt-in: ls_ivf_create's default assignment and everything else of
 * leansearch_ivf.h are untouched.
 *
 * Definitions
 *   - assignment: the list of row r is what ls_search over a float32 index of the centroids returns for the row with
 *     k = 1, bit for bit: the largest inner product in the scan kernels' summation order, ties to the lowest list; a row
 *     no centroid scores (NaN, or every score <= -FLT_MAX) goes to list 0. This is ls_ivf_create(assign = NULL)'s rule.
 *     nlist < 8192: below that every route of ls_search scores in scan order, so "the k = 1 search" is one set of bits.
 *   - means: of the LAST assignment. A list with rows: the float64 sum of its float32 rows, added one by one in
 *     ascending row order, divided by the row count (as a double). A list without rows: its current centroid as double.
 *   - fp32 rows only; d must have an fp32 row geometry (d <= 1024); n == 0 is legal (assign writes nothing, the counts
 *     are zeros, the means are the centroids).
 * Conventions are leansearch.h's: every argument is checked before any device is touched, LS_ERR_NO_DEVICE without a
 * GPU, the message in ls_last_error(). Calls on one trainer are serialised by its mutex, on its own stream.
 */
#ifndef LEANSEARCH_IVF_BUILD_H
#define LEANSEARCH_IVF_BUILD_H

#include "leansearch_ivf.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ls_ivf_trainer ls_ivf_trainer; /* training rows resident in HBM, one device */

/* rows: host float32 [n, d], uploaded once. 1 <= nlist < 8192. */
int ls_ivf_trainer_create(ls_ivf_trainer** out, const float* rows, int64_t n, int32_t d, int32_t nlist, int32_t device);
/* centroids: host float32 [nlist, d]. out_assign: host int32 [n] or NULL; out_counts: host int64 [nlist] or NULL. */
int ls_ivf_trainer_assign(ls_ivf_trainer* t, const float* centroids, int32_t* out_assign, int64_t* out_counts);
/* out_means: host float64 [nlist, d], of the last ls_ivf_trainer_assign (LS_ERR_INVALID_ARG before any). */
int ls_ivf_trainer_means(ls_ivf_trainer* t, double* out_means);
/* Kernel time (hipEvents on the trainer's stream) of the most recent assignment kernel and the most recent means kernel;
 * 0 for a kernel that has not run (n == 0 launches no assignment kernel). Either pointer may be NULL. */
int ls_ivf_trainer_last_kernel_ms(ls_ivf_trainer* t, float* assign_ms, float* means_ms);
void ls_ivf_trainer_destroy(ls_ivf_trainer* t);

/* Stateless: the list of every row of a host array (out_assign host int32 [n]) - what ls_ivf_create(assign = NULL)
 * computes. The rows are uploaded in steps of 65536 rows (environment LS_IVF_ASSIGN_STEP: another row count), one
 * kernel launch per step. */
int ls_ivf_assign(const float* rows, int64_t n, int32_t d, const float* centroids, int32_t nlist, int32_t* out_assign,
                  int32_t device);

/* Rows [row0, row0 + count) of a built IVF handle in ORIGINAL row order, host float32 [count, d] (fp16 / sq8 storage:
 * the stored values, as ls_reconstruct). */
int ls_ivf_reconstruct(ls_ivf* ivf, int64_t row0, int64_t count, float* out);

#ifdef __cplusplus
}
#endif
#endif /* LEANSEARCH_IVF_BUILD_H */
