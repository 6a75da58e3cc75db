/*
 * leansearch_sq8.h — the 8-bit storage dtype of libleansearch.so (LS_DTYPE_SQ8): int8 codes in HBM, exact f32 scan.
 *
 * The shape of faiss's `IndexScalarQuantizer(d, QT_8bit, METRIC_INNER_PRODUCT)`: a quarter of the fp32 index's bytes.
 * It is NOT faiss's QT_8bit (unsigned affine codes, faiss's own decode): the codes are signed and symmetric, defined
 * here, and parity with faiss is unpinned as everywhere else. An sq8 index is an ordinary `ls_index`: every call of
 * leansearch.h works on it (search, device search, subsets, add, reconstruct, set_base); leansearch_ivf.h takes the
 * dtype too.
 *
 * Definitions (tests/sq8_ref.c restates the score)
 *   step    step[i] > 0, float32, one per dimension, fixed for the life of the handle. Given by the caller, or trained
 *           from the rows present at creation: max |x_i| over the finite values of column i, divided by 127.0f
 *           (float32 division); 1.0f where that maximum is 0.
 *   code    c = clamp(rintf(x_i / step_i), -127, 127): correctly rounded float32 division, ties to even. NaN -> 0,
 *           +-inf -> +-127. Rows are 16-byte chunks of 16 codes, zero padded. ls_reconstruct returns (float)c * step_i.
 *   query   q'_i = (q_i * inv) * step_i, two rounded float32 multiplies; inv is the LS_FLAG_NORMALIZE factor or 1.
 *           The query is not quantised.
 *   score   ceil(d / 16) chunks are padded to L * V (ls_sq8_geom). Lane `sub` of the L lanes of a row takes chunks
 *           sub, sub + L, ..; it runs ONE chain acc = fmaf((float)c, q', acc) from 0 over its 16 * V codes in memory
 *           order; the L partial sums are combined by the balanced xor tree (lane ^ 1, ^ 2, ^ 4, ..).
 *   Everything else is leansearch.h's: the total order, the padding, the k rule. By default every query is served alone
 *   by the scan path; with ls_set_sq8_small_batch (leansearch_sq8_batch.h) 2..16 queries share one pass that computes
 *   this score bit for bit. Either way a query's bits depend neither on its company nor on the entry point.
 * ls_create_sharded* and ls_create_replicated refuse LS_DTYPE_SQ8 (every shard would train its own step);
 * ls_set_f16_small_batch refuses it as it refuses fp32.
 */
#ifndef LEANSEARCH_SQ8_H
#define LEANSEARCH_SQ8_H

#include "leansearch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* corpus: host float32 [n, d], d <= 4096. step: host float32 [d], every entry finite and > 0 (else LS_ERR_INVALID_ARG,
 * before any device check), or NULL: trained from the rows. ls_create / ls_create_from_device with LS_DTYPE_SQ8 are this
 * call with a NULL step. */
int ls_create_sq8(ls_index** out, const float* corpus, int64_t n, int32_t d, const float* step_or_null, int32_t device);
int ls_sq8_step(ls_index* index, float* out /* host [d] */);
/* the codes of rows [row0, row0 + count): host int8 [count, d] (the padding is not returned) */
int ls_sq8_codes(ls_index* index, int64_t row0, int64_t count, int8_t* out);
/* the stored row of a d-dimensional sq8 index: chunks = L * V of 16 bytes. No device needed. */
int ls_sq8_geom(int32_t d, int32_t* chunks, int32_t* lanes_per_row, int32_t* chunks_per_lane);

#ifdef __cplusplus
}
#endif
#endif /* LEANSEARCH_SQ8_H */
