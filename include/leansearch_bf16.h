/*
 * leansearch_bf16.h — the bfloat16 storage dtype of libleansearch.so (LS_DTYPE_BF16 = 3): bf16 rows in HBM, exact f32 scan.
 *
 * The half-size index that is LOSSLESS for an embedder that emits bfloat16: bf16 -> f32 is a 16-bit shift, so a stored
 * element converts exactly, and the query stays float32. (LS_DTYPE_F16 re-rounds bf16 values - range and subnormals
 * differ - and rounds the query to fp16 as well.)
 *
 * Definition
 *   storage    the fp16 index's layout: a row is `chunks` 16-byte chunks of 8 elements, zero padded; the eight
 *              geometries of 2-byte rows (16/32/48/64/96/128/192/256 chunks), d <= 2048. Element 2 * i of a chunk is
 *              the low half of its 32-bit word i.
 *   encoding   of a float32 with bit pattern u, round to nearest even:
 *                NaN             (u >> 16) | 0x0040
 *                anything else   (u + 0x7fff + ((u >> 16) & 1)) >> 16
 *              so finite values above the largest bf16 become +-inf; subnormals and -0 are kept.
 *   decoding   bits << 16, exact.
 *   score      the query is prepared exactly as for an fp32 index (LS_FLAG_NORMALIZE: the library's one summation order,
 *              one rounded multiply per element). With L lanes per row and V chunks per lane, lane `sub` runs ONE chain
 *              from 0 over its chunks sub, sub + L, ... and their elements in memory order,
 *              acc = fmaf((float)x, q, acc); the L partial sums are combined by the balanced xor tree every dtype uses.
 *              tests/bf16_ref.c restates it in plain C; the GPU's scores equal it bit for bit.
 *   ranking    order, ties by row, the (-FLT_MAX, -1) padding and the NaN rule are the shared selection step's.
 *
 * Inner product only, one device only: ls_create_l2, ls_create_l2_from_device and ls_ivf_create_l2 refuse LS_DTYPE_BF16,
 * and so do ls_create_sharded, ls_create_sharded_from_device and ls_create_replicated - all LS_ERR_INVALID_ARG with a
 * message that names bf16, before any device check.
 *
 * ls_create, ls_create_from_device and ls_ivf_create accept LS_DTYPE_BF16 (rows handed in as float32, encoded on the
 * device); there is no create entry of its own. An IVF handle keeps f32 centroids, and its coarse stage, ls_ivf_assign
 * and the trainer see the f32 rows as given.
 *
 * What a bf16 handle answers elsewhere - in every case what an sq8 handle answers (the two are served alike):
 *   ls_search, ls_search_subset, ls_range_search(_subset)    every query of a call goes out alone on the scan kernel
 *                                                            (concurrent callers gathered into one call as well); a
 *                                                            query's bits do not depend on its company.
 *   ls_search_device (sync, LS_FLAG_ASYNC, LS_FLAG_PIPELINE,  accepted; one scan launch per query, never a small-batch
 *     LS_FLAG_INORDER), ls_check, ls_export_flags             pass or the batched matrix-core path, whatever nq is;
 *                                                            ls_export_flags exports zeros.
 *   ls_add, ls_remove, ls_ivf_add, ls_ivf_remove             new rows are encoded as at create; stored rows move as bytes.
 *   ls_reconstruct, ls_ivf_reconstruct                       the decoded rows (exactly the stored values).
 *   ls_set_f16_small_batch, ls_set_sq8_small_batch           refused (on and off) with words that say "bf16 rows".
 *   ls_set_subset_small_batch(1), ls_ivf_set_small_batch(1)  refused likewise; switching them off is LS_OK.
 *   ls_set_l2_small_batch                                    refused: not an L2 index.
 *   ls_sq8_step, ls_sq8_codes                                refused: not an sq8 index.
 */
#ifndef LEANSEARCH_BF16_H
#define LEANSEARCH_BF16_H

#include "leansearch.h"
#include "leansearch_ivf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The stored bits of rows [row0, row0 + count) as uint16 [count, d] in host memory. A single-device bf16 index only. */
int ls_bf16_rows(ls_index* index, int64_t row0, int64_t count, uint16_t* out);

/* Elements whose stored value differs from the float32 handed in (NaN never counts), summed over every row ever handed
 * to create or add on this handle; removal does not lower it. 0: the index holds exactly what it was given. */
int ls_bf16_inexact(ls_index* index, int64_t* out);
int ls_ivf_bf16_inexact(ls_ivf* index, int64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* LEANSEARCH_BF16_H */
