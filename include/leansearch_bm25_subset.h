/*
 * leansearch_bm25_subset.h — BM25 retrieval over a subset of the documents of one ls_bm25 index.
 *
 * The lexical half of a prefiltered hybrid search: the top-k names among the documents of some packages instead of the
 * global top-k that a post-filter then throws away. Opt-in: ls_bm25_search of leansearch.h is untouched.
 *
 * Definitions
 *   - a subset is a set of documents of one index, given as a bitmap in the layout ls_subset_create takes: document r is
 *     selected iff (bitmap[r >> 3] >> (r & 7)) & 1; bits at r >= n_docs are ignored, documents past a short bitmap are not
 *     selected.
 *   - the result is what the unfiltered search would return if only the selected documents could be candidates. The corpus
 *     statistics stay GLOBAL (idf, length normalisation and non-occurrence shift are the index's stored values), so every
 *     returned score is bit-identical to the score the unfiltered search gives that document: the same float32 additions
 *     in query-token order, then + shift. Order: (score descending, document ascending), ORIGINAL document numbers;
 *     (-FLT_MAX, -1) padding; NaN / <= -FLT_MAX scores are never returned.
 *   - k rule: with m selected documents, min(k, m) > LS_MAX_K is LS_ERR_K_TOO_LARGE. m == 0 returns all padding.
 *   - a subset belongs to its handle: an int32 id, freed by ls_bm25_subset_destroy or with the handle. The index is
 *     immutable, so a subset never goes stale while its handle lives.
 *
 * Conventions are leansearch.h's: LS_OK or a negative LS_ERR_* code, thread-local message in ls_last_error(). Every argument
 * is checked before any device call (NULL handle, unknown id, token id out of range, k <= 0: LS_ERR_INVALID_ARG). Calls on
 * one handle are serialised inside, with ls_bm25_search.
 */
#ifndef LEANSEARCH_BM25_SUBSET_H
#define LEANSEARCH_BM25_SUBSET_H

#include "leansearch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bitmap: host bytes [nbytes] (NULL allowed when nbytes == 0). The bitmap is compacted on the host to an ascending list,
 * uploaded once. out_docs (optional) receives the number of selected documents. */
int ls_bm25_subset_create(ls_bm25* index, const uint8_t* bitmap, int64_t nbytes, int32_t* out_id, int64_t* out_docs);

int ls_bm25_subset_destroy(ls_bm25* index, int32_t id);

/* token_ids host int32 [n_tokens], in query order (duplicates count twice); out_scores host float32 [k]; out_docs host
 * int64 [k]. Synchronous. */
int ls_bm25_search_subset(ls_bm25* index, int32_t subset, const int32_t* token_ids, int32_t n_tokens, int32_t k,
                          float* out_scores, int64_t* out_docs);

#ifdef __cplusplus
}
#endif
#endif /* LEANSEARCH_BM25_SUBSET_H */
