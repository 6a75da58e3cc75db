// ls_ivf_state.h — private: the IVF handle and its subsets, shared by ls_ivf.hip (which creates, searches and frees
// them) and ls_ivf_mutate.hip (which changes the rows of a built handle).
#pragma once
#include "ls_index.h"
#include "ls_ivf_build_plan.h"

#include "../../include/leansearch_ivf_l2.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <vector>

struct ls_ivf_subset {
    int64_t m = 0;                  // selected rows
    u32* d_soff = nullptr;          // [nlist + 1] offsets of the lists in the two arrays below
    u32* d_srow = nullptr;          // [m] storage row of every selected row, list after list
    u32* d_sid = nullptr;           // [m] original row of every selected row
    std::vector<int64_t> sizes;     // [nlist] selected rows per list
    std::vector<int64_t> top_rows;  // [nlist + 1]: selected rows of the p fullest lists (the bound of a query's M)
};

static inline void ivf_subset_free(ls_ivf_subset* ss) {  // (the handle's device is current)
    if (!ss) return;
    for (void* p : {(void*)ss->d_soff, (void*)ss->d_srow, (void*)ss->d_sid}) (void)hipFree(p);
    delete ss;
}

struct ls_ivf {
    mutable std::mutex mu;  // calls on one handle are serialised (ls_ivf_add changes n and the host tables under it)
    int32_t device = 0, d = 0, dtype = 0, nlist = 0;
    int32_t metric = 0;  // LS_METRIC_* (include/leansearch_ivf_l2.h), fixed at creation: 1 = `cent` is an ls_create_l2 handle,
                         // every fine score is a negated squared distance, results leave as distances (ls_l2_out)
    int64_t n = 0;
    ls_index* cent = nullptr;  // fp32 index of the centroids
    ls_index* rows = nullptr;  // the corpus, list after list
    u32* d_ids = nullptr;      // [n] storage row -> original row
    u32* d_off = nullptr;      // [nlist + 1]
    std::vector<int64_t> sizes;     // [nlist]
    std::vector<int64_t> top_rows;  // [nlist + 1]: rows of the p largest lists (the host's bound of a query's M)
    std::vector<int32_t> assign;    // [n]
    std::vector<u32> off;           // [nlist + 1] host copy of d_off
    std::map<int32_t, ls_ivf_subset*> subsets;
    int32_t next_subset = 1;
    hipStream_t stream = nullptr;
    float* h_q = nullptr;      size_t hq_cap = 0;  // pinned
    float* h_s = nullptr;      size_t hs_cap = 0;  // pinned: the selection writes the results here
    int64_t* h_i = nullptr;    size_t hi_cap = 0;  // pinned
    u32* h_any = nullptr;      // pinned word: some query of the call raised its flag
    float* d_q = nullptr;      size_t q_cap = 0;
    float* d_ps = nullptr;     size_t ps_cap = 0;   // coarse results [nq, nprobe]: scores ...
    int64_t* d_pi = nullptr;   size_t pi_cap = 0;   // ... and list numbers: the probe lists
    u32* d_flags = nullptr;    size_t flags_cap = 0;  // [nq] raised by a selection that could not prove its keys
    bool flags_clean = false;  // every word of d_flags is zero (no reset command on the usual call's path)
    std::vector<u32> h_flags;
    u64* d_cand = nullptr;     // [max_blocks * LS_KP_MAX]
    u64* d_bound = nullptr;    // [max_blocks]
    int32_t max_blocks = 0;
    u32* d_counters = nullptr;
    float* d_S = nullptr;      // [n] original-row-indexed scores of the second launch (allocated at first need)
    // range search (ls_ivf_range_search): its own block of rs_vecs <= LS_RANGE_GROUP original-row-indexed score vectors,
    // rs_stride floats apart (allocated at first need, dropped with d_S when n changes), and the collect step's scratch
    float* d_RS = nullptr;
    int rs_vecs = 0;
    long long rs_stride = 0;
    ls_range_scratch* range = nullptr;
    bool profiling = false;
    std::vector<hipEvent_t> ev;  // 3 per query: begin, coarse done, fine done
    int prof_n = 0, last_rescued = 0;
    // ls_ivf_set_small_batch (ls_ivf_batch.hip): groups of 2..16 queries share a pass over the union of their lists
    bool small_batch = false;
    int cand_queries = 1;      // queries d_cand / d_bound have room for (16 once the option was switched on)
    ls_ivf_union un{};         // the union step's arrays (allocated when the option is first switched on)
    u32* h_m = nullptr;        size_t hm_cap = 0;  // pinned: the union size of every pass of the last call
    int last_passes = 0;
    int64_t last_union_rows = 0;
    // ls_ivf_add / ls_ivf_remove (with profiling on): events around the row mover's launch, and what the last call of
    // each kind took and moved
    hipEvent_t move_ev[2] = {nullptr, nullptr};
    float add_ms = 0.0f, rm_ms = 0.0f;
    int64_t add_bytes = 0, rm_bytes = 0;
    int64_t bf16_inexact = 0;  // LS_DTYPE_BF16: elements stored inexactly, over every row handed to create or add (ls_ivf_bf16_inexact)
};

// assign = NULL: the library's own exact search over the centroids, k = 1: the largest inner product - on an L2 handle
// the smallest distance -, ties to the lowest list number, a row no centroid scores to list 0 (ls_ivf_create and
// ls_ivf_add). On an L2 centroid index the search is one launch per row, so an L2 handle takes the L2 assignment kernel
// (ls_ivf_assign_l2: one launch per upload step, the same bits) where that kernel's shape limits hold; the environment
// LS_IVF_L2_ASSIGN=search keeps the per-row search (the timing of DESIGN.md 4.12).
static inline int ivf_default_assign(ls_index* cent, int32_t metric, int32_t nlist, int32_t device, const float* rows,
                                     int64_t n, int32_t d, int32_t* out) {
    if (metric == LS_METRIC_L2 && n > 0 && nlist <= LS_IVFB_MAX_NLIST && n < 0x7fffffffll) {
        const char* e = getenv("LS_IVF_L2_ASSIGN");
        if (!e || strcmp(e, "search") != 0) {
            std::vector<float> c((size_t)nlist * d);
            if (int rc = ls_reconstruct(cent, 0, nlist, c.data())) return rc;  // (f32 rows: the centroids themselves)
            return ls_ivf_assign_l2(rows, n, d, c.data(), nlist, out, device);
        }
    }
    const int64_t step = 1 << 16;
    std::vector<float> s((size_t)std::min(step, std::max<int64_t>(n, 1)));
    std::vector<int64_t> i(s.size());
    for (int64_t r0 = 0; r0 < n; r0 += step) {
        const int64_t m = std::min(step, n - r0);
        if (int rc = ls_search(cent, rows + r0 * d, m, 1, 0, s.data(), i.data())) return rc;
        for (int64_t j = 0; j < m; ++j) out[r0 + j] = i[(size_t)j] >= 0 ? (int32_t)i[(size_t)j] : 0;
    }
    return LS_OK;
}

// sizes -> top_rows[p]: the rows of the p largest lists
static inline void ivf_top_rows(const std::vector<int64_t>& sizes, std::vector<int64_t>& top_rows) {
    std::vector<int64_t> sorted(sizes);
    std::sort(sorted.begin(), sorted.end(), std::greater<int64_t>());
    top_rows.assign(sizes.size() + 1, 0);
    for (size_t p = 0; p < sizes.size(); ++p) top_rows[p + 1] = top_rows[p] + sorted[p];
}
