// ls_ivf.hip — IVF-flat search (include/leansearch_ivf.h): probe `nprobe` inverted lists, scan only their rows.
//
// The handle owns two plain single-device indexes: `cent`, an fp32 index of the nlist centroids (the coarse quantiser),
// and `rows`, the corpus stored LIST AFTER LIST in the standard padded row layout (within a list ascending by original
// row), plus ids[n] (storage row -> original row) and off[nlist + 1] (first storage row of every list).
//
// A search is two stages on the handle's stream and nothing returns to the host in between:
//   coarse  the exact scan-path search of `cent` with k = nprobe (ls_search_device, LS_FLAG_ASYNC: exact in stream
//           order); its result rows stay in HBM: they ARE the probe list.
//   fine    ls_ivf_scan_kernel. Every workgroup reads the probe list, builds the prefix sums of the probed lists' sizes
//           in LDS (M = rows probed; the host only knows an upper bound, the sum of the nprobe largest lists, and plans
//           workgroups and k' from it) and the waves take tiles of TR positions of [0, M) round-robin, exactly as the
//           plain scan takes tiles of rows. Position -> (probed list, storage row) is ONE search in the prefix per
//           tile - lane i looks position i of the tile up - a tile ahead of the row loads, which fetch the storage
//           rows from the looking lanes. The dot products are ls_scan_dev.h's (the scan kernel's own dot / group_sum
//           of the same F16, L, V), so every score is bit-identical to the flat scan's of that row. Keys carry the
//           ORIGINAL row (ord(score) << 32 | ~ids[storage row]): selection, bounds and finalize_body work in original
//           rows and ties come out row-ascending without a post-pass. Workgroups without tiles emit empty candidates.
//   select  the stand-alone ls_finalize_kernel over the emitted keys, without a score vector: a query whose keys
//           cannot be proven complete raises a flag word and is served again after the call's one wait by the
//           always-exact second launch: the same fine kernel also scatters its scores into an ORIGINAL-row-indexed
//           vector (reset to NaN = "not probed"), and finalize_body's rescue / general selection runs over that
//           vector. Same bits either way.
//
// Small batches (include/leansearch_ivf_batch.h, opt-in, fp32 rows, no subset): where the plan of ls_mq_plan.h
// (LS_MQ_IVF) serves the (handle, k, nprobe), a call's queries are taken in groups of min(left, 16) while two or more
// are left, and a group runs ONE coarse search (its probe lists land in d_pi as above), the union step and ONE pass
// over the union of the group's lists on the f32 matrix cores (ls_ivf_batch.hip: the same bits), and ONE selection
// launch with the group's jobs - each the first launch's job above, so a flagged query is served again by the same
// second launch. A lone rest, and every call where the plan declines or the option is off, takes the chains above.
//
// An IVF subset (include/leansearch_ivf_subset.h) is the same search through the row-list form of the fine kernel
// (ls_ivf_subset.hip): the selection is compacted once, on the host (ls_ivf_subset_plan.h), into soff / srow / sid; a
// search plans its workgroups and k' from the subset's own top_rows (never more than the handle's, so the scratch
// sized at create holds) and hands the kernel soff for off, sid for ids and srow as the list. Coarse stage, flag
// words, the one wait, the second launch over the ORIGINAL-row-indexed vector and the events are shared.
//
// An L2 handle (include/leansearch_ivf_l2.h, ls_ivf::metric) is the same search with `cent` an ls_create_l2 index - probed
// through ls_i_search_device, since the public ls_search_device refuses L2 indexes - and the fine kernel's L2
// instantiations (ls_l2_ivf.hip): every score is -distance, so keys, selection, the second launch and the range collect
// step work unchanged, and the results become distances where they are copied out (ls_l2_out). No small batches.
//
// Rows join and leave a built handle in ls_ivf_mutate.hip (ls_ivf_add, ls_ivf_remove); the handle itself is
// ls_ivf_state.h's. This file keeps create, search, the subsets, reconstruct and the options.
#include "ls_scan_launch.h"
#include "ls_ivf_state.h"
#include "ls_ivf_subset_plan.h"
#include "ls_range_plan.h"
#include "ls_switch_plan.h"

#include "../../include/leansearch_range.h"
#include "../../include/leansearch_ivf_batch.h"
#include "../../include/leansearch_ivf_build.h"
#include "../../include/leansearch_ivf_subset.h"

#include <algorithm>
#include <map>
#include <mutex>
#include <numeric>
#include <vector>

#define LS_IVF_PROF_MAX 64


template <bool F16>
static int ivf_launch_dt(const ls_geom& g, const ivf_launch& a, hipStream_t s) {
    return ls_geom_dispatch<false, true>("ls_ivf_search", g, [&](auto L, auto V) -> int {
        return ls_ivf_scan_launch<F16, L(), V()>(g, a, s);
    });
}

static int ivf_launch_scan(const ls_geom& g, const ivf_launch& a, hipStream_t s) {
    if (a.nprobe < 1 || a.nprobe > LS_IVF_MAX_PROBE || a.kprime < 1 || a.kprime + 1 > LS_KP_MAX || a.blocks < 1) {
        ls_set_error("ls_ivf_search: launch plan out of range (nprobe %d kprime %d blocks %d)", a.nprobe, a.kprime,
                     a.blocks);
        return LS_ERR_INVALID_ARG;
    }
    if (a.l2) return ls_ivf_launch_scan_l2(g, a, s);  // (plain and row-list form: ls_l2_ivf.hip)
    if (g.bf16) return ls_ivf_launch_scan_bf16(g, a, s);  // (plain and row-list form: ls_bf16_ivf.hip)
    if (a.srow) return ls_ivf_launch_scan_subset(g, a, s);
    if (g.elem == 1) return ls_ivf_launch_scan_sq8(g, a, s);
    return g.elem == 2 ? ivf_launch_dt<true>(g, a, s) : ivf_launch_dt<false>(g, a, s);
}

// ---- the handle ---------------------------------------------------------------------------------------------------
static void ivf_free(ls_ivf* v) {
    if (!v) return;
    ls_device_guard guard;
    (void)hipSetDevice(v->device);
    if (v->stream) (void)hipStreamSynchronize(v->stream);
    if (v->cent) ls_destroy(v->cent);
    if (v->rows) ls_destroy(v->rows);
    (void)hipSetDevice(v->device);
    for (auto& kv : v->subsets) ivf_subset_free(kv.second);
    for (void* p : {(void*)v->d_ids, (void*)v->d_off, (void*)v->d_q, (void*)v->d_ps, (void*)v->d_pi, (void*)v->d_flags,
                    (void*)v->d_cand, (void*)v->d_bound, (void*)v->d_counters, (void*)v->d_S, (void*)v->d_RS, (void*)v->un.lmask,
                    (void*)v->un.lpre, (void*)v->un.row, (void*)v->un.id, (void*)v->un.mask, (void*)v->un.m})
        (void)hipFree(p);
    ls_i_range_scratch_free(v->range);
    for (void* p : {(void*)v->h_q, (void*)v->h_s, (void*)v->h_i, (void*)v->h_any, (void*)v->h_m})
        if (p) (void)hipHostFree(p);
    for (hipEvent_t e : v->ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : v->move_ev)
        if (e) (void)hipEventDestroy(e);
    if (v->stream) (void)hipStreamDestroy(v->stream);
    delete v;
}

static int ivf_build(ls_ivf* v, const float* corpus, const float* centroids, const int32_t* assign) {
    const int64_t n = v->n;
    const int32_t d = v->d, nlist = v->nlist;
    if (int rc = v->metric == LS_METRIC_L2 ? ls_create_l2(&v->cent, centroids, nlist, d, LS_DTYPE_F32, v->device)
                                           : ls_create(&v->cent, centroids, nlist, d, LS_DTYPE_F32, v->device))
        return rc;
    v->assign.resize((size_t)n);
    if (assign) {
        for (int64_t r = 0; r < n; ++r) {
            if (assign[r] < 0 || assign[r] >= nlist) {
                ls_set_error("ls_ivf_create: assign[%lld] = %d is not a list (nlist %d)", (long long)r, assign[r], nlist);
                return LS_ERR_INVALID_ARG;
            }
            v->assign[(size_t)r] = assign[r];
        }
    } else if (int rc = ivf_default_assign(v->cent, v->metric, nlist, v->device, corpus, n, d, v->assign.data())) {
        return rc;
    }
    // counting sort by list: storage order = list after list, ascending original row inside a list
    v->sizes.assign((size_t)nlist, 0);
    for (int64_t r = 0; r < n; ++r) v->sizes[(size_t)v->assign[(size_t)r]]++;
    std::vector<u32> off((size_t)nlist + 1, 0);
    for (int32_t l = 0; l < nlist; ++l) off[(size_t)l + 1] = off[(size_t)l] + (u32)v->sizes[(size_t)l];
    std::vector<u32> ids((size_t)n);
    {
        std::vector<u32> at(off.begin(), off.end() - 1);
        for (int64_t r = 0; r < n; ++r) ids[at[(size_t)v->assign[(size_t)r]]++] = (u32)r;
    }
    ivf_top_rows(v->sizes, v->top_rows);
    {
        std::vector<float> perm((size_t)n * d);
        for (int64_t sr = 0; sr < n; ++sr)
            std::copy(corpus + (int64_t)ids[(size_t)sr] * d, corpus + ((int64_t)ids[(size_t)sr] + 1) * d,
                      perm.begin() + sr * d);
        if (int rc = ls_create(&v->rows, perm.data(), n, d, v->dtype, v->device)) return rc;
        if (v->dtype == LS_DTYPE_BF16)
            if (int rc = ls_i_bf16_inexact(v->rows, &v->bf16_inexact)) return rc;
    }
    LS_HIP(hipSetDevice(v->device));
    LS_HIP(hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking));
    LS_HIP(hipMalloc((void**)&v->d_ids, sizeof(u32) * (size_t)std::max<int64_t>(n, 1)));
    LS_HIP(hipMalloc((void**)&v->d_off, sizeof(u32) * ((size_t)nlist + 1)));
    if (n > 0) LS_HIP(hipMemcpy(v->d_ids, ids.data(), sizeof(u32) * (size_t)n, hipMemcpyHostToDevice));
    LS_HIP(hipMemcpy(v->d_off, off.data(), sizeof(u32) * ((size_t)nlist + 1), hipMemcpyHostToDevice));
    v->off = std::move(off);
    v->max_blocks = 2 * v->rows->n_cu;  // ls_scan_blocks() <= 2 workgroups per CU
    LS_HIP(hipMalloc((void**)&v->d_cand, sizeof(u64) * (size_t)v->max_blocks * LS_KP_MAX));
    LS_HIP(hipMalloc((void**)&v->d_bound, sizeof(u64) * (size_t)v->max_blocks));
    LS_HIP(hipMalloc((void**)&v->d_counters, sizeof(u32) * 16));
    LS_HIP(hipMemset(v->d_counters, 0, sizeof(u32) * 16));
    LS_HIP(hipHostMalloc((void**)&v->h_any, sizeof(u32), hipHostMallocDefault));
    *v->h_any = 0;
    return LS_OK;
}

// the fine launch of query qi of the call (its probe list in d_pi, its raw query in d_q), planned for kf ranks over at
// most rows_bound probed rows; S: the original-row-indexed vector it also scatters its scores into, or nullptr
static ivf_launch ivf_fine_args(const ls_ivf* v, const ls_ivf_subset* ss, int64_t qi, int32_t kf, int np, bool normalize,
                                int64_t rows_bound, float* S) {
    const ls_geom& g = v->rows->g;
    const int blocks = std::min(ls_scan_blocks(rows_bound, g, v->rows->n_cu), v->max_blocks);
    const int kprime = ls_kprime(blocks, (int)std::max<int64_t>(std::min<int64_t>(kf, rows_bound), 1), LS_KP_MAX);
    ivf_launch a{};
    a.corpus = v->rows->d_corpus;
    a.ids = ss ? ss->d_sid : v->d_ids;
    a.off = ss ? ss->d_soff : v->d_off;
    a.srow = ss ? ss->d_srow : nullptr;
    a.probe = (const long long*)(v->d_pi + qi * np);
    a.nprobe = np;
    a.q = v->d_q + qi * v->d;
    a.normalize = normalize;
    a.S = S;
    a.cand = v->d_cand;
    a.bound = v->d_bound;
    a.blocks = blocks;
    a.kprime = kprime;
    a.step = v->rows->d_sq8_step;
    a.l2 = v->metric == LS_METRIC_L2;
    return a;
}

// one query's fine launch + selection on the handle's stream. S == nullptr: first launch (a query that cannot be
// proven raises d_flags[qi]); else the always-exact second launch over the original-row-indexed vector S.
// ss: the subset to search, or nullptr. k: the slots a query owns in the output; kf <= k: the ranks to fill (a subset
// of m rows asks for min(k, m), so that the second launch - whose n is ntotal - never selects more than LS_MAX_K).
static int ivf_fine(ls_ivf* v, const ls_ivf_subset* ss, int64_t qi, int32_t k, int32_t kf, int np, bool normalize,
                    int64_t rows_bound, float* S) {
    const ivf_launch a = ivf_fine_args(v, ss, qi, kf, np, normalize, rows_bound, S);
    const int blocks = a.blocks, kprime = a.kprime;
    if (int rc = ivf_launch_scan(v->rows->g, a, v->stream)) return rc;
    ls_fin_batch jobs{};
    ls_fin_params& p = jobs.p0;
    p.S = S;
    p.n = S ? v->n : rows_bound;  // (first launch: keys only - n bounds k, nothing is read by row)
    p.cand = v->d_cand;
    p.bound = v->d_bound;
    p.blocks = blocks;
    p.kprime = kprime;
    p.k = kf;
    p.keys_cap = LS_FINAL_CAP;
    p.force_slow = 0;
    p.base = 0;
    p.out_scores = v->h_s + qi * k;
    p.out_indices = (long long*)(v->h_i + qi * k);
    p.counters = v->d_counters;
    p.repair = S ? nullptr : v->d_flags + qi;
    p.repair_any = S ? nullptr : v->h_any;
    jobs.njobs = 1;
    return ls_launch_finalize(jobs, v->stream);
}

// the handle as ls_mq_plan.h's input (LS_MQ_IVF)
static ls_mq_in ivf_mq_in(const ls_ivf* v) {
    ls_mq_in in{};
    in.kind = LS_MQ_IVF;
    in.opt_in = v->small_batch && v->metric != LS_METRIC_L2;  // (an L2 handle never has it on: every query is served alone)
    in.multi_query = in.mq = in.single_device = true;
    in.f32 = v->dtype == LS_DTYPE_F32;
    in.n_cu = v->rows->n_cu;
    in.max_blocks = v->max_blocks;
    in.chunks = v->rows->g.chunks;
    in.nlist = v->nlist;
    return in;
}

// queries [i0, i0 + g) of the call, their probe lists in d_pi: the union step, ONE pass over the union, ONE selection
// launch with the group's jobs (each as ivf_fine's first launch: keys only, a query that cannot be proven raises
// d_flags[i] and is served again by the second launch). rows_q: the rows one query probes at most.
static int ivf_group_pass(ls_ivf* v, int64_t i0, int g, int32_t k, int np, bool normalize, int64_t rows_q,
                          const ls_mq_plan& mp, u32* h_m) {
    if (g > v->cand_queries) {
        ls_set_error("ls_ivf_search: a group of %d queries, candidate blocks for %d", g, v->cand_queries);
        return LS_ERR_INVALID_ARG;
    }
    const ls_geom& geo = v->rows->g;
    ls_scan_args a{};
    a.d_q = v->d_q + i0 * v->d;
    a.nq = g;
    a.normalize = normalize;
    a.d_cand = v->d_cand;
    a.c_stride = (long long)v->max_blocks * LS_KP_MAX;
    a.d_bound = v->d_bound;
    a.b_stride = v->max_blocks;
    a.blocks = mp.blocks;
    a.kprime = mp.kprime;
    a.mq_keys = mp.keys;
    if (int rc = ls_ivf_launch_union((const long long*)(v->d_pi + i0 * np), g, np, v->d_off, v->d_ids, v->nlist, v->un, h_m,
                                     v->stream))
        return rc;
    if (int rc = ls_launch_mq_ivf_union(v->rows->d_corpus, v->un, ls_mq_ivf_bound(v->n, rows_q, g), geo, a, v->stream))
        return rc;
    ls_fin_batch jobs{};
    ls_fin_params& p = jobs.p0;
    p.S = nullptr;
    p.n = rows_q;  // (keys only - n bounds k, nothing is read by row)
    p.cand = v->d_cand;
    p.bound = v->d_bound;
    p.blocks = mp.blocks;
    p.kprime = mp.kprime;
    p.k = k;
    p.keys_cap = LS_FINAL_CAP;
    p.force_slow = 0;
    p.base = 0;
    p.out_scores = v->h_s + i0 * k;
    p.out_indices = (long long*)(v->h_i + i0 * k);
    p.counters = v->d_counters;
    p.repair = v->d_flags + i0;
    p.repair_any = v->h_any;
    jobs.cand_stride = a.c_stride;
    jobs.bound_stride = a.b_stride;
    jobs.njobs = g;
    for (int j = 0; j < LS_QUERIES_PER_LAUNCH_MAX; ++j) jobs.idx[j] = (unsigned char)j;
    return ls_launch_finalize(jobs, v->stream);
}

// the coarse search of queries [i, i + nq) of the call: their probe lists land in d_pi. On an L2 handle `cent` is an
// ls_create_l2 index, which the public ls_search_device refuses: the stream-ordered search behind it is reached directly
// (one scan launch per query; the -distance values in d_ps are read by nobody).
static int ivf_coarse(ls_ivf* v, int64_t i, int64_t nq, int np, uint32_t cflags, hipStream_t s) {
    if (v->metric == LS_METRIC_L2)
        return ls_i_search_device(v->cent, v->d_q + i * v->d, nq, np, cflags, v->d_ps + i * np, v->d_pi + i * np, s);
    return ls_search_device(v->cent, v->d_q + i * v->d, nq, np, cflags, v->d_ps + i * np, v->d_pi + i * np, s);
}

static int ivf_search_locked(ls_ivf* v, const ls_ivf_subset* ss, const float* q, int64_t nq, int32_t k, int np,
                             bool normalize, float* out_s, int64_t* out_i) {
    const size_t on = (size_t)nq * k, qn = (size_t)nq * v->d;
    const int64_t rows_bound = ss ? ss->top_rows[(size_t)np] : v->top_rows[(size_t)np];
    const int32_t kf = ss ? (int32_t)std::min<int64_t>(k, std::max<int64_t>(ss->m, 1)) : k;
    v->prof_n = 0;
    v->last_rescued = 0;
    v->last_passes = 0;
    v->last_union_rows = 0;
    const bool l2 = v->metric == LS_METRIC_L2;  // (every score handed back below leaves as a distance, ls_l2_out)
    const float pad = l2 ? FLT_MAX : -FLT_MAX;
    if (rows_bound == 0) {  // no row can be probed (n == 0, or only empty lists can be)
        std::fill(out_s, out_s + on, pad);
        std::fill(out_i, out_i + on, (int64_t)-1);
        return LS_OK;
    }
    LS_HIP(hipSetDevice(v->device));
    hipStream_t s = v->stream;
    if (int r = ls_grow_pinned(&v->h_q, &v->hq_cap, qn)) return r;
    if (int r = ls_grow_pinned(&v->h_s, &v->hs_cap, on)) return r;
    if (int r = ls_grow_pinned(&v->h_i, &v->hi_cap, on)) return r;
    if (int r = ls_grow(&v->d_q, &v->q_cap, qn)) return r;
    if (int r = ls_grow(&v->d_ps, &v->ps_cap, (size_t)nq * np)) return r;
    if (int r = ls_grow(&v->d_pi, &v->pi_cap, (size_t)nq * np)) return r;
    {
        const size_t had = v->flags_cap;
        if (int r = ls_grow(&v->d_flags, &v->flags_cap, (size_t)nq)) return r;
        if (v->flags_cap != had) v->flags_clean = false;
    }
    std::copy(q, q + qn, v->h_q);
    *v->h_any = 0;
    LS_HIP(hipMemcpyAsync(v->d_q, v->h_q, sizeof(float) * qn, hipMemcpyHostToDevice, s));
    if (!v->flags_clean) {
        LS_HIP(hipMemsetAsync(v->d_flags, 0, sizeof(u32) * v->flags_cap, s));
        v->flags_clean = true;
    }
    const uint32_t cflags = (normalize ? LS_FLAG_NORMALIZE : 0u) | LS_FLAG_ASYNC;
    // ls_ivf_set_small_batch: ONE predicate per (handle, k, nprobe) - ls_mq_plan.h; where it fails, the chains below
    const ls_mq_in mq_in = ivf_mq_in(v);
    const bool batch = !ss && nq >= 2 && ls_mq_ivf_served(mq_in, v->n, rows_bound, k);
    if (batch)
        if (int r = ls_grow_pinned(&v->h_m, &v->hm_cap, (size_t)(nq / 2 + 1))) return r;
    for (int64_t i = 0; i < nq;) {  // one chain per query - or per group -, all queued before the one wait
        hipEvent_t* pe = nullptr;
        int group = batch ? ls_mq_subset_group(nq - i) : 0;  // min(left, 16) while two or more are left
        ls_mq_plan mp{0, 0, 0};
        if (group) mp = ls_mq_ivf_plan(mq_in, v->n, rows_bound, k, group);
        if (group && mp.keys == 0) group = 0;
        if (group) {
            if (v->profiling && v->prof_n < LS_IVF_PROF_MAX) {
                if (int rc = ls_prof_events(v->ev, (size_t)v->prof_n, 3, &pe)) return rc;
                LS_HIP(hipEventRecord(pe[0], s));
            }
            // (a query's probe lists do not depend on its company: one centroid search for the group)
            if (int rc = ivf_coarse(v, i, group, np, cflags, s)) return rc;
            LS_HIP(hipSetDevice(v->device));
            if (pe) LS_HIP(hipEventRecord(pe[1], s));
            if (int rc = ivf_group_pass(v, i, group, k, np, normalize, rows_bound, mp, v->h_m + v->last_passes)) return rc;
            if (pe) {
                LS_HIP(hipEventRecord(pe[2], s));
                v->prof_n++;
            }
            v->last_passes++;
            i += group;
            continue;
        }
        if (v->profiling && v->prof_n < LS_IVF_PROF_MAX) {
            if (int rc = ls_prof_events(v->ev, (size_t)v->prof_n, 3, &pe)) return rc;
            LS_HIP(hipEventRecord(pe[0], s));
        }
        if (int rc = ivf_coarse(v, i, 1, np, cflags, s)) return rc;
        LS_HIP(hipSetDevice(v->device));
        if (pe) LS_HIP(hipEventRecord(pe[1], s));
        if (int rc = ivf_fine(v, ss, i, k, kf, np, normalize, rows_bound, nullptr)) return rc;
        if (pe) {
            LS_HIP(hipEventRecord(pe[2], s));
            v->prof_n++;
        }
        ++i;
    }
    LS_HIP(hipStreamSynchronize(s));
    for (int j = 0; j < v->last_passes; ++j) v->last_union_rows += v->h_m[j];
    if (*v->h_any) {
        v->flags_clean = false;
        v->h_flags.resize((size_t)nq);
        LS_HIP(hipMemcpy(v->h_flags.data(), v->d_flags, sizeof(u32) * (size_t)nq, hipMemcpyDeviceToHost));
        if (!v->d_S) LS_HIP(hipMalloc((void**)&v->d_S, sizeof(float) * (size_t)v->n));
        for (int64_t i = 0; i < nq; ++i) {
            if (!v->h_flags[(size_t)i]) continue;
            v->last_rescued++;
            LS_HIP(hipMemsetAsync(v->d_S, 0xff, sizeof(float) * (size_t)v->n, s));  // NaN: "this row was not probed"
            if (int rc = ivf_fine(v, ss, i, k, kf, np, normalize, rows_bound, v->d_S)) return rc;
        }
        LS_HIP(hipStreamSynchronize(s));
    }
    if (l2) std::transform(v->h_s, v->h_s + on, out_s, ls_l2_out);  // (-FLT_MAX in the unfilled slots: +FLT_MAX)
    else std::copy(v->h_s, v->h_s + on, out_s);
    std::copy(v->h_i, v->h_i + on, out_i);
    if (kf < k)  // a subset of fewer than k rows: the slots past its rows were not written
        for (int64_t i = 0; i < nq; ++i) {
            std::fill(out_s + i * k + kf, out_s + (i + 1) * k, pad);
            std::fill(out_i + i * k + kf, out_i + (i + 1) * k, (int64_t)-1);
        }
    return LS_OK;
}

// ---- range search (include/leansearch_range.h; the compaction is ls_range.hip's) ------------------------------------------
// Per group of up to LS_RANGE_GROUP queries: every query's coarse search (as above: its probe list lands in d_pi), its
// vector reset to NaN = "not probed", and the fine launch with S set - the launch ivf_fine makes for a rescue, without
// the selection (its keys are thrown away: the plan of k = 1); then the group's collect step over the vectors. The
// vectors are the handle's own block (not d_S: ls_ivf_search is untouched).
static int ivf_range_locked(ls_ivf* v, const ls_ivf_subset* ss, const float* q, int64_t nq, float radius, int np,
                            bool normalize, ls_range_result* res) {
    const int64_t rows_bound = ss ? ss->top_rows[(size_t)np] : v->top_rows[(size_t)np];
    if (nq == 0 || rows_bound == 0) return LS_OK;  // no row can be probed: every segment is empty, nothing is launched
    LS_HIP(hipSetDevice(v->device));
    hipStream_t s = v->stream;
    const size_t qn = (size_t)nq * v->d;
    if (int r = ls_grow_pinned(&v->h_q, &v->hq_cap, qn)) return r;
    if (int r = ls_grow(&v->d_q, &v->q_cap, qn)) return r;
    if (int r = ls_grow(&v->d_ps, &v->ps_cap, (size_t)nq * np)) return r;
    if (int r = ls_grow(&v->d_pi, &v->pi_cap, (size_t)nq * np)) return r;
    const int vecs = (int)std::min<int64_t>(nq, LS_RANGE_GROUP);
    if (v->rs_vecs < vecs) {  // (calls are synchronous and hold the mutex: nothing in flight reads the old block)
        (void)hipFree(v->d_RS);
        v->d_RS = nullptr;
        v->rs_vecs = 0;
        v->rs_stride = ls_range_stride(v->n);
        LS_HIP(hipMalloc((void**)&v->d_RS, sizeof(float) * (size_t)v->rs_stride * vecs));
        v->rs_vecs = vecs;
    }
    if (!v->range) v->range = new ls_range_scratch();
    std::copy(q, q + qn, v->h_q);
    LS_HIP(hipMemcpyAsync(v->d_q, v->h_q, sizeof(float) * qn, hipMemcpyHostToDevice, s));
    const uint32_t cflags = (normalize ? LS_FLAG_NORMALIZE : 0u) | LS_FLAG_ASYNC;
    // L2 handle: the vectors hold -distance, so dist < radius is S > -radius - the same strict predicate - and the emitted
    // scores leave as distances (as ls_range.hip does for flat handles)
    const bool l2 = v->metric == LS_METRIC_L2;
    const float s_radius = l2 ? -radius : radius;
    for (int64_t grp = 0; grp < ls_range_groups(nq); ++grp) {
        const int64_t q0 = grp * LS_RANGE_GROUP;
        const int G = ls_range_group_size(nq, grp);
        for (int j = 0; j < G; ++j) {
            const int64_t i = q0 + j;
            float* S = v->d_RS + (long long)j * v->rs_stride;
            if (int rc = ivf_coarse(v, i, 1, np, cflags, s)) return rc;
            LS_HIP(hipSetDevice(v->device));
            LS_HIP(hipMemsetAsync(S, 0xff, sizeof(float) * (size_t)v->n, s));  // NaN: "this row was not probed"
            if (int rc = ivf_launch_scan(v->rows->g, ivf_fine_args(v, ss, i, 1, np, normalize, rows_bound, S), s)) return rc;
        }
        if (int rc = ls_i_range_collect(*v->range, v->d_RS, v->rs_stride, v->n, G, s_radius, nullptr, 0, v->profiling, res,
                                        q0, s))
            return rc;
        if (l2) ls_i_range_l2_out(res, q0, G);
    }
    return LS_OK;
}

static int ivf_range_entry(const char* who, ls_ivf* v, bool with_subset, int32_t subset, const float* q, int64_t nq,
                           float radius, int32_t nprobe, uint32_t flags, ls_range_result** out) {
    if (out) *out = nullptr;
    if (!v || !out || nq < 0 || (nq > 0 && !q)) {
        ls_set_error("%s: bad argument (nq=%lld)", who, (long long)nq);
        return LS_ERR_INVALID_ARG;
    }
    if (nprobe < 1) {
        ls_set_error("%s: nprobe = %d (at least one list)", who, nprobe);
        return LS_ERR_INVALID_ARG;
    }
    if (flags & ~LS_FLAG_NORMALIZE) {
        ls_set_error("%s: unsupported flags 0x%x (only LS_FLAG_NORMALIZE)", who, flags);
        return LS_ERR_INVALID_ARG;
    }
    if (std::min(nprobe, v->nlist) > LS_IVF_MAX_PROBE) {
        ls_set_error("%s: min(nprobe, nlist) = %d exceeds LS_MAX_K = %d", who, std::min(nprobe, v->nlist), LS_MAX_K);
        return LS_ERR_INVALID_ARG;
    }
    const int np = std::min(nprobe, v->nlist);
    std::lock_guard<std::mutex> lk(v->mu);
    const ls_ivf_subset* ss = nullptr;
    if (with_subset) {
        auto it = v->subsets.find(subset);
        if (it == v->subsets.end()) {
            ls_set_error("%s: no subset %d on this handle", who, subset);
            return LS_ERR_INVALID_ARG;
        }
        ss = it->second;
    }
    if (int rc = ls_i_check_device(v->device)) return rc;
    ls_device_guard guard;
    ls_range_result* res = ls_i_range_result_new(nq);
    const int rc = ivf_range_locked(v, ss, q, nq, radius, np, (flags & LS_FLAG_NORMALIZE) != 0, res);
    if (rc != LS_OK) {
        ls_range_free(res);
        return rc;
    }
    *out = res;
    return LS_OK;
}

// the argument checks ls_ivf_search and ls_ivf_search_subset share (`who` names the call in the message)
static int ivf_check_search_args(const char* who, const ls_ivf* v, const float* q, int64_t nq, int32_t k, int32_t nprobe,
                                 uint32_t flags, const float* out_scores, const int64_t* out_rows) {
    if (!v || nq < 0 || k <= 0 || k > (1 << 20) || (nq > 0 && (!q || !out_scores || !out_rows))) {
        ls_set_error("%s: bad argument (nq=%lld k=%d)", who, (long long)nq, k);
        return LS_ERR_INVALID_ARG;
    }
    if (nprobe < 1) {
        ls_set_error("%s: nprobe = %d (at least one list)", who, nprobe);
        return LS_ERR_INVALID_ARG;
    }
    if (flags & ~LS_FLAG_NORMALIZE) {
        ls_set_error("%s: unsupported flags 0x%x (only LS_FLAG_NORMALIZE)", who, flags);
        return LS_ERR_INVALID_ARG;
    }
    if (std::min(nprobe, v->nlist) > LS_IVF_MAX_PROBE) {
        ls_set_error("%s: min(nprobe, nlist) = %d exceeds LS_MAX_K = %d", who, std::min(nprobe, v->nlist), LS_MAX_K);
        return LS_ERR_INVALID_ARG;
    }
    return LS_OK;
}

static int ivf_create(const char* who, int32_t metric, ls_ivf** out, const float* corpus, int64_t n, int32_t d,
                      int32_t dtype, const float* centroids, int32_t nlist, const int32_t* assign, int32_t device) {
    if (!out) {
        ls_set_error("%s: out is null", who);
        return LS_ERR_INVALID_ARG;
    }
    *out = nullptr;
    if (metric == LS_METRIC_L2 && dtype == LS_DTYPE_SQ8) {  // (before any device check)
        ls_set_error("%s: an L2 IVF index stores fp32 or fp16 rows (LS_DTYPE_SQ8 serves the inner product only)", who);
        return LS_ERR_INVALID_ARG;
    }
    if (metric == LS_METRIC_L2 && dtype == LS_DTYPE_BF16) {  // (likewise)
        ls_set_error("%s: an L2 IVF index stores fp32 or fp16 rows (bf16 rows, LS_DTYPE_BF16, serve the inner product only)", who);
        return LS_ERR_INVALID_ARG;
    }
    if (n < 0 || d <= 0 || (n > 0 && !corpus)) {
        ls_set_error("%s: bad shape n=%lld d=%d", who, (long long)n, d);
        return LS_ERR_INVALID_ARG;
    }
    if (nlist < 1 || !centroids) {
        ls_set_error("%s: nlist = %d (at least one list and its centroid)", who, nlist);
        return LS_ERR_INVALID_ARG;
    }
    if (dtype != LS_DTYPE_F32 && dtype != LS_DTYPE_F16 && dtype != LS_DTYPE_SQ8 && dtype != LS_DTYPE_BF16) {
        ls_set_error("%s: unknown dtype %d", who, dtype);
        return LS_ERR_INVALID_ARG;
    }
    ls_geom g;
    if (ls_pick_geom(d, dtype, &g) != LS_OK) {
        ls_set_error("%s: unsupported d=%d / dtype=%d (max stored row is 4096 bytes)", who, d, dtype);
        return LS_ERR_INVALID_ARG;
    }
    if (int rc = ls_i_check_device(device)) return rc;
    ls_device_guard guard;
    ls_ivf* v = new ls_ivf();
    v->device = device;
    v->n = n;
    v->d = d;
    v->dtype = dtype;
    v->nlist = nlist;
    v->metric = metric;
    const int rc = ivf_build(v, corpus, centroids, assign);
    if (rc != LS_OK) {
        ivf_free(v);
        return rc;
    }
    *out = v;
    return LS_OK;
}

extern "C" {

int ls_ivf_create(ls_ivf** out, const float* corpus, int64_t n, int32_t d, int32_t dtype, const float* centroids,
                  int32_t nlist, const int32_t* assign, int32_t device) {
    return ivf_create("ls_ivf_create", LS_METRIC_INNER_PRODUCT, out, corpus, n, d, dtype, centroids, nlist, assign, device);
}

int ls_ivf_create_l2(ls_ivf** out, const float* corpus, int64_t n, int32_t d, int32_t dtype, const float* centroids,
                     int32_t nlist, const int32_t* assign, int32_t device) {
    return ivf_create("ls_ivf_create_l2", LS_METRIC_L2, out, corpus, n, d, dtype, centroids, nlist, assign, device);
}

int32_t ls_ivf_metric(const ls_ivf* v) { return v ? v->metric : -1; }

int ls_ivf_search(ls_ivf* v, const float* q, int64_t nq, int32_t k, int32_t nprobe, uint32_t flags, float* out_scores,
                  int64_t* out_rows) {
    if (int rc = ivf_check_search_args("ls_ivf_search", v, q, nq, k, nprobe, flags, out_scores, out_rows)) return rc;
    const int np = std::min(nprobe, v->nlist);
    if (std::min<int64_t>(k, v->n) > LS_MAX_K) {
        ls_set_error("ls_ivf_search: min(k, rows of the index) = %lld exceeds LS_MAX_K = %d",
                     (long long)std::min<int64_t>(k, v->n), LS_MAX_K);
        return LS_ERR_K_TOO_LARGE;
    }
    if (int rc = ls_i_check_device(v->device)) return rc;
    if (nq == 0) return LS_OK;
    std::lock_guard<std::mutex> lk(v->mu);
    ls_device_guard guard;
    return ivf_search_locked(v, nullptr, q, nq, k, np, (flags & LS_FLAG_NORMALIZE) != 0, out_scores, out_rows);
}

int ls_ivf_subset_create(ls_ivf* v, const uint8_t* bitmap, int64_t nbytes, int32_t* out_id, int64_t* out_rows) {
    if (!v || !out_id || nbytes < 0 || (nbytes > 0 && !bitmap)) {
        ls_set_error("ls_ivf_subset_create: bad argument");
        return LS_ERR_INVALID_ARG;
    }
    if (int rc = ls_i_check_device(v->device)) return rc;
    std::lock_guard<std::mutex> lk(v->mu);  // (ls_ivf_add changes the host tables: compacted under the lock)
    ls_ivf_subset_plan plan;
    ls_ivf_subset_compact(v->assign.data(), v->n, v->nlist, v->off.data(), bitmap, nbytes, plan);
    ls_ivf_subset* ss = new ls_ivf_subset();
    ss->m = plan.m;
    ss->top_rows = std::move(plan.top_rows);
    ss->sizes.resize((size_t)v->nlist);
    for (int32_t l = 0; l < v->nlist; ++l) ss->sizes[(size_t)l] = (int64_t)plan.soff[(size_t)l + 1] - plan.soff[(size_t)l];
    ls_device_guard guard;
    auto upload = [&]() -> int {
        LS_HIP(hipSetDevice(v->device));
        const size_t mm = (size_t)std::max<int64_t>(ss->m, 1);
        LS_HIP(hipMalloc((void**)&ss->d_soff, sizeof(u32) * ((size_t)v->nlist + 1)));
        LS_HIP(hipMalloc((void**)&ss->d_srow, sizeof(u32) * mm));
        LS_HIP(hipMalloc((void**)&ss->d_sid, sizeof(u32) * mm));
        LS_HIP(hipMemcpy(ss->d_soff, plan.soff.data(), sizeof(u32) * ((size_t)v->nlist + 1), hipMemcpyHostToDevice));
        if (ss->m > 0) {
            LS_HIP(hipMemcpy(ss->d_srow, plan.srow.data(), sizeof(u32) * (size_t)ss->m, hipMemcpyHostToDevice));
            LS_HIP(hipMemcpy(ss->d_sid, plan.sid.data(), sizeof(u32) * (size_t)ss->m, hipMemcpyHostToDevice));
        }
        return LS_OK;
    };
    const int rc = upload();
    if (rc != LS_OK) {
        ivf_subset_free(ss);
        return rc;
    }
    const int32_t id = v->next_subset++;
    v->subsets[id] = ss;
    *out_id = id;
    if (out_rows) *out_rows = ss->m;
    return LS_OK;
}

int ls_ivf_subset_destroy(ls_ivf* v, int32_t subset) {
    if (!v) {
        ls_set_error("ls_ivf_subset_destroy: handle is null");
        return LS_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lk(v->mu);
    auto it = v->subsets.find(subset);
    if (it == v->subsets.end()) {
        ls_set_error("ls_ivf_subset_destroy: no subset %d on this handle", subset);
        return LS_ERR_INVALID_ARG;
    }
    ls_ivf_subset* ss = it->second;
    v->subsets.erase(it);
    ls_device_guard guard;
    (void)hipSetDevice(v->device);
    ivf_subset_free(ss);  // (searches are synchronous and hold the mutex: nothing in flight reads it)
    return LS_OK;
}

int ls_ivf_subset_list_sizes(ls_ivf* v, int32_t subset, int64_t* out) {
    if (!v || !out) {
        ls_set_error("ls_ivf_subset_list_sizes: bad argument");
        return LS_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lk(v->mu);
    auto it = v->subsets.find(subset);
    if (it == v->subsets.end()) {
        ls_set_error("ls_ivf_subset_list_sizes: no subset %d on this handle", subset);
        return LS_ERR_INVALID_ARG;
    }
    std::copy(it->second->sizes.begin(), it->second->sizes.end(), out);
    return LS_OK;
}

int ls_ivf_search_subset(ls_ivf* v, int32_t subset, const float* q, int64_t nq, int32_t k, int32_t nprobe,
                         uint32_t flags, float* out_scores, int64_t* out_rows) {
    if (int rc = ivf_check_search_args("ls_ivf_search_subset", v, q, nq, k, nprobe, flags, out_scores, out_rows))
        return rc;
    const int np = std::min(nprobe, v->nlist);
    std::lock_guard<std::mutex> lk(v->mu);
    auto it = v->subsets.find(subset);
    if (it == v->subsets.end()) {
        ls_set_error("ls_ivf_search_subset: no subset %d on this handle", subset);
        return LS_ERR_INVALID_ARG;
    }
    const ls_ivf_subset* ss = it->second;
    if (std::min<int64_t>(k, ss->m) > LS_MAX_K) {
        ls_set_error("ls_ivf_search_subset: min(k, selected rows) = %lld exceeds LS_MAX_K = %d",
                     (long long)std::min<int64_t>(k, ss->m), LS_MAX_K);
        return LS_ERR_K_TOO_LARGE;
    }
    if (int rc = ls_i_check_device(v->device)) return rc;
    if (nq == 0) return LS_OK;
    ls_device_guard guard;
    return ivf_search_locked(v, ss, q, nq, k, np, (flags & LS_FLAG_NORMALIZE) != 0, out_scores, out_rows);
}

int ls_ivf_range_search(ls_ivf* v, const float* q, int64_t nq, float radius, int32_t nprobe, uint32_t flags,
                        ls_range_result** out) {
    return ivf_range_entry("ls_ivf_range_search", v, false, 0, q, nq, radius, nprobe, flags, out);
}

int ls_ivf_range_search_subset(ls_ivf* v, int32_t subset, const float* q, int64_t nq, float radius, int32_t nprobe,
                               uint32_t flags, ls_range_result** out) {
    return ivf_range_entry("ls_ivf_range_search_subset", v, true, subset, q, nq, radius, nprobe, flags, out);
}

int64_t ls_ivf_ntotal(const ls_ivf* v) { return v ? v->n : 0; }
int32_t ls_ivf_dim(const ls_ivf* v) { return v ? v->d : 0; }
int32_t ls_ivf_nlist(const ls_ivf* v) { return v ? v->nlist : 0; }

int ls_ivf_list_sizes(const ls_ivf* v, int64_t* out) {
    if (!v || !out) {
        ls_set_error("ls_ivf_list_sizes: bad argument");
        return LS_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lk(v->mu);
    std::copy(v->sizes.begin(), v->sizes.end(), out);
    return LS_OK;
}

int ls_ivf_assignment(const ls_ivf* v, int32_t* out) {
    if (!v || (v->n > 0 && !out)) {
        ls_set_error("ls_ivf_assignment: bad argument");
        return LS_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lk(v->mu);
    std::copy(v->assign.begin(), v->assign.end(), out);
    return LS_OK;
}

// (include/leansearch_ivf_build.h) rows [row0, row0 + count) in ORIGINAL order. The handle stores the rows list after
// list: original row r sits at storage row off[assign[r]] + (rows of its list before r). The wanted storage rows are
// read slab by slab through the rows index's own ls_reconstruct (only slabs that hold a wanted row) and scattered.
int ls_ivf_reconstruct(ls_ivf* v, int64_t row0, int64_t count, float* out) {
    if (!v || row0 < 0 || count < 0 || row0 + count > v->n || (count > 0 && !out)) {
        ls_set_error("ls_ivf_reconstruct: bad argument");
        return LS_ERR_INVALID_ARG;
    }
    if (count == 0) return LS_OK;
    if (int rc = ls_i_check_device(v->device)) return rc;
    std::lock_guard<std::mutex> lk(v->mu);
    const int32_t d = v->d;
    std::vector<std::pair<u32, int64_t>> want((size_t)count);  // (storage row, original row)
    {
        std::vector<u32> at(v->off.begin(), v->off.end() - 1);
        for (int64_t r = 0; r < row0 + count; ++r) {
            const u32 s = at[(size_t)v->assign[(size_t)r]]++;
            if (r >= row0) want[(size_t)(r - row0)] = {s, r};
        }
    }
    std::sort(want.begin(), want.end());
    const int64_t slab = std::max<int64_t>(1, (int64_t)(64ll << 20) / ((int64_t)d * 4));
    std::vector<float> buf;
    for (size_t i = 0; i < want.size();) {
        const int64_t s0 = want[i].first, m = std::min<int64_t>(slab, v->n - s0);
        buf.resize((size_t)m * d);
        if (int rc = ls_reconstruct(v->rows, s0, m, buf.data())) return rc;
        for (; i < want.size() && (int64_t)want[i].first < s0 + m; ++i)
            std::copy(buf.begin() + ((int64_t)want[i].first - s0) * d, buf.begin() + ((int64_t)want[i].first - s0 + 1) * d,
                      out + (want[i].second - row0) * d);
    }
    return LS_OK;
}

void ls_ivf_destroy(ls_ivf* v) {
    if (!v) return;
    { std::lock_guard<std::mutex> lk(v->mu); }
    ivf_free(v);
}

int ls_ivf_set_profiling(ls_ivf* v, int32_t enabled) {
    if (!v) {
        ls_set_error("ls_ivf_set_profiling: handle is null");
        return LS_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lk(v->mu);
    v->profiling = enabled != 0;
    v->prof_n = 0;
    return LS_OK;
}

int ls_ivf_set_small_batch(ls_ivf* v, int32_t enable) {
    if (!v) {
        ls_set_error("ls_ivf_set_small_batch: handle is null");
        return LS_ERR_INVALID_ARG;
    }
    const ls_switch_answer a = ls_switch_ask(LS_SW_IVF, v->metric, v->dtype, LS_PLACE_NA, enable);
    if (a.rc != LS_OK) {  // (before any device check)
        ls_set_error(a.fmt, a.fill);
        return a.rc;
    }
    std::lock_guard<std::mutex> lk(v->mu);  // (searches are synchronous and hold the mutex: nothing is in flight)
    if (!enable) {
        v->small_batch = false;
        return LS_OK;
    }
    if (v->cand_queries < LS_MQ_NQ) {  // first time on: candidate blocks for 16 queries, the union step's arrays
        if (int rc = ls_i_check_device(v->device)) return rc;
        ls_device_guard guard;
        LS_HIP(hipSetDevice(v->device));
        LS_HIP(hipStreamSynchronize(v->stream));
        ls_ivf_union& u = v->un;
        u.cap = (std::max<int64_t>(v->n, 1) + 15) / 16 * 16 + 16;
        if (!u.lmask) LS_HIP(hipMalloc((void**)&u.lmask, sizeof(u32) * (size_t)v->nlist));
        if (!u.lpre) LS_HIP(hipMalloc((void**)&u.lpre, sizeof(u32) * ((size_t)v->nlist + 1)));
        if (!u.row) LS_HIP(hipMalloc((void**)&u.row, sizeof(u32) * (size_t)u.cap));
        if (!u.id) LS_HIP(hipMalloc((void**)&u.id, sizeof(u32) * (size_t)u.cap));
        if (!u.mask) LS_HIP(hipMalloc((void**)&u.mask, sizeof(unsigned short) * (size_t)u.cap));
        if (!u.m) LS_HIP(hipMalloc((void**)&u.m, sizeof(u32)));
        LS_HIP(hipMemset(u.m, 0, sizeof(u32)));
        u64 *cand = nullptr, *bound = nullptr;
        LS_HIP(hipMalloc((void**)&cand, sizeof(u64) * (size_t)LS_MQ_NQ * v->max_blocks * LS_KP_MAX));
        if (hipMalloc((void**)&bound, sizeof(u64) * (size_t)LS_MQ_NQ * v->max_blocks) != hipSuccess) {
            (void)hipFree(cand);
            ls_set_error("ls_ivf_set_small_batch: out of device memory");
            return LS_ERR_HIP;
        }
        (void)hipFree(v->d_cand);
        (void)hipFree(v->d_bound);
        v->d_cand = cand;
        v->d_bound = bound;
        v->cand_queries = LS_MQ_NQ;
    }
    v->small_batch = true;
    return LS_OK;
}

int ls_ivf_last_passes(ls_ivf* v, int32_t* passes, int64_t* union_rows) {
    if (!v) {
        ls_set_error("ls_ivf_last_passes: handle is null");
        return LS_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lk(v->mu);
    if (passes) *passes = v->last_passes;
    if (union_rows) *union_rows = v->last_union_rows;
    return LS_OK;
}

int ls_ivf_last_kernel_ms(ls_ivf* v, float* coarse_ms, float* fine_ms, int32_t* rescued) {
    if (!v) {
        ls_set_error("ls_ivf_last_kernel_ms: handle is null");
        return LS_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lk(v->mu);
    float c = 0.0f, f = 0.0f;
    if (v->prof_n > 0) {
        ls_device_guard guard;
        LS_HIP(hipSetDevice(v->device));
        for (int i = 0; i < v->prof_n; ++i) {
            float a = 0.0f, b = 0.0f;
            LS_HIP(hipEventElapsedTime(&a, v->ev[3 * (size_t)i], v->ev[3 * (size_t)i + 1]));
            LS_HIP(hipEventElapsedTime(&b, v->ev[3 * (size_t)i + 1], v->ev[3 * (size_t)i + 2]));
            c += a;
            f += b;
        }
    }
    if (coarse_ms) *coarse_ms = c;
    if (fine_ms) *fine_ms = f;
    if (rescued) *rescued = v->last_rescued;
    return LS_OK;
}

}  // extern "C"
