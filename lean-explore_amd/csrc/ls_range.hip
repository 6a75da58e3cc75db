// ls_range.hip — range search (include/leansearch_range.h): every row whose score exceeds a radius.
//
// The scores are the unchanged scan kernels': a query's scan launch writes its score vector S (rows of a flat handle,
// list positions of a flat subset, original rows of an IVF handle with NaN = "not probed"). This file is the step from
// S to a compacted, ordered, variable-length result - a deterministic threshold compaction in three launches per group
// of up to LS_RANGE_GROUP queries (grid.y = the query), dealt by ls_range_plan.h:
//   count    one workgroup per slab of LS_RANGE_SLAB rows: 16-byte loads, the predicate, four ballots per wave, the
//            waves' totals through LDS -> cnt[q][slab].
//   offsets  one workgroup per query: the 64-bit exclusive prefix of its slab counts -> off[q][slab], and the query's
//            total into pinned host memory.
//   emit     the count kernel's traversal again; a hit's slot is its query's base + off[q][slab] + its rank inside
//            the slab in (thread, component) order - row order. rows[slot] = (map ? map[pos] : pos) + base, scores[slot].
// No atomics, no workgroup waits for another, nothing depends on timing: the result is a function of S alone.
//
// Host flow per group (ls_i_range_collect): the scans are queued first, then count and offsets; ONE wait; the totals
// size the device result buffers (ls_grow) and the group's slice of the result object; emit and the copies into the
// result at its lims; ONE wait. The flat entry points live here; the IVF ones (ls_ivf.hip) queue their own scans and
// share the collect step.
#include "ls_range_plan.h"
#include "ls_subset_state.h"
#include "../../include/leansearch_range.h"

#include <algorithm>
#include <vector>

struct ls_range_result {
    int64_t nq = 0;
    std::vector<int64_t> lims;  // [nq + 1]
    std::vector<float> scores;
    std::vector<int64_t> rows;
    float kernel_ms = 0.0f;
};

struct ls_range_bases {
    long long at[LS_RANGE_GROUP];  // first slot of every query of the group in the group's device buffers
};

// the four rows of thread `tid` of `slab`: hit[c] = row r0 + c exists and passes the predicate
__device__ __forceinline__ void ls_range_look(const float* __restrict__ S, long long n, long long r0, float radius,
                                              float (&v)[LS_RANGE_VEC], bool (&hit)[LS_RANGE_VEC]) {
#pragma unroll
    for (int c = 0; c < LS_RANGE_VEC; ++c) {
        v[c] = 0.0f;
        hit[c] = false;
    }
    if (r0 < n) {  // (r0 is a multiple of 4 below n and the vector is allocated in multiples of 64 floats)
        const float4 x = *reinterpret_cast<const float4*>(S + r0);
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
#pragma unroll
        for (int c = 0; c < LS_RANGE_VEC; ++c) hit[c] = r0 + c < n && ls_range_hit(v[c], radius);
    }
}

__global__ __launch_bounds__(LS_RANGE_THREADS) void ls_range_count_kernel(const float* __restrict__ S, long long s_stride,
                                                                          long long n, float radius,
                                                                          u32* __restrict__ cnt, long long nslab) {
    __shared__ u32 wt[LS_RANGE_WAVES];
    const int tid = threadIdx.x, lane = tid & (LS_RANGE_WAVE - 1), wave = tid / LS_RANGE_WAVE;
    const long long slab = blockIdx.x, q = blockIdx.y;
    float v[LS_RANGE_VEC];
    bool hit[LS_RANGE_VEC];
    ls_range_look(S + q * s_stride, n, ls_range_row0(slab, tid), radius, v, hit);
    unsigned long long b[LS_RANGE_VEC];
#pragma unroll
    for (int c = 0; c < LS_RANGE_VEC; ++c) b[c] = __ballot(hit[c]);
    if (lane == 0) wt[wave] = ls_range_wave_total(b);
    __syncthreads();
    if (tid == 0) cnt[q * nslab + slab] = ls_range_slab_total(wt);
}

__global__ __launch_bounds__(LS_RANGE_OFF_THREADS) void ls_range_offsets_kernel(const u32* __restrict__ cnt,
                                                                                long long nslab,
                                                                                long long* __restrict__ off,
                                                                                long long* __restrict__ total) {
    __shared__ long long part[LS_RANGE_OFF_THREADS];
    const int tid = threadIdx.x;
    const long long q = blockIdx.x;
    const long long b = ls_range_seg_begin(nslab, tid), e = ls_range_seg_end(nslab, tid);
    const u32* c = cnt + q * nslab;
    long long s = 0;
    for (long long i = b; i < e; ++i) s += c[i];
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < LS_RANGE_OFF_THREADS; o <<= 1) {  // inclusive scan of the segment sums
        const long long x = tid >= o ? part[tid - o] : 0ll;
        __syncthreads();
        part[tid] += x;
        __syncthreads();
    }
    long long run = tid ? part[tid - 1] : 0ll;
    for (long long i = b; i < e; ++i) {
        off[q * nslab + i] = run;
        run += c[i];
    }
    if (tid == LS_RANGE_OFF_THREADS - 1) total[q] = part[LS_RANGE_OFF_THREADS - 1];
}

__global__ __launch_bounds__(LS_RANGE_THREADS) void ls_range_emit_kernel(const float* __restrict__ S, long long s_stride,
                                                                         long long n, float radius,
                                                                         const long long* __restrict__ off,
                                                                         long long nslab, ls_range_bases qb,
                                                                         const u32* __restrict__ map, long long base,
                                                                         float* __restrict__ scores,
                                                                         long long* __restrict__ rows) {
    __shared__ u32 wt[LS_RANGE_WAVES];
    const int tid = threadIdx.x, lane = tid & (LS_RANGE_WAVE - 1), wave = tid / LS_RANGE_WAVE;
    const long long slab = blockIdx.x, q = blockIdx.y;
    const long long r0 = ls_range_row0(slab, tid);
    float v[LS_RANGE_VEC];
    bool hit[LS_RANGE_VEC];
    ls_range_look(S + q * s_stride, n, r0, radius, v, hit);
    unsigned long long b[LS_RANGE_VEC];
#pragma unroll
    for (int c = 0; c < LS_RANGE_VEC; ++c) b[c] = __ballot(hit[c]);
    if (lane == 0) wt[wave] = ls_range_wave_total(b);
    __syncthreads();
    const long long slot0 = qb.at[q] + off[q * nslab + slab] + ls_range_wave_base(wt, wave) + ls_range_lane_rank(b, lane);
#pragma unroll
    for (int c = 0; c < LS_RANGE_VEC; ++c)
        if (hit[c]) {
            const long long slot = slot0 + ls_range_comp_rank(b, lane, c);
            const long long pos = r0 + c;
            rows[slot] = (map ? (long long)map[pos] : pos) + base;
            scores[slot] = v[c] + 0.0f;  // (-0.0 comes out as +0.0, as the selection's keys give it: ls_ord)
        }
}

void ls_i_range_scratch_free(ls_range_scratch* rs) {
    if (!rs) return;
    (void)hipFree(rs->d_cnt);
    (void)hipFree(rs->d_off);
    (void)hipFree(rs->d_scores);
    (void)hipFree(rs->d_rows);
    if (rs->h_q) (void)hipHostFree(rs->h_q);
    if (rs->h_total) (void)hipHostFree(rs->h_total);
    for (hipEvent_t e : rs->ev)
        if (e) (void)hipEventDestroy(e);
    delete rs;
}

ls_range_result* ls_i_range_result_new(int64_t nq) {
    ls_range_result* r = new ls_range_result();
    r->nq = nq;
    r->lims.assign((size_t)nq + 1, 0);
    return r;
}

// L2 handles: the segments of queries [q0, q0 + G) were collected as -distance and leave as distances
void ls_i_range_l2_out(ls_range_result* res, int64_t q0, int G) {
    for (size_t e = (size_t)res->lims[(size_t)q0]; e < (size_t)res->lims[(size_t)(q0 + G)]; ++e)
        res->scores[e] = ls_l2_out(res->scores[e]);
}

int ls_i_range_collect(ls_range_scratch& rs, const float* d_S, long long s_stride, long long n, int G, float radius,
                       const u32* map, long long base, bool prof, ls_range_result* res, int64_t q0, hipStream_t s) {
    if (G < 1 || G > LS_RANGE_GROUP || q0 < 0 || q0 + G > res->nq) {
        ls_set_error("ls_range_search: a group of %d queries at %lld of %lld", G, (long long)q0, (long long)res->nq);
        return LS_ERR_INVALID_ARG;
    }
    const long long nslab = ls_range_slabs(n);
    if (nslab == 0) {
        for (int j = 0; j < G; ++j) res->lims[(size_t)(q0 + j + 1)] = res->lims[(size_t)(q0 + j)];
        return LS_OK;
    }
    if (nslab > 0x7fffffffll) {
        ls_set_error("ls_range_search: %lld rows exceed one launch's slabs", n);
        return LS_ERR_INVALID_ARG;
    }
    if (int rc = ls_grow(&rs.d_cnt, &rs.cnt_cap, (size_t)G * nslab)) return rc;
    if (int rc = ls_grow(&rs.d_off, &rs.off_cap, (size_t)G * nslab)) return rc;
    if (!rs.h_total) LS_HIP(hipHostMalloc((void**)&rs.h_total, sizeof(long long) * LS_RANGE_GROUP, hipHostMallocDefault));
    if (prof)
        for (hipEvent_t& e : rs.ev)
            if (!e) LS_HIP(hipEventCreate(&e));
    const dim3 grid((unsigned)nslab, (unsigned)G);
    if (prof) LS_HIP(hipEventRecord(rs.ev[0], s));
    hipLaunchKernelGGL(ls_range_count_kernel, grid, dim3(LS_RANGE_THREADS), 0, s, d_S, s_stride, n, radius, rs.d_cnt,
                       nslab);
    LS_HIP(hipGetLastError());
    hipLaunchKernelGGL(ls_range_offsets_kernel, dim3((unsigned)G), dim3(LS_RANGE_OFF_THREADS), 0, s,
                       (const u32*)rs.d_cnt, nslab, rs.d_off, rs.h_total);
    LS_HIP(hipGetLastError());
    if (prof) LS_HIP(hipEventRecord(rs.ev[1], s));
    LS_HIP(hipStreamSynchronize(s));
    ls_range_bases qb{};
    long long total = 0;
    for (int j = 0; j < G; ++j) {
        qb.at[j] = total;
        total += rs.h_total[j];
        res->lims[(size_t)(q0 + j + 1)] = res->lims[(size_t)(q0 + j)] + rs.h_total[j];
    }
    if (total > 0) {
        if (int rc = ls_grow(&rs.d_scores, &rs.scores_cap, (size_t)total)) return rc;
        if (int rc = ls_grow(&rs.d_rows, &rs.rows_cap, (size_t)total)) return rc;
        const size_t at = (size_t)res->lims[(size_t)q0];
        res->scores.resize(at + (size_t)total);
        res->rows.resize(at + (size_t)total);
        if (prof) LS_HIP(hipEventRecord(rs.ev[2], s));
        hipLaunchKernelGGL(ls_range_emit_kernel, grid, dim3(LS_RANGE_THREADS), 0, s, d_S, s_stride, n, radius,
                           (const long long*)rs.d_off, nslab, qb, map, base, rs.d_scores, rs.d_rows);
        LS_HIP(hipGetLastError());
        if (prof) LS_HIP(hipEventRecord(rs.ev[3], s));
        LS_HIP(hipMemcpyAsync(res->scores.data() + at, rs.d_scores, sizeof(float) * (size_t)total, hipMemcpyDeviceToHost, s));
        LS_HIP(hipMemcpyAsync(res->rows.data() + at, rs.d_rows, sizeof(long long) * (size_t)total, hipMemcpyDeviceToHost, s));
        LS_HIP(hipStreamSynchronize(s));
    }
    if (prof) {
        float a = 0.0f, b = 0.0f;
        LS_HIP(hipEventElapsedTime(&a, rs.ev[0], rs.ev[1]));
        if (total > 0) LS_HIP(hipEventElapsedTime(&b, rs.ev[2], rs.ev[3]));
        res->kernel_ms += a + b;
    }
    return LS_OK;
}

// ---- flat handles (the caller holds the handle's ls_quiesce) ----------------------------------------------------------
// One scan launch per query - the plain single-query scan, or the row-list scan over subset `ss` - into the score
// vectors of one scratch generation, taken the way a subset search takes it; then the group's collect step.
static int range_flat(ls_index* ix, const ls_subset* ss, const float* q, int64_t nq, float radius, bool normalize,
                      ls_range_result* res) {
    const int64_t rows = ss ? ss->m : ix->n;
    if (nq == 0 || rows <= 0) return LS_OK;  // nothing to launch: every segment is empty
    LS_HIP(hipSetDevice(ix->device));
    if (!ix->range) ix->range = new ls_range_scratch();
    ls_range_scratch& rs = *ix->range;
    const ls_geom& g = ix->g;
    const size_t qn = (size_t)nq * g.d;
    if (int rc = ls_grow_pinned(&rs.h_q, &rs.hq_cap, qn)) return rc;
    std::copy(q, q + qn, rs.h_q);
    const int blocks = ix->opt_blocks > 0 ? std::min(ix->opt_blocks, ix->max_blocks) : ls_scan_blocks(rows, g, ix->n_cu);
    const int kprime = ls_i_pick_kprime(ix, blocks, 1);  // (the launch's own top-k' work is thrown away: the plan of k = 1)
    // L2 handle (ls_index::metric): S holds -distance, so dist < radius is S > -radius - the same strict predicate - and the
    // emitted scores leave as distances (radius <= 0, -inf, NaN: nothing passes; +inf: every valid row)
    const bool l2 = ix->metric == LS_METRIC_L2;
    const float s_radius = l2 ? -radius : radius;
    hipStream_t s = ix->own_stream;
    for (int64_t grp = 0; grp < ls_range_groups(nq); ++grp) {
        const int64_t q0 = grp * LS_RANGE_GROUP;
        const int G = ls_range_group_size(nq, grp);
        if (int rc = ls_i_flush_pending(ix)) return rc;  // (their jobs name a scratch generation)
        const int gen = (int)(ix->set_rr++ % LS_NSETS);
        ls_index::scratch_set& st = ix->sets[gen];
        if (st.last_stream && st.last_stream != s) LS_HIP(hipStreamSynchronize(st.last_stream));
        st.last_stream = s;
        for (int j = 0; j < G; ++j) {
            ls_scan_args a{};
            a.d_q = rs.h_q + (q0 + j) * g.d;
            a.nq = 1;
            a.normalize = normalize;
            a.reverse = false;
            ls_fill_scratch_args(a, ix, st, blocks, kprime);
            a.d_S = st.d_S + (long long)j * ix->s_stride;
            a.mq_keys = 0;
            a.nfin = 0;
            a.d_step = ix->d_sq8_step;
            a.l2 = l2;
            if (int rc = ss ? ls_launch_scan_subset(ix->d_corpus, ss->d_list, rows, g, a, s)
                            : ls_launch_scan(ix->d_corpus, rows, g, a, s))
                return rc;
        }
        ix->n_launches_total += (uint64_t)G;  // (the scans)
        if (int rc = ls_i_range_collect(rs, st.d_S, ix->s_stride, rows, G, s_radius, ss ? ss->d_list : nullptr, ix->base,
                                        ix->profiling, res, q0, s))
            return rc;
        if (l2) ls_i_range_l2_out(res, q0, G);
    }
    return LS_OK;
}

static int range_flat_entry(const char* who, ls_index* ix, bool with_subset, int32_t subset, const float* q, int64_t nq,
                            float radius, uint32_t flags, ls_range_result** out) {
    if (out) *out = nullptr;
    if (!ix || !out || nq < 0 || (nq > 0 && !q)) {
        ls_set_error("%s: bad argument (nq=%lld)", who, (long long)nq);
        return LS_ERR_INVALID_ARG;
    }
    if (flags & ~LS_FLAG_NORMALIZE) {
        ls_set_error("%s: unsupported flags 0x%x (only LS_FLAG_NORMALIZE)", who, flags);
        return LS_ERR_INVALID_ARG;
    }
    if (ix->group) {
        ls_set_error("%s: a %s handle (range search serves single-device handles)", who,
                     ls_group_is_replicated(ix) ? "replicated" : "sharded");
        return LS_ERR_INVALID_ARG;
    }
    if (int rc = ls_i_check_device(ix->device)) return rc;
    ls_quiesce lk(ix);
    const ls_subset* ss = nullptr;
    if (with_subset) {
        if (ix->subsets) {
            auto it = ix->subsets->by_id.find(subset);
            if (it != ix->subsets->by_id.end()) ss = it->second;
        }
        if (!ss) {
            ls_set_error("%s: no subset %d on this handle", who, subset);
            return LS_ERR_INVALID_ARG;
        }
    }
    ls_device_guard guard;
    ls_range_result* res = ls_i_range_result_new(nq);
    const int rc = range_flat(ix, ss, q, nq, radius, (flags & LS_FLAG_NORMALIZE) != 0, res);
    if (rc != LS_OK) {
        delete res;
        return rc;
    }
    *out = res;
    return LS_OK;
}

extern "C" {

int ls_range_search(ls_index* ix, const float* q, int64_t nq, float radius, uint32_t flags, ls_range_result** out) {
    return range_flat_entry("ls_range_search", ix, false, 0, q, nq, radius, flags, out);
}

int ls_range_search_subset(ls_index* ix, int32_t subset, const float* q, int64_t nq, float radius, uint32_t flags,
                           ls_range_result** out) {
    return range_flat_entry("ls_range_search_subset", ix, true, subset, q, nq, radius, flags, out);
}

int64_t ls_range_nq(const ls_range_result* r) { return r ? r->nq : 0; }
const int64_t* ls_range_lims(const ls_range_result* r) { return r ? r->lims.data() : nullptr; }
const float* ls_range_scores(const ls_range_result* r) { return r && !r->scores.empty() ? r->scores.data() : nullptr; }
const int64_t* ls_range_rows(const ls_range_result* r) { return r && !r->rows.empty() ? r->rows.data() : nullptr; }
float ls_range_kernel_ms(const ls_range_result* r) { return r ? r->kernel_ms : 0.0f; }
void ls_range_free(ls_range_result* r) { delete r; }

}  // extern "C"
