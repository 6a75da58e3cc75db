// ls_subset.hip — exact search over a subset of the rows of one index (faiss IDSelectorBitmap semantics).
//
// A subset is the ascending list of the selected local rows of a handle, built once from a bitmap at
// ls_subset_create (row r selected iff (bitmap[r >> 3] >> (r & 7)) & 1) and owned by the handle. A subset search is
// the plain single-query scan with one change: the row loads go through the list (ls_scan.hip, RowList). Everything
// else - tiles, score vector, keys, bounds, the finalize and its rescue - works in list positions over an index of m
// "rows"; the list is ascending, so position order is row order and ties still come out row-ascending. Results are
// mapped pos -> list[pos] + base at the end: on the host (synchronous calls) or by ls_subset_map_kernel (the shards of
// a sharded handle, whose results feed the device merge).
//
// Several queries (ls_set_subset_small_batch, fp32 single-device handles, off by default): where the plan of
// ls_mq_plan.h (LS_MQ_ROWLIST) serves the (subset, k), groups of 2..16 queries of a call share ONE pass over the
// selected rows (ls_mq_subset.hip: the same bits on the f32 matrix cores) and one finalize launch carries the group's
// jobs; a lone query, and every call with the option off, takes the single-query launches above.
//
// Compaction (per handle, at creation): per-workgroup popcounts of 8192 bits, one workgroup's deterministic exclusive
// scan of the counts, then every workgroup writes its rows at its offset with ballot + mbcnt. Handles up to 2^32 - 1
// rows (u32 list entries and offsets).
#include "ls_subset_state.h"  // ls_subset, ls_subset_state (shared with ls_remove.hip)

#include <algorithm>
#include <memory>

#define LS_SUB_WG 256
#define LS_SUB_ITERS 32
#define LS_SUB_ROWS (LS_SUB_WG * LS_SUB_ITERS)  // bits one compaction workgroup covers
#define LS_SUB_SCAN_THREADS 1024

__device__ __forceinline__ bool ls_sub_bit(const unsigned char* __restrict__ bm, long long off, long long r) {
    const long long b = off + r;
    return (bm[b >> 3] >> (b & 7)) & 1;
}

__global__ __launch_bounds__(LS_SUB_WG) void ls_subset_count_kernel(const unsigned char* __restrict__ bm, long long off,
                                                                    long long rows, u32* __restrict__ counts) {
    __shared__ u32 wc[LS_SUB_WG / LS_WAVE];
    const long long r0 = (long long)blockIdx.x * LS_SUB_ROWS;
    u32 c = 0;
    for (int i = 0; i < LS_SUB_ITERS; ++i) {
        const long long r = r0 + (long long)i * LS_SUB_WG + threadIdx.x;
        c += (u32)__popcll(__ballot(r < rows && ls_sub_bit(bm, off, r)));
    }
    if ((threadIdx.x & (LS_WAVE - 1)) == 0) wc[threadIdx.x / LS_WAVE] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 t = 0;
        for (int w = 0; w < LS_SUB_WG / LS_WAVE; ++w) t += wc[w];
        counts[blockIdx.x] = t;
    }
}

// counts[0 .. nwg) -> exclusive offsets in place, total in *total. One workgroup: thread t owns a contiguous segment.
__global__ __launch_bounds__(LS_SUB_SCAN_THREADS) void ls_subset_scan_kernel(u32* __restrict__ counts, long long nwg,
                                                                            u32* __restrict__ total) {
    __shared__ u32 part[LS_SUB_SCAN_THREADS];
    const long long per = (nwg + LS_SUB_SCAN_THREADS - 1) / LS_SUB_SCAN_THREADS;
    const long long b = (long long)threadIdx.x * per, e = std::min(b + per, nwg);
    u32 s = 0;
    for (long long i = b; i < e; ++i) s += counts[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < LS_SUB_SCAN_THREADS; o <<= 1) {  // inclusive scan of the segment sums
        const u32 v = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0u;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    u32 run = threadIdx.x ? part[threadIdx.x - 1] : 0u;
    for (long long i = b; i < e; ++i) {
        const u32 c = counts[i];
        counts[i] = run;
        run += c;
    }
    if (threadIdx.x == LS_SUB_SCAN_THREADS - 1) *total = part[LS_SUB_SCAN_THREADS - 1];
}

__global__ __launch_bounds__(LS_SUB_WG) void ls_subset_write_kernel(const unsigned char* __restrict__ bm, long long off,
                                                                    long long rows, const u32* __restrict__ offs,
                                                                    u32* __restrict__ list) {
    __shared__ u32 wc[LS_SUB_WG / LS_WAVE];
    const int lane = threadIdx.x & (LS_WAVE - 1), wave = threadIdx.x / LS_WAVE;
    const long long r0 = (long long)blockIdx.x * LS_SUB_ROWS;
    u32 pos = offs[blockIdx.x];
    for (int i = 0; i < LS_SUB_ITERS; ++i) {
        const long long r = r0 + (long long)i * LS_SUB_WG + threadIdx.x;
        const bool sel = r < rows && ls_sub_bit(bm, off, r);
        const u64 mask = __ballot(sel);
        if (lane == 0) wc[wave] = (u32)__popcll(mask);
        __syncthreads();
        u32 before = 0, all = 0;
        for (int w = 0; w < LS_SUB_WG / LS_WAVE; ++w) {
            before += w < wave ? wc[w] : 0u;
            all += wc[w];
        }
        const u32 rank = __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u));
        if (sel) list[pos + before + rank] = (u32)r;
        pos += all;
        __syncthreads();
    }
}

// positions -> rows: idx[i] = list[idx[i]] + base (padding -1 stays)
__global__ __launch_bounds__(256) void ls_subset_map_kernel(long long* __restrict__ idx, long long count,
                                                            const u32* __restrict__ list, long long base) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < count) {
        const long long v = idx[i];
        if (v >= 0) idx[i] = (long long)list[v] + base;
    }
}

__global__ __launch_bounds__(256) void ls_subset_pad_kernel(float* __restrict__ s, long long* __restrict__ idx,
                                                            long long count) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < count) {
        s[i] = -FLT_MAX;
        idx[i] = -1;
    }
}

static ls_subset_state* state_of(ls_index* ix) {
    if (!ix->subsets) ix->subsets = new ls_subset_state();
    return ix->subsets;
}

static ls_subset* find_subset(ls_index* ix, int32_t id) {
    if (!ix->subsets) return nullptr;
    auto it = ix->subsets->by_id.find(id);
    return it == ix->subsets->by_id.end() ? nullptr : it->second;
}

void ls_i_subsets_free(ls_index* ix) {
    ls_subset_state* st = ix->subsets;
    if (!st) return;
    for (auto& kv : st->by_id) {
        (void)hipFree(kv.second->d_list);
        delete kv.second;
    }
    (void)hipFree(st->d_q);
    (void)hipFree(st->d_s);
    (void)hipFree(st->d_i);
    (void)hipFree(st->d_gs);
    (void)hipFree(st->d_gi);
    st->merge_tmp.release();
    if (st->h_q) (void)hipHostFree(st->h_q);
    if (st->h_s) (void)hipHostFree(st->h_s);
    if (st->h_i) (void)hipHostFree(st->h_i);
    delete st;
    ix->subsets = nullptr;
}

// ---- one single-device handle (caller holds its ls_quiesce, its device is current) -------------------------------
int ls_launch_subset_scan(u32* d_counts, int64_t nwg, u32* d_total, hipStream_t s) {
    hipLaunchKernelGGL(ls_subset_scan_kernel, dim3(1), dim3(LS_SUB_SCAN_THREADS), 0, s, d_counts, (long long)nwg, d_total);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

int ls_i_subset_compact(const uint8_t* slice, int64_t need, int64_t off, int64_t n, hipStream_t s, u32** d_list,
                        int64_t* m_out) {
    *d_list = nullptr;
    *m_out = 0;
    if (n <= 0) return LS_OK;
    const int64_t nwg = (n + LS_SUB_ROWS - 1) / LS_SUB_ROWS;
    unsigned char* d_bm = nullptr;
    u32* d_counts = nullptr;
    u32* list = nullptr;
    u32 m = 0;
    auto body = [&]() -> int {
        LS_HIP(hipMalloc((void**)&d_bm, (size_t)need));
        LS_HIP(hipMalloc((void**)&d_counts, sizeof(u32) * (size_t)(nwg + 1)));
        LS_HIP(hipMemcpyAsync(d_bm, slice, (size_t)need, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(ls_subset_count_kernel, dim3((unsigned)nwg), dim3(LS_SUB_WG), 0, s, d_bm, (long long)off,
                           (long long)n, d_counts);
        LS_HIP(hipGetLastError());
        if (int rc = ls_launch_subset_scan(d_counts, nwg, d_counts + nwg, s)) return rc;
        LS_HIP(hipMemcpyAsync(&m, d_counts + nwg, sizeof(u32), hipMemcpyDeviceToHost, s));
        LS_HIP(hipStreamSynchronize(s));
        if (m > 0) {
            LS_HIP(hipMalloc((void**)&list, sizeof(u32) * (size_t)m));
            hipLaunchKernelGGL(ls_subset_write_kernel, dim3((unsigned)nwg), dim3(LS_SUB_WG), 0, s, d_bm,
                               (long long)off, (long long)n, d_counts, list);
            LS_HIP(hipGetLastError());
            LS_HIP(hipStreamSynchronize(s));
        }
        return LS_OK;
    };
    const int rc = body();
    (void)hipFree(d_bm);
    (void)hipFree(d_counts);
    if (rc != LS_OK) {
        (void)hipFree(list);
        return rc;
    }
    *d_list = list;
    *m_out = m;
    return LS_OK;
}

// Bits [bit0, bit0 + n) of `bitmap` (nbytes bytes; missing bytes select nothing) -> ascending list of local rows.
static int subset_build(ls_index* ix, const uint8_t* bitmap, int64_t nbytes, int64_t bit0, ls_subset** out) {
    const int64_t n = ix->n;
    ls_subset* ss = new ls_subset();
    ss->n_at_create = n;
    int rc = LS_OK;
    if (n > 0) {
        // the handle's slice of the bitmap, realigned to a byte: bit (bit0 & 7) + r is local row r
        const int64_t off = bit0 & 7, byte0 = bit0 >> 3;
        const int64_t need = (off + n + 7) / 8;
        std::vector<uint8_t> slice((size_t)need, 0);
        if (byte0 < nbytes) std::copy(bitmap + byte0, bitmap + std::min(nbytes, byte0 + need), slice.begin());
        hipStream_t s = ix->own_stream;
        auto body = [&]() -> int {
            if (int r = ls_i_subset_compact(slice.data(), need, off, n, s, &ss->d_list, &ss->m)) return r;
            if (ss->m > 0) {
                ss->h_list.resize((size_t)ss->m);
                LS_HIP(hipMemcpyAsync(ss->h_list.data(), ss->d_list, sizeof(u32) * (size_t)ss->m, hipMemcpyDeviceToHost, s));
                LS_HIP(hipStreamSynchronize(s));
            }
            return LS_OK;
        };
        rc = body();
    }
    if (rc != LS_OK) {
        (void)hipFree(ss->d_list);
        delete ss;
        return rc;
    }
    *out = ss;
    return LS_OK;
}

static int32_t subset_register(ls_index* ix, ls_subset* ss) {
    ls_subset_state* st = state_of(ix);
    const int32_t id = st->next_id++;
    st->by_id[id] = ss;
    return id;
}

static int subset_check_k(int64_t m, int32_t k) {
    if (std::min<int64_t>(k, m) > LS_MAX_K) {
        ls_set_error("ls_search_subset: min(k, selected rows) = %lld exceeds LS_MAX_K = %d",
                     (long long)std::min<int64_t>(k, m), LS_MAX_K);
        return LS_ERR_K_TOO_LARGE;
    }
    return LS_OK;
}

// nq queries (fp32 [nq, d], memory the kernels can read) over subset `ss` -> d_out [nq, k] on stream s, rows as list
// positions (map = false) or mapped to list[pos] + ix->base (map = true). One scan launch and one finalize launch per
// query, in stream order - or, where ls_mq_make_plan (LS_MQ_ROWLIST) serves the call and d_q_pass (the same queries in DEVICE memory:
// every workgroup of a pass reads all of them) is given, one pass and one finalize launch per group of 2..16 queries.
static int subset_run(ls_index* ix, const ls_subset* ss, const float* d_q, int64_t nq, int32_t k, bool normalize,
                      float* d_out_s, int64_t* d_out_i, bool map, hipStream_t s, const float* d_q_pass = nullptr) {
    const int64_t m = ss->m;
    if (m == 0) {
        const long long cnt = (long long)nq * k;
        hipLaunchKernelGGL(ls_subset_pad_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, d_out_s,
                           (long long*)d_out_i, cnt);
        LS_HIP(hipGetLastError());
        return LS_OK;
    }
    const ls_geom& g = ix->g;
    const int64_t keff = std::min<int64_t>(k, m);
    const int blocks = ix->opt_blocks > 0 ? std::min(ix->opt_blocks, ix->max_blocks) : ls_scan_blocks(m, g, ix->n_cu);
    const int kprime = ls_i_pick_kprime(ix, blocks, (int)std::max<int64_t>(keff, 1));
    const ls_mq_plan mp = d_q_pass && nq >= 2 ? ls_mq_make_plan(ls_i_mq_in(ix, true), m, k, LS_MQ_NQ) : ls_mq_plan{0, 0, 0};
    // (a pass always writes its score vectors - the rescue of a query whose keys prove nothing sweeps S, so there is no
    // repair and no retry: room for 16 of them per generation, at first use)
    if (mp.keys > 0)
        if (int rc = ls_i_grow_score_vectors(ix, LS_MQ_NQ)) return rc;
    if (int rc = ls_i_flush_pending(ix)) return rc;  // (their jobs name a scratch generation)
    const int gen = (int)(ix->set_rr++ % LS_NSETS);
    ls_index::scratch_set& st = ix->sets[gen];
    if (st.last_stream && st.last_stream != s) LS_HIP(hipStreamSynchronize(st.last_stream));
    st.last_stream = s;
    for (int64_t i = 0; i < nq;) {
        // a group of 2..16 queries: one pass over the selected rows, one finalize launch with the group's jobs. (One
        // generation's candidate blocks hold LS_QUERIES_PER_LAUNCH_MAX queries at this stride, its score vectors 16.)
        // A lone query (and every query where no pass serves the call): the single-query row-list scan.
        const int group = mp.keys > 0 ? ls_mq_subset_group(nq - i) : 0;
        const int real = group ? group : 1;
        ls_scan_args a{};
        a.d_q = (group ? d_q_pass : d_q) + i * g.d;
        a.nq = real;
        a.normalize = normalize;
        a.reverse = false;
        ls_fill_scratch_args(a, ix, st, group ? mp.blocks : blocks, group ? mp.kprime : kprime);
        a.mq_keys = group ? mp.keys : 0;
        a.nfin = 0;
        if (!group) a.d_step = ix->d_sq8_step;
        a.l2 = ix->metric == LS_METRIC_L2;  // (never a group - ls_i_mq_in declines its passes)
        hipEvent_t* pe = nullptr;  // (ls_set_profiling: one event pair around the launch + its finalize, read by ls_last_kernel_ms)
        if (ix->profiling && ix->prof_n < LS_PROF_MAX) {
            if (int rc = ls_prof_events(ix->prof_ev, ix->prof_n, 2, &pe)) return rc;
            LS_HIP(hipEventRecord(pe[0], s));
        }
        if (int rc = group ? ls_launch_mq_subset(ix->d_corpus, ss->d_list, m, g, a, s)
                           : ls_launch_scan_subset(ix->d_corpus, ss->d_list, m, g, a, s))
            return rc;
        ls_fin_batch jobs;  // (rows as list positions: base 0)
        ls_fill_fin_jobs(jobs, ix, st, a.blocks, a.kprime, m, k, 0, d_out_s + i * k, d_out_i + i * k, st.d_S, real);
        if (int rc = ls_launch_finalize(jobs, s)) return rc;
        ix->n_launches_total += 2;
        if (group) ix->n_mqs_launches++;
        if (pe) {
            LS_HIP(hipEventRecord(pe[1], s));
            ix->prof_n++;
        }
        i += real;
    }
    if (map) {
        const long long cnt = (long long)nq * k;
        hipLaunchKernelGGL(ls_subset_map_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s,
                           (long long*)d_out_i, cnt, (const u32*)ss->d_list, (long long)ix->base);
        LS_HIP(hipGetLastError());
    }
    return LS_OK;
}

// ---- group handles -----------------------------------------------------------------------------------------------
static int group_subset_create(ls_index* ix, const uint8_t* bitmap, int64_t nbytes, int32_t* out_id,
                               int64_t* out_rows) {
    const int G = ls_shard_count(ix);
    const bool repl = ls_group_is_replicated(ix);
    ls_subset* gs = new ls_subset();
    gs->n_at_create = ix->n;
    int rc = LS_OK;
    for (int g = 0; g < G && rc == LS_OK; ++g) {
        ls_index* sub = ls_group_member(ix, g);
        ls_quiesce lk(sub);
        if (hipSetDevice(sub->device) != hipSuccess) {
            ls_set_error("ls_subset_create: hipSetDevice(%d) failed", sub->device);
            rc = LS_ERR_HIP;
            break;
        }
        ls_subset* ss = nullptr;
        // each shard compacts its own slice of the bitmap (its first row is generally not a multiple of 8)
        rc = subset_build(sub, bitmap, nbytes, repl ? 0 : ls_group_member_row0(ix, g), &ss);
        if (rc != LS_OK) break;
        gs->member.push_back(subset_register(sub, ss));
        if (!repl || g == 0) gs->m += ss->m;
    }
    if (rc != LS_OK) {
        for (int g = 0; g < (int)gs->member.size(); ++g) {
            ls_index* sub = ls_group_member(ix, g);
            ls_quiesce lk(sub);
            ls_subset* ss = find_subset(sub, gs->member[g]);
            (void)hipSetDevice(sub->device);
            if (ss) (void)hipFree(ss->d_list);
            sub->subsets->by_id.erase(gs->member[g]);
            delete ss;
        }
        delete gs;
        return rc;
    }
    *out_id = subset_register(ix, gs);
    if (out_rows) *out_rows = gs->m;
    return LS_OK;
}

// The synchronous single-device call (the caller holds ix's ls_quiesce): no copy commands - the kernels read the
// queries from, and the selection writes the results to, pinned host memory (as the plain host path does); positions
// are mapped to rows in the host copy of the list (at most nq * k lookups).
static int plain_search_subset(ls_index* ix, const ls_subset* ss, const float* q, int64_t nq, int32_t k, bool normalize,
                               float* out_scores, int64_t* out_indices) {
    LS_HIP(hipSetDevice(ix->device));
    ls_subset_state* st = state_of(ix);
    const size_t on = (size_t)nq * k, qn = (size_t)nq * ix->g.d;
    if (int r = ls_grow_pinned(&st->h_q, &st->hq_cap, qn)) return r;
    if (int r = ls_grow_pinned(&st->h_s, &st->hs_cap, on)) return r;
    if (int r = ls_grow_pinned(&st->h_i, &st->hi_cap, on)) return r;
    std::copy(q, q + qn, st->h_q);
    hipStream_t s = ix->own_stream;
    // (a pass's workgroups all read all of its queries: the call's queries go to device memory with one copy)
    const float* d_q_pass = nullptr;
    if (nq >= 2 && ls_mq_make_plan(ls_i_mq_in(ix, true), ss->m, k, LS_MQ_NQ).keys > 0) {
        if (int r = ls_grow(&st->d_q, &st->q_cap, qn)) return r;
        LS_HIP(hipMemcpyAsync(st->d_q, st->h_q, sizeof(float) * qn, hipMemcpyHostToDevice, s));
        d_q_pass = st->d_q;
    }
    if (int r = subset_run(ix, ss, st->h_q, nq, k, normalize, st->h_s, st->h_i, false, s, d_q_pass)) return r;
    LS_HIP(hipStreamSynchronize(s));
    const u32* list = ss->h_list.data();
    const int64_t base = ix->base;
    if (ix->metric == LS_METRIC_L2) std::transform(st->h_s, st->h_s + on, out_scores, ls_l2_out);  // (distances out)
    else std::copy(st->h_s, st->h_s + on, out_scores);
    for (size_t j = 0; j < on; ++j) {
        const int64_t p = st->h_i[j];
        out_indices[j] = p >= 0 ? (int64_t)list[p] + base : -1;
    }
    return LS_OK;
}

// Group handles (the caller holds the group's ls_quiesce). Replicated: the calls are dealt round-robin to the replicas,
// each of which holds the subset. Sharded: every shard's work is queued first - its local top-k over its slice of the
// subset, mapped to global rows ON the shard, copied to the primary device - so the shards run concurrently; then the
// G lists are merged by the sharded search's own merge (ls_i_merge_rounds: rounds of merges when G * k keys exceed one
// launch).
static int group_search_subset(ls_index* ix, ls_subset* gs, const float* q, int64_t nq, int32_t k, bool normalize,
                               float* out_s, int64_t* out_i) {
    const int G = ls_shard_count(ix);
    ls_subset_state* st = state_of(ix);
    if (ls_group_is_replicated(ix)) {
        const int r = (int)(st->rr++ % (uint32_t)G);
        ls_index* sub = ls_group_member(ix, r);
        ls_quiesce lk(sub);
        const ls_subset* ss = find_subset(sub, gs->member[r]);
        if (!ss) {
            ls_set_error("ls_search_subset: replica %d lost its subset", r);
            return LS_ERR_INVALID_ARG;
        }
        return plain_search_subset(sub, ss, q, nq, k, normalize, out_s, out_i);
    }
    const size_t on = (size_t)nq * k;
    ls_index* prim = ls_group_member(ix, 0);
    LS_HIP(hipSetDevice(prim->device));
    if (int rc = ls_grow(&st->d_gs, &st->gs_cap, on * G)) return rc;
    if (int rc = ls_grow(&st->d_gi, &st->gi_cap, on * G)) return rc;
    std::vector<std::unique_ptr<ls_quiesce>> held;  // every shard, in shard order, for the whole call
    for (int g = 0; g < G; ++g) held.emplace_back(new ls_quiesce(ls_group_member(ix, g)));
    for (int g = 0; g < G; ++g) {
        ls_index* sub = ls_group_member(ix, g);
        LS_HIP(hipSetDevice(sub->device));
        ls_subset_state* ss_st = state_of(sub);
        const ls_subset* ss = find_subset(sub, gs->member[g]);
        if (!ss) {
            ls_set_error("ls_search_subset: shard %d lost its subset", g);
            return LS_ERR_INVALID_ARG;
        }
        if (int rc = ls_grow(&ss_st->d_q, &ss_st->q_cap, (size_t)nq * ix->g.d)) return rc;
        if (int rc = ls_grow(&ss_st->d_s, &ss_st->s_cap, on)) return rc;
        if (int rc = ls_grow(&ss_st->d_i, &ss_st->i_cap, on)) return rc;
        hipStream_t s = sub->own_stream;
        LS_HIP(hipMemcpyAsync(ss_st->d_q, q, sizeof(float) * (size_t)nq * ix->g.d, hipMemcpyHostToDevice, s));
        if (int rc = subset_run(sub, ss, ss_st->d_q, nq, k, normalize, ss_st->d_s, ss_st->d_i, true, s)) return rc;
        float* dst_s = st->d_gs + (size_t)g * on;
        int64_t* dst_i = st->d_gi + (size_t)g * on;
        if (sub->device == prim->device) {
            LS_HIP(hipMemcpyAsync(dst_s, ss_st->d_s, sizeof(float) * on, hipMemcpyDeviceToDevice, s));
            LS_HIP(hipMemcpyAsync(dst_i, ss_st->d_i, sizeof(int64_t) * on, hipMemcpyDeviceToDevice, s));
        } else {
            LS_HIP(hipMemcpyPeerAsync(dst_s, prim->device, ss_st->d_s, sub->device, sizeof(float) * on, s));
            LS_HIP(hipMemcpyPeerAsync(dst_i, prim->device, ss_st->d_i, sub->device, sizeof(int64_t) * on, s));
        }
    }
    for (int g = 0; g < G; ++g) {
        ls_index* sub = ls_group_member(ix, g);
        LS_HIP(hipSetDevice(sub->device));
        LS_HIP(hipStreamSynchronize(sub->own_stream));
    }
    LS_HIP(hipSetDevice(prim->device));
    hipStream_t ps = prim->own_stream;
    if (int rc = ls_grow_pinned(&st->h_s, &st->hs_cap, on)) return rc;
    if (int rc = ls_grow_pinned(&st->h_i, &st->hi_cap, on)) return rc;
    if (int rc = ls_i_merge_rounds(st->d_gs, st->d_gi, (int64_t)(on * sizeof(float)), (int64_t)(on * sizeof(int64_t)), G,
                                   nq, k, st->h_s, st->h_i, st->merge_tmp, ps))
        return rc;
    LS_HIP(hipStreamSynchronize(ps));
    std::copy(st->h_s, st->h_s + on, out_s);
    std::copy(st->h_i, st->h_i + on, out_i);
    return LS_OK;
}

extern "C" {

int ls_subset_create(ls_index* ix, const uint8_t* bitmap, int64_t nbytes, int32_t* out_id, int64_t* out_rows) {
    if (!ix || !out_id || nbytes < 0 || (nbytes > 0 && !bitmap)) {
        ls_set_error("ls_subset_create: bad argument");
        return LS_ERR_INVALID_ARG;
    }
    if (int rc = ls_i_check_device(ix->device)) return rc;
    ls_quiesce lk(ix);
    ls_device_guard guard;
    int rc;
    if (ix->group) {
        rc = group_subset_create(ix, bitmap, nbytes, out_id, out_rows);
    } else {
        LS_HIP(hipSetDevice(ix->device));
        ls_subset* ss = nullptr;
        rc = subset_build(ix, bitmap, nbytes, 0, &ss);
        if (rc == LS_OK) {
            *out_id = subset_register(ix, ss);
            if (out_rows) *out_rows = ss->m;
        }
    }
    return rc;
}

int ls_subset_destroy(ls_index* ix, int32_t id) {
    if (!ix) {
        ls_set_error("ls_subset_destroy: index is null");
        return LS_ERR_INVALID_ARG;
    }
    ls_quiesce lk(ix);
    ls_subset* ss = find_subset(ix, id);
    if (!ss) {
        ls_set_error("ls_subset_destroy: no subset %d on this handle", id);
        return LS_ERR_INVALID_ARG;
    }
    ix->subsets->by_id.erase(id);
    ls_device_guard guard;
    if (ix->group) {
        for (int g = 0; g < (int)ss->member.size(); ++g) {
            ls_index* sub = ls_group_member(ix, g);
            ls_quiesce lks(sub);
            ls_subset* ms = find_subset(sub, ss->member[g]);
            if (!ms) continue;
            sub->subsets->by_id.erase(ss->member[g]);
            (void)hipSetDevice(sub->device);
            (void)hipFree(ms->d_list);
            delete ms;
        }
    } else {
        (void)hipSetDevice(ix->device);
        (void)hipFree(ss->d_list);
    }
    delete ss;
    return LS_OK;
}

int ls_search_subset(ls_index* ix, int32_t subset, const float* q, int64_t nq, int32_t k, uint32_t flags,
                     float* out_scores, int64_t* out_indices) {
    if (!ix || nq < 1 || k <= 0 || k > (1 << 20) || !q || !out_scores || !out_indices) {
        ls_set_error("ls_search_subset: bad argument (nq=%lld k=%d)", (long long)nq, k);
        return LS_ERR_INVALID_ARG;
    }
    if (flags & ~LS_FLAG_NORMALIZE) {
        ls_set_error("ls_search_subset: unsupported flags 0x%x (only LS_FLAG_NORMALIZE)", flags);
        return LS_ERR_INVALID_ARG;
    }
    if (int rc = ls_i_check_device(ix->device)) return rc;
    const bool normalize = (flags & LS_FLAG_NORMALIZE) != 0;
    // a subset call is never folded into the plain callers' batches: it waits until no synchronous host call is in
    // flight and takes the handle (as ls_add or ls_set_base do); plain callers pay nothing when none happens
    ls_quiesce lk(ix);
    ls_subset* ss = find_subset(ix, subset);
    if (!ss) {
        ls_set_error("ls_search_subset: no subset %d on this handle", subset);
        return LS_ERR_INVALID_ARG;
    }
    if (int rc = subset_check_k(ss->m, k)) return rc;
    ls_device_guard guard;
    if (ix->group) return group_search_subset(ix, ss, q, nq, k, normalize, out_scores, out_indices);
    return plain_search_subset(ix, ss, q, nq, k, normalize, out_scores, out_indices);
}

}  // extern "C"
