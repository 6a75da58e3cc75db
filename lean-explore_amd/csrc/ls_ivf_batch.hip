// ls_ivf_batch.hip — IVF search, small batches on fp32 rows (opt-in: ls_ivf_set_small_batch): 2..16 queries of a call
// share ONE pass over the union of the lists they probe, with the inner products on the f32 matrix cores and
// BIT-IDENTICAL to each query's own probed-list scan (ls_ivf.hip).
//
// Replaces faiss `index.search(X, k)` on `IndexIVFFlat(IndexFlatIP(d), d, nlist, METRIC_INNER_PRODUCT)` with
// `index.nprobe = 64` and more than one row in X (the reference's own call is src/lean_explore/search/engine.py:238-250
// with one query), which ls_ivf_search served with one chain per query - centroid search, probed-list scan, selection:
// every probed row was read once per query that probes it.
//
// Roofline: HBM over the union. One pass reads M * d * 4 bytes of rows and 10 bytes per position of (storage row,
// original row, query mask) once, for up to 16 queries - at nlist 447 / nprobe 64, 16 queries probe most of the index
// between them, so the pass is one corpus read where the chains were 16 x 64 / 447 of one each; the matrix work is
// ls_mq.hip's (M * d / 64 v_mfma_f32_16x16x4_f32 of 32 cycles: a third of the HBM time at every row length). Small
// unions are bound by the launch floors of the group (its centroid search + four launches) instead. Measured
// (tools/ivf_small_batch_time.py; 200 k rows, nlist 447, nprobe 64, 16 queries; union step + pass +
// the group's selection launch): 83.8 us at d = 384 over 191 541 rows (41.5 us of bytes at 7.09 TB/s; the 16 chains'
// first launches: 409.7 us), 173.6 us at d = 1024, k = 1000 over 189 395 rows (109.4 us of bytes; 778.8 us).
//
// Two steps here, between the group's centroid search and its selection launch (ls_ivf.hip):
//   union  ls_ivf_union_lists_kernel (one workgroup): from the group's probe lists d_pi[g][nprobe] a 16-bit mask per list
//          (bit q: query q of the group probes it) by LDS atomics, then the prefix sums of the sizes of the lists with a
//          non-zero mask - the union in ascending list number, storage order inside a list - and its size M, which stays
//          on the device. ls_ivf_union_rows_kernel (one workgroup per list) then materialises three flat arrays per union
//          position: storage row, original row (ids[storage row]) and the list's mask - 10 bytes beside a 256-4096-byte
//          row - and fills them up to the next multiple of 16 positions with mask 0.
//   pass   ls_mq_kernel (ls_mq_kernel.h) with the union as its row source: one B block, four waves, the eight fp32 row
//          geometries x 3 / 5 / 8 keys per lane; no score vectors, no granules, no riding jobs. The lane transpose, the
//          chain and group order, the add tree, the list merge, the rank-and-emit and the query staging are the plain
//          pass's text, so a score is the scan kernel's bits; a row enters only the lists of the queries whose mask bit
//          is set, and the keys carry the ORIGINAL row, compared as (score, then original row ascending) while the tiles
//          stream (ls_mq_dev.h, mq_take_scores_union), as the probed-list scan's keys do.
//
// Its own translation unit: the kernels of ls_mq.hip and ls_mq_subset.hip keep their code.
#include "ls_mq_kernel.h"

#ifndef LS_IVFB_KERNEL_ONLY  // (scratch builds that instantiate a kernel or two and look at their resources / ISA)
#include "ls_mq_launch.h"

#define LS_IVFB_LIST_THREADS 1024
#define LS_IVFB_ROW_THREADS 256

// probe: [g][np] list numbers of the group's queries (-1: the centroid search had fewer valid centroids).
// -> lmask[nlist], lpre[nlist + 1] (positions of the union before every list), *m = *h_m = the union's size.
__global__ __launch_bounds__(LS_IVFB_LIST_THREADS) void ls_ivf_union_lists_kernel(
    const long long* __restrict__ probe, int g, int np, const u32* __restrict__ off, int nlist, u32* __restrict__ lmask,
    u32* __restrict__ lpre, u32* __restrict__ m, u32* __restrict__ h_m) {
    __shared__ u32 msk[LS_IVF_BATCH_MAX_NLIST];
    __shared__ u32 part[LS_IVFB_LIST_THREADS];
    const int tid = threadIdx.x;
    for (int l = tid; l < nlist; l += LS_IVFB_LIST_THREADS) msk[l] = 0u;
    __syncthreads();
    for (int i = tid; i < g * np; i += LS_IVFB_LIST_THREADS) {
        const long long l = probe[i];
        if (l >= 0 && l < nlist) atomicOr(&msk[l], 1u << (i / np));
    }
    __syncthreads();
    // thread t owns a contiguous segment of the lists (as ls_subset_scan_kernel does)
    const int per = (nlist + LS_IVFB_LIST_THREADS - 1) / LS_IVFB_LIST_THREADS;
    const int j0 = min(tid * per, nlist), j1 = min(j0 + per, nlist);
    u32 run = 0;
    for (int j = j0; j < j1; ++j) run += msk[j] ? off[j + 1] - off[j] : 0u;
    part[tid] = run;
    __syncthreads();
    for (int o = 1; o < LS_IVFB_LIST_THREADS; o <<= 1) {  // inclusive scan of the segment sums
        const u32 v = tid >= o ? part[tid - o] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    run = tid ? part[tid - 1] : 0u;
    for (int j = j0; j < j1; ++j) {
        lpre[j] = run;
        lmask[j] = msk[j];
        run += msk[j] ? off[j + 1] - off[j] : 0u;
    }
    if (tid == LS_IVFB_LIST_THREADS - 1) {
        const u32 total = part[LS_IVFB_LIST_THREADS - 1];
        lpre[nlist] = total;
        *m = total;
        if (h_m) __hip_atomic_store(h_m, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// workgroup l: the positions of list l, if the group probes it. Workgroup 0 also fills the last tile (mask 0: no query;
// an empty union gets one such tile, so that position 0 names a row of the corpus). cap: entries the arrays hold.
__global__ __launch_bounds__(LS_IVFB_ROW_THREADS) void ls_ivf_union_rows_kernel(
    const u32* __restrict__ lmask, const u32* __restrict__ lpre, const u32* __restrict__ off, const u32* __restrict__ ids,
    int nlist, u32* __restrict__ urow, u32* __restrict__ uid, unsigned short* __restrict__ umask, long long cap) {
    const int l = blockIdx.x, tid = threadIdx.x;
    if (l == 0) {
        const long long total = lpre[nlist];
        const long long end = total > 0 ? (total + 15) / 16 * 16 : 16;
        for (long long p = total + tid; p < end && p < cap; p += LS_IVFB_ROW_THREADS) {
            urow[p] = 0u;
            uid[p] = 0u;
            umask[p] = 0;
        }
    }
    const u32 mk = lmask[l];
    if (!mk) return;
    const u32 b = off[l], cnt = off[l + 1] - b;
    const long long p0 = lpre[l];
    for (u32 j = tid; j < cnt; j += LS_IVFB_ROW_THREADS) {
        const long long p = p0 + j;
        if (p >= cap) break;  // (never: the union holds at most the index's rows)
        urow[p] = b + j;
        uid[p] = ids[b + j];
        umask[p] = (unsigned short)mk;
    }
}

int ls_ivf_launch_union(const long long* d_probe, int g, int np, const u32* d_off, const u32* d_ids, int nlist,
                        const ls_ivf_union& u, u32* h_m, hipStream_t s) {
    if (!d_probe || g < 1 || g > LS_MQ_NQ || np < 1 || nlist < 1 || nlist > LS_IVF_BATCH_MAX_NLIST || !d_off || !d_ids ||
        !u.lmask || !u.lpre || !u.row || !u.id || !u.mask || !u.m || u.cap < 16) {
        ls_set_error("ls_ivf_launch_union: bad arguments (group %d nprobe %d nlist %d)", g, np, nlist);
        return LS_ERR_INVALID_ARG;
    }
    hipLaunchKernelGGL(ls_ivf_union_lists_kernel, dim3(1), dim3(LS_IVFB_LIST_THREADS), 0, s, d_probe, g, np, d_off, nlist,
                       u.lmask, u.lpre, u.m, h_m);
    LS_HIP(hipGetLastError());
    hipLaunchKernelGGL(ls_ivf_union_rows_kernel, dim3((unsigned)nlist), dim3(LS_IVFB_ROW_THREADS), 0, s,
                       (const u32*)u.lmask, (const u32*)u.lpre, d_off, d_ids, nlist, u.row, u.id, u.mask, (long long)u.cap);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// a.nq = the group's real query count (2..16); bound = the host's bound of the union (it plans a.blocks / a.kprime /
// a.mq_keys: ls_mq_ivf_plan); no score vectors (a.d_S null), no riding selection jobs, no granules.
int ls_launch_mq_ivf_union(const void* d_corpus, const ls_ivf_union& u, int64_t bound, const ls_geom& g,
                           const ls_scan_args& a, hipStream_t s) {
    if (!ls_mq_args_ok(g, a, 4, LS_MQ_NQ, LS_MQ_WAVES) || !d_corpus || !u.row || !u.id || !u.mask || !u.m || !a.d_q ||
        a.d_S || !a.d_cand || !a.d_bound || a.nfin != 0 || a.d_gran || bound < 1 || bound > u.cap - 16) {
        ls_set_error("ls_launch_mq_ivf_union: bad arguments (elem %d nq %d bound %lld blocks %d kprime %d keys %d)", g.elem,
                     a.nq, (long long)bound, a.blocks, a.kprime, a.mq_keys);
        return LS_ERR_INVALID_ARG;
    }
    ls_scan_args b{};  // (no jobs, no granules, no tag, no kept queries, no score vectors: the other arguments are zeros)
    b.d_q = a.d_q, b.nq = a.nq, b.normalize = a.normalize;
    b.d_cand = a.d_cand, b.c_stride = a.c_stride, b.d_bound = a.d_bound, b.b_stride = a.b_stride;
    b.blocks = a.blocks, b.kprime = a.kprime, b.mq_keys = a.mq_keys;
    const mq_union_src src{u.row, u.id, u.mask, u.m};
    return ls_geom_dispatch<false, true>("ls_launch_mq_ivf_union", g, [&](auto l, auto v) {
        return ls_mq_dispatch<false>(b, [&](auto mk, auto) {
            constexpr int L = decltype(l)::value, V = decltype(v)::value, M = decltype(mk)::value;
            return ls_mq_launch<ls_mq_kernel<L, V, M, 1, LS_MQ_WAVES, mq_union_src>>(
                "ls_launch_mq_ivf_union", LS_MQ_WAVES, mq_lds_bytes(g.chunks, M, 1, LS_MQ_WAVES), LS_PIGGY_LDS_MAX,
                (const mq_f32x4*)d_corpus, bound, g, b, s, src);
        });
    });
}
#else
#ifndef LS_IVFB_ONLY_L
#define LS_IVFB_ONLY_L 16
#endif
#ifndef LS_IVFB_ONLY_V
#define LS_IVFB_ONLY_V 3
#endif
template __global__ void ls_mq_kernel<LS_IVFB_ONLY_L, LS_IVFB_ONLY_V, 3, 1, LS_MQ_WAVES, mq_union_src>(
    const mq_f32x4*, long long, const float*, int, int, int, float*, long long, u64*, long long, u64*, long long, int, int,
    ls_fin_batch, void*, long long, u32, float*, mq_union_src);
template __global__ void ls_mq_kernel<LS_IVFB_ONLY_L, LS_IVFB_ONLY_V, 8, 1, LS_MQ_WAVES, mq_union_src>(
    const mq_f32x4*, long long, const float*, int, int, int, float*, long long, u64*, long long, u64*, long long, int, int,
    ls_fin_batch, void*, long long, u32, float*, mq_union_src);
#endif  // LS_IVFB_KERNEL_ONLY
