// ls_ivf_kernel.h — the probed-list scan kernel of ls_ivf.hip (see there) as a template in a header: ls_ivf.hip
// instantiates the f32 / fp16 kernels, ls_sq8_ivf.hip the sq8 ones (a trailing ls_sq8_arg argument selects QuerySq8,
// as in ls_scan_kernel.h).
// Tail: empty, or `const u32*` (then, optionally, the ls_sq8_arg) - the row-list form that serves an IVF subset
// (include/leansearch_ivf_subset.h; instantiated by ls_ivf_subset.hip / ls_sq8_ivf_subset.hip). `off` is then the
// subset's soff (offsets of the lists in the compacted arrays), so the prefix counts SELECTED rows per probed list
// and a position resolves to an index x of the compacted arrays: the storage row is srows[x] (the trailing list) and
// the original row is ids[x] (the subset's sid) - two independent loads where the plain form has the one ids[srow].
// The instantiations without a list are the plain probed-list scan, unchanged.
// An ls_l2_arg at the end of the pack (after the list, if any; ls_l2_ivf.hip): the query registers are QueryL2 and a
// row's score is its negated squared distance, negated once behind group_sum, as in ls_scan_kernel.h.
// An ls_bf16_arg at the end of the pack (after the list, if any; ls_bf16_ivf.hip): bfloat16 rows, QueryBf16.
#pragma once
#include "ls_index.h"
#include "ls_scan_dev.h"

#define LS_IVF_MAX_PROBE LS_MAX_K  // probed lists per query (the coarse search's k)
// ---- fine stage ---------------------------------------------------------------------------------------------------
template <bool F16, int L, int V, int U, typename... Tail>
__global__ __launch_bounds__(LS_SCAN_THREADS) void ls_ivf_scan_kernel(
    const f32x4* __restrict__ corpus, int chunks, const u32* __restrict__ ids, const u32* __restrict__ off,
    const long long* __restrict__ probe, int nprobe, const float* __restrict__ qraw, int d, int normalize,
    float* __restrict__ S, u64* __restrict__ cand, u64* __restrict__ bound, int kprime, Tail... tail) {
    constexpr int R = LS_WAVE / L;  // rows per wave load step
    constexpr int TR = U * R;       // positions per tile
    static_assert(TR <= LS_WAVE, "a tile's scores must fit one per lane");
    constexpr bool SQ8 = ls_pack_sq8<Tail...>::value;
    constexpr bool L2 = ls_pack_l2<Tail...>::value;
    static_assert(!L2 || !SQ8, "an L2 launch scans f32 or fp16 rows");
    constexpr bool BF16 = ls_pack_bf16<Tail...>::value;
    static_assert(!BF16 || (!SQ8 && !L2 && !F16), "a bf16 launch serves the inner product");
    constexpr bool IDX = sizeof...(Tail) == (SQ8 || L2 || BF16 ? 2 : 1);  // a row list leads the pack
    __shared__ u32 pre[LS_IVF_MAX_PROBE + 1];  // pre[j]: rows of the probed lists before the j-th
    __shared__ u32 lrow[LS_IVF_MAX_PROBE];     // first storage row of the j-th probed list
    __shared__ u32 part[LS_SCAN_THREADS];
    __shared__ u64 sm[LS_SCAN_WAVES * LS_KP_MAX];
    const int tid = threadIdx.x;
    const int lane = tid & (LS_WAVE - 1);
    const int wave = tid / LS_WAVE;
    const int sub = lane & (L - 1);
    const int grp = lane / L;
    const int kp = kprime + 1;

    // ---- prefix sums of the probed lists' sizes (a probe entry of -1: the coarse search had fewer valid centroids)
    {
        const int per = (nprobe + LS_SCAN_THREADS - 1) / LS_SCAN_THREADS;
        const int j0 = tid * per, j1 = min(j0 + per, nprobe);
        u32 run = 0;
        for (int j = j0; j < j1; ++j) {
            const long long l = probe[j];
            u32 b = 0, e = 0;
            if (l >= 0) {
                b = off[l];
                e = off[l + 1];
            }
            lrow[j] = b;
            pre[j] = run;
            run += e - b;
        }
        part[tid] = run;
        __syncthreads();
        for (int o = 1; o < LS_SCAN_THREADS; o <<= 1) {
            const u32 v = tid >= o ? part[tid - o] : 0u;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        const u32 before = tid ? part[tid - 1] : 0u;
        for (int j = j0; j < j1; ++j) pre[j] += before;
        if (tid == LS_SCAN_THREADS - 1) pre[nprobe] = part[LS_SCAN_THREADS - 1];
        __syncthreads();
    }
    const long long M = pre[nprobe];
    const long long W = (long long)gridDim.x * LS_SCAN_WAVES;
    const long long gw = (long long)blockIdx.x * LS_SCAN_WAVES + wave;
    const long long NT = (M + TR - 1) / TR;
    const int top = 1 << (31 - __clz(nprobe));  // largest power of two <= nprobe

    // lane i: storage row and original row of position i of tile t (positions past M repeat the last one, masked)
    auto fetch = [&](long long t, u32& srow, u32& id) {
        if (t >= NT) return;
        long long p = t * TR + (lane < TR ? lane : TR - 1);
        p = p < M ? p : M - 1;
        int lo = 0;  // the largest j with pre[j] <= p (empty lists share their successor's prefix and lose)
        for (int w = top; w > 0; w >>= 1) {
            const int m = lo + w;
            if (m < nprobe && (long long)pre[m] <= p) lo = m;
        }
        srow = lrow[lo] + (u32)(p - pre[lo]);
        if constexpr (IDX) {  // that is an index of the subset's compacted arrays: two independent loads
            const u32* __restrict__ srows = [](const u32* l, auto...) { return l; }(tail...);
            const u32 x = srow;
            srow = srows[x];
            id = ids[x];
        } else {
            id = ids[srow];
        }
    };
    f32x4 xb[U][V];
    auto issue_loads = [&](u32 srow) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long r = (u32)__shfl((int)srow, u * R + grp, LS_WAVE);
            const f32x4* p = corpus + r * chunks + sub;
#pragma unroll
            for (int v = 0; v < V; ++v) xb[u][v] = __builtin_nontemporal_load(p + L * v);
        }
    };
    long long t = gw;
    u32 srow_n = 0, id_n = 0, id_c = 0;
    fetch(t, srow_n, id_n);
    if (t < NT) {  // the first tile's loads fly while the query is prepared
        issue_loads(srow_n);
        id_c = id_n;
        fetch(t + W, srow_n, id_n);
    }

    scan_query_t<F16, V, SQ8, L2, BF16> qr;
    {
        (void)qr.load(qraw, d, sub, L);
        float inv = 1.0f;
        if (normalize) {  // the library's canonical summation order (ls_common.h)
            const float ss = ls_wave_sumsq(qraw, d, lane);
            if (ss > 0.0f) inv = 1.0f / sqrtf(ss);
        }
        qr.scale(inv);
        if constexpr (SQ8) qr.apply_step(ls_pack_step(tail...), d, sub, L);
    }

    u64 lst = 0;  // lanes 0..kp-1: this wave's best keys, descending
    u64 thr = 0;  // key in lane kp-1 (wave-uniform)
    while (t < NT) {
        float sc = 0.0f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float gs = group_sum<L>(qr.dot(xb[u]));  // valid in all L lanes of a group
            const float s = L2 ? -gs : gs;                 // (L2: the score is the negated distance)
            const float sel = pick_group<L>(s, lane);     // lane i <- group (i % R)
            if (lane / R == u) sc = sel;
        }
        const long long pos = t * TR + lane;
        const u32 myid = id_c;
        t += W;
        if (t < NT) {  // overlaps the selection below
            issue_loads(srow_n);
            id_c = id_n;
            fetch(t + W, srow_n, id_n);
        }
        const bool valid = lane < TR && pos < M;
        if (valid && S) S[myid] = sc;  // (second launch only: the original-row-indexed score vector)
        const u64 key = valid ? ls_make_key(sc, myid) : 0ull;
        u64 mask = __ballot(key > thr);
        while (mask) {  // rare once the threshold has warmed up
            const int j = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const u64 v = readlane64(key, j);
            wave_insert(lst, v, lane, kp);
            thr = readlane64(lst, kp - 1);
        }
    }

    // merge the 4 wave lists -> this workgroup's best kprime keys + bound (as the scan kernel does)
    if (lane < LS_KP_MAX) sm[wave * LS_KP_MAX + lane] = (lane < kp) ? lst : 0ull;
    __syncthreads();
    if (wave == 0) {
        const u64 mine = sm[lane];  // LS_SCAN_WAVES * LS_KP_MAX == 64 slots
        int rank = 0;
        for (int w = 0; w < LS_SCAN_WAVES; ++w)
            for (int j = 0; j < kp; ++j) {
                const int i = w * LS_KP_MAX + j;
                const u64 o = sm[i];
                rank += (o > mine) || (o == mine && i < lane);
            }
        if (rank < kprime) cand[(long long)blockIdx.x * kprime + rank] = mine;
        if (rank == kprime) bound[blockIdx.x] = mine;
    }
}

struct ivf_launch {
    const void* corpus;
    const u32 *ids, *off;  // (a subset launch: the subset's sid and soff)
    const long long* probe;
    int nprobe;
    const float* q;
    bool normalize;
    float* S;
    u64 *cand, *bound;
    int blocks, kprime;
    const float* step;  // sq8 rows only
    const u32* srow;    // subset launches only: storage row of every compacted position
    bool l2;            // L2 handle (ls_ivf::metric): ivf_launch_scan hands over to ls_l2_ivf.hip
};
int ls_ivf_launch_scan_sq8(const ls_geom& g, const ivf_launch& a, hipStream_t s);         // (ls_sq8_ivf.hip)
int ls_ivf_launch_scan_subset(const ls_geom& g, const ivf_launch& a, hipStream_t s);      // (ls_ivf_subset.hip)
int ls_ivf_launch_scan_l2(const ls_geom& g, const ivf_launch& a, hipStream_t s);          // (ls_l2_ivf.hip: both forms)
int ls_ivf_launch_scan_subset_sq8(const ls_geom& g, const ivf_launch& a, hipStream_t s);  // (ls_sq8_ivf_subset.hip)
int ls_ivf_launch_scan_bf16(const ls_geom& g, const ivf_launch& a, hipStream_t s);        // (ls_bf16_ivf.hip: both forms)
