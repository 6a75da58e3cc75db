// ls_ivf_assign_kernel.h — the body of the IVF assignment kernels (ls_ivf_build.hip has the description): rows x
// centroids -> the list of every row, as a device function template that the two kernels wrap. ls_ivf_build.hip
// instantiates ls_ivf_assign_kernel<L, V, U> (L2 = false: the inner product, QueryRegs), ls_l2_ivf.hip
// ls_ivf_assign_l2_kernel<L, V, U> (L2 = true; include/leansearch_ivf_l2.h): the tile's rows sit in
// QueryL2<false, V> registers and the score of (row, centroid) is -group_sum<L>(rq[u].dot(centroid chunks)), with
// t = centroid_i - row_i - the row plays the query's role, so the bits are those of ls_search(ls_create_l2 index of the
// centroids, row, k = 1). Tile plan, centroid double-buffering, key and argmax are shared.
#pragma once
#include "ls_index.h"
#include "ls_scan_dev.h"
#include "ls_ivf_build_plan.h"

template <int L, int V, int U, bool L2>
__device__ __forceinline__ void ls_ivf_assign_body(const f32x4* __restrict__ rows, long long n,
                                                   const f32x4* __restrict__ cent, int nlist, int* __restrict__ assign) {
    constexpr int R = LS_WAVE / L;  // rows per wave load step
    constexpr int TR = U * R;       // rows per tile
    constexpr int CH = L * V;       // chunks per stored row
    constexpr int CB = ls_ivfb_cent_batch(V);
    const int lane = threadIdx.x & (LS_WAVE - 1);
    const int wave = threadIdx.x / LS_WAVE;
    const int sub = lane & (L - 1);
    const int grp = lane / L;
    const long long W = (long long)gridDim.x * LS_SCAN_WAVES;
    const long long gw = (long long)blockIdx.x * LS_SCAN_WAVES + wave;
    const long long NT = (n + TR - 1) / TR;
    const int NB = ls_ivfb_cent_batches(nlist, CB);

    for (long long step = 0;; ++step) {
        const long long t = ls_ivfb_tile(W, gw, step);  // (wave-uniform)
        if (t >= NT) break;
        scan_query_t<false, V, false, L2> rq[U];  // the tile: row u of this lane's group, chunks sub, sub + L, ..
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long r = ls_ivfb_row_load(ls_ivfb_row(t, TR, R, u, grp), n);
            const f32x4* p = rows + r * CH + sub;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const f32x4 x = __builtin_nontemporal_load(p + L * v);
                rq[u].q[v] = make_float4(x.x, x.y, x.z, x.w);
            }
        }
        u64 best[U];
#pragma unroll
        for (int u = 0; u < U; ++u) best[u] = 0ull;

        auto load = [&](f32x4 (&buf)[CB][V], int b) {
#pragma unroll
            for (int j = 0; j < CB; ++j) {
                const f32x4* p = cent + (long long)ls_ivfb_cent_load(ls_ivfb_cent(b, CB, j), nlist) * CH + sub;
#pragma unroll
                for (int v = 0; v < V; ++v) buf[j][v] = p[L * v];
            }
        };
        auto score = [&](const f32x4 (&buf)[CB][V], int b) {
#pragma unroll
            for (int j = 0; j < CB; ++j) {
                const int c = ls_ivfb_cent(b, CB, j);
                if (!ls_ivfb_cent_valid(c, nlist)) break;  // (uniform: the whole wave is in group_sum's DPP steps)
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const float gs = group_sum<L>(rq[u].dot(buf[j]));
                    const float s = L2 ? -gs : gs;  // (L2: the score is the negated distance)
                    const u64 key = ls_make_key(s, (u32)c);
                    best[u] = key > best[u] ? key : best[u];
                }
            }
        };
        f32x4 b0[CB][V], b1[CB][V];
        load(b0, 0);
        for (int b = 0; b < NB; b += 2) {  // two batches per trip: one is scored while the other one's loads fly
            if (b + 1 < NB) load(b1, b + 1);
            score(b0, b);
            if (b + 1 < NB) {
                if (b + 2 < NB) load(b0, b + 2);
                score(b1, b + 1);
            }
        }
        if (sub == 0) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long r = ls_ivfb_row(t, TR, R, u, grp);
                if (ls_ivfb_row_valid(r, n)) assign[r] = best[u] ? (int)(0xffffffffu - (u32)best[u]) : 0;
            }
        }
    }
}

// the L2 form's launcher (ls_l2_ivf.hip); the arguments are ivfb_launch_assign's of ls_ivf_build.hip
int ls_ivf_launch_assign_l2(const ls_geom& g, const void* d_rows, int64_t n, const void* d_cent, int32_t nlist,
                            int32_t* d_assign, int32_t n_cu, hipStream_t s);
