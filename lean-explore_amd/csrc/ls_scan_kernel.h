// ls_scan_kernel.h — the scan kernel template (see ls_scan.hip for the work decomposition). A header so that the
// sq8 instantiations (ls_sq8_scan.hip) compile in their own translation unit; ls_scan.hip instantiates the f32 / fp16
// kernels from the same text.
#pragma once
#include "ls_scan_dev.h"

// Waves per SIMD the register allocation must leave room for. The 8-query fp16 kernel of 3-chunk
// lanes (d = 384 fp16) would take 271 VGPRs, i.e. ONE wave per SIMD; held to 256 it spills 19
// registers outside the tile loop and runs two. (4-chunk lanes at 8 queries would spill 80-180:
// they stay at one wave.)
__host__ __device__ constexpr int scan_min_waves(bool f16, int V, int NQ) {
    return (f16 && V == 3 && NQ == 8) ? 2 : 1;
}
// (sq8: two waves per SIMD, i.e. at most 256 VGPRs and no AGPR copies. Left at one, the scheduler converts a whole
// tile's codes to f32 ahead of the fmaf chains and takes 300-500 registers for it.)
template <typename... X>
__host__ __device__ constexpr int scan_min_waves_for(bool f16, int V, int NQ) {
    return ls_pack_sq8<X...>::value ? 2 : scan_min_waves(f16, V, NQ);
}

// SMALL: a wave sees at most 64 rows in the whole launch (small shards: a few tiles per wave).
// The running sorted list is then the wrong tool - nearly every row of a wave's first tiles
// enters it, one serial insert (~0.2 us) per row: 3.5 of the 10.3 us of a scan-only launch at
// N = 10 k - so the wave parks tile i's TR scores in lanes i*TR .. and ranks its <= 64 keys
// once, by counting, after the last tile.
// SMALL also keeps PF = 4 tiles in flight per wave: with a handful of tiles per wave each HBM round
// trip would otherwise be paid in sequence (1.0-1.4 us per tile of a 4-tile wave).
// RowList: empty, or `const u32*` - the subset scan (ls_subset.hip, NQ == 1 only): `n` then counts positions in an
// ascending list of selected rows and everything but the row loads (S, keys, tiles, selection) works in positions;
// a row load reads corpus + list[pos] * chunks. The list entries of the next tile a buffer loads are fetched while
// its current tile is in flight. The instantiations without a list are the plain scan, unchanged.
// An ls_sq8_arg at the end of the pack (after the list, if any; NQ == 1 only): the rows are int8 codes and the query
// registers are QuerySq8 (ls_scan_dev.h); F16 is false and unused.
// An ls_l2_arg at the end of the pack (after the list, if any): the query registers are QueryL2 and a row's score is its
// negated squared distance, negated once behind group_sum. Without a list NQ may be 4 or 8: the queries
// sit in QueryL2Pair registers, two chains per float2 operation, and a sum is negated once behind rs_step (4.11b).
// An ls_bf16_arg at the end of the pack (after the list, if any; NQ == 1 only): the rows are bfloat16 and the query
// registers are QueryBf16 (ls_scan_dev.h); F16 is false and unused.
template <bool F16, int L, int V, int U, int NQ, bool SMALL, typename... RowList>
__global__ __launch_bounds__(LS_SCAN_THREADS, scan_min_waves_for<RowList...>(F16, V, NQ)) void ls_scan_kernel(
    const f32x4* __restrict__ corpus, long long n, int chunks, const float* __restrict__ qraw,
    int d, int normalize, int reverse, float* __restrict__ S, long long s_stride,
    u64* __restrict__ cand, long long c_stride, u64* __restrict__ bound, long long b_stride,
    int kprime, int nfin, ls_fin_batch fin, void* __restrict__ gran, long long g_stride, u32 tag,
    float* __restrict__ qkeep, RowList... rowlist) {
    // The first `nfin` workgroups of a launch run the PREVIOUS launch's selection jobs
    // (finalize_body, ls_select_dev.h) while every other workgroup scans for the current queries:
    // selection costs neither a launch nor a kernel boundary and hides under the scan.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_dyn[];
    if ((int)blockIdx.x < nfin) {
        // (a job of this launch's OWN queries - ls_fin_params::wait - sweeps the tagged granules the
        // scan workgroups below are writing; they never wait for anything. Should they not get to
        // run while this workgroup holds its slot (a CU-masked stream, a partitioned device) the
        // sweep gives up after 200 ms and asks the host for a retry.)
        // (a single-query launch without a score vector keeps its raw query for the repair, ls_api.hip
        // mq_repair: the riding selection workgroup has the time, the scan workgroups do not)
        if (NQ == 1 && qkeep && blockIdx.x == 0)
            for (int e = threadIdx.x; e < d; e += LS_SCAN_THREADS) qkeep[e] = qraw[e];
        for (int j = blockIdx.x; j < fin.njobs; j += nfin) {  // (nfin workgroups share the fin.njobs jobs)
            if (j != (int)blockIdx.x) __syncthreads();        // the previous job's LDS is free again
            finalize_body<LS_SCAN_THREADS>(ls_fin_job(fin, j), smem_dyn, threadIdx.x);
        }
        return;
    }
    const int bid = (int)blockIdx.x - nfin;
    const int nblk = (int)gridDim.x - nfin;
    if (NQ == 1 && qkeep && nfin == 0 && bid == 0)  // (nothing rides on this launch: scan workgroup 0 copies)
        for (int e = threadIdx.x; e < d; e += LS_SCAN_THREADS) qkeep[e] = qraw[e];
#ifdef LS_HANDOFF_TIMING
    if (threadIdx.x == 0) atomicMax(&g_ho[0], ~wall_clock64());
#endif
#ifdef LS_SCAN_TIMING  // developer instrumentation: phase stamps (100 MHz ticks) of one scan workgroup
    unsigned long long stamp[6];
#define LS_SSTAMP(i) stamp[i] = wall_clock64()
#else
#define LS_SSTAMP(i) do {} while (0)
#endif
    LS_SSTAMP(0);
    constexpr int R = LS_WAVE / L;  // rows per wave load step
    constexpr int TR = U * R;       // rows per tile: one tile = U steps = TR contiguous rows
    static_assert(TR <= LS_WAVE, "a tile's scores must fit one per lane");
    const int lane = threadIdx.x & (LS_WAVE - 1);
    const int wave = threadIdx.x / LS_WAVE;
    const int sub = lane & (L - 1);
    const int grp = lane / L;
    const int kp = kprime + 1;

    // Tiles are dealt round-robin to waves; the 4 waves of a workgroup take 4 adjacent tiles,
    // so one workgroup iteration covers 4*TR contiguous rows and its S stores fill whole lines.
    const long long W = (long long)nblk * LS_SCAN_WAVES;
    const long long gw = (long long)bid * LS_SCAN_WAVES + wave;
    const long long NT = (n + TR - 1) / TR;

    constexpr bool SQ8 = ls_pack_sq8<RowList...>::value;
    constexpr bool L2 = ls_pack_l2<RowList...>::value;
    constexpr bool BF16 = ls_pack_bf16<RowList...>::value;
    using QR = scan_query_t<F16, V, SQ8, L2, BF16>;
    constexpr int PF = SMALL ? QR::SMALL_PF : 1;  // tile buffers (statically indexed: the loop body is unrolled PF times)
    f32x4 xb[PF][U][V];
    constexpr bool IDX = sizeof...(RowList) == (SQ8 || L2 || BF16 ? 2 : 1);
    static_assert(!IDX || NQ == 1, "the subset scan serves one query per launch");
    static_assert(!SQ8 || NQ == 1, "an sq8 launch serves one query");
    static_assert(!BF16 || (NQ == 1 && !SQ8 && !L2 && !F16), "a bf16 launch serves one inner-product query");
    static_assert(!L2 || !SQ8, "an L2 launch scans f32 or fp16 rows");
    constexpr bool L2MQ = L2 && NQ > 1;  // several L2 queries: QueryL2Pair registers, the reduce-scatter branch only
    static_assert(!L2MQ || (LS_SCAN_MQ_SCATTER && NQ % 2 == 0 && !SMALL), "L2 query pairs ride on the reduce-scatter branch");
    u32 li[PF][IDX ? U : 1];  // IDX: rows of the next tile buffer pb loads
    auto fetch_list = [&](u32 (&e)[IDX ? U : 1], long long t) {
        if constexpr (IDX) {
            const u32* __restrict__ list = [](const u32* l, auto...) { return l; }(rowlist...);
            if (t >= NT) return;
            if (reverse) t = NT - 1 - t;
            const long long r0 = t * TR + grp;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long long r = r0 + u * R;
                e[u] = list[r < n ? r : n - 1];
            }
        }
    };
    auto issue_loads = [&](f32x4 (&x)[U][V], long long t, int pb) {
        const long long t_in = t;
        if (reverse) t = NT - 1 - t;  // optional back-to-front sweep (see ls_api.hip)
        const long long r0 = t * TR + grp;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            long long r = r0 + u * R;
            r = r < n ? r : n - 1;  // ragged last tile: re-read the last row, masked out below
            if constexpr (IDX) r = li[pb][u];
            const f32x4* p = corpus + r * chunks + sub;
#pragma unroll
            for (int v = 0; v < V; ++v) x[u][v] = __builtin_nontemporal_load(p + L * v);
        }
        if constexpr (IDX) fetch_list(li[pb], t_in + PF * W);  // buffer pb's next tile
        (void)t_in;
    };
    long long t = gw;
    if constexpr (IDX) {  // every buffer's first tile: one batch of independent list loads
#pragma unroll
        for (int pf = 0; pf < PF; ++pf) fetch_list(li[pf], t + pf * W);
    }
    // the first tile's loads fly while the queries are prepared (SMALL: the query goes first -
    // loads return in order, it must not queue behind four tiles - and the tiles follow it)
    if (!SMALL && t < NT) issue_loads(xb[0], t, 0);

    // NQ queries -> registers, with faiss.normalize_L2 (reference search/engine.py:242) fused
    // in: x *= 1/sqrt(sum x^2), rows of zero norm untouched. One pass over the corpus then
    // serves all NQ queries (the reference sends one query at a time; small batches share the
    // HBM traffic this way).
    QR qr[NQ];  // (L2MQ: unused, the queries sit in qp)
    QueryL2Pair<F16, V> qp[L2MQ ? NQ / 2 : 1];
    if constexpr (L2MQ) {
#pragma unroll
        for (int pr = 0; pr < NQ / 2; ++pr) {
            const float* qa = qraw + (long long)(2 * pr) * d;
            float inv[2] = {1.0f, 1.0f};
            if (normalize) {  // the library's canonical summation order (ls_common.h)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float ss = ls_wave_sumsq(qa + (long long)h * d, d, lane);
                    if (ss > 0.0f) inv[h] = 1.0f / sqrtf(ss);
                }
            }
            qp[pr].prepare(qa, qa + d, inv[0], inv[1], d, sub, L);
        }
    }
#pragma unroll
    for (int qi = 0; qi < (L2MQ ? 0 : NQ); ++qi) {
        (void)qr[qi].load(qraw + (long long)qi * d, d, sub, L);
        float inv = 1.0f;
        if (normalize) {  // the library's canonical summation order (ls_common.h)
            const float ss = ls_wave_sumsq(qraw + (long long)qi * d, d, lane);
            if (ss > 0.0f) inv = 1.0f / sqrtf(ss);
        }
        qr[qi].scale(inv);
        if constexpr (SQ8) qr[qi].apply_step(ls_pack_step(rowlist...), d, sub, L);
    }

    if constexpr (SMALL) {
        // hipcc waits with vmcnt(0) for the query (the normalise branch merges in front of its
        // first use), i.e. for every load issued before: the four tiles go out behind it
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int pf = 0; pf < PF; ++pf)
            if (t + pf * W < NT) issue_loads(xb[pf], t + pf * W, pf);
    }
    LS_SSTAMP(1);
    u64 lst[NQ];  // per query, lanes 0..kp-1: this wave's best keys, descending
    u64 thr[NQ];  // key in lane kp-1 (wave-uniform): a row must beat it to matter
#pragma unroll
    for (int qi = 0; qi < NQ; ++qi) {
        lst[qi] = 0;
        thr[qi] = 0;
    }

    int ti = 0;  // SMALL: tiles this wave has seen
    auto tile_step = [&](f32x4 (&x)[U][V], int pb) {  // tile t sits in buffer x = xb[pb]
        if (t >= NT) return;
        if constexpr (NQ > 1 && LS_SCAN_MQ_SCATTER) {
            // ---- several queries: all U*NQ partial sums, one reduce-scatter, one score per lane --
            constexpr int P = U * NQ;
            constexpr int NSC = ls_ilog2(L) < ls_ilog2(P) ? ls_ilog2(L) : ls_ilog2(P);  // scatter steps
            constexpr int NRES = P >> NSC;                                               // results per lane
            float p[P];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if constexpr (L2MQ) {
#pragma unroll
                    for (int pr = 0; pr < NQ / 2; ++pr) qp[pr].dot(x[u], p[u * NQ + 2 * pr], p[u * NQ + 2 * pr + 1]);
                } else {
#pragma unroll
                    for (int qi = 0; qi < NQ; ++qi) p[u * NQ + qi] = qr[qi].dot(x[u]);
                }
            }
            const long long tt = reverse ? NT - 1 - t : t;
            t += W;
            if (t + (PF - 1) * W < NT) issue_loads(x, t + (PF - 1) * W, pb);  // overlaps everything below
            rs_step<L, 1, P, P>::run(p, sub);
            if constexpr (L2) {  // (the score is the negated distance: negated once, behind the sum - as behind group_sum)
#pragma unroll
                for (int c = 0; c < NRES; ++c) p[c] = -p[c];
            }
            // lane `sub` now holds pairs j = (c << NSC) | (sub & (2^NSC - 1)), c < NRES; with lanes
            // to spare (L > P) the copies in lanes sub >= P are ignored
            const bool holder = (sub >> NSC) == 0 || NSC == ls_ilog2(L);
            u64 key[NRES];
            int myq[NRES];
#pragma unroll
            for (int c = 0; c < NRES; ++c) {
                const int j = (c << NSC) | (sub & ((1 << NSC) - 1));
                const int qi = j % NQ, u = j / NQ;
                const long long row = tt * TR + u * R + grp;
                const bool valid = holder && row < n;
                if (valid && S) S[qi * s_stride + row] = p[c];
                key[c] = valid ? ls_make_key(p[c], (u32)row) : 0ull;
                myq[c] = qi;
            }
#pragma unroll
            for (int qi = 0; qi < NQ; ++qi) {
#pragma unroll
                for (int c = 0; c < NRES; ++c) {
                    const u64 kq = myq[c] == qi ? key[c] : 0ull;
                    u64 mask = __ballot(kq > thr[qi]);
                    while (mask) {  // rare once the threshold has warmed up
                        const int j = __ffsll((long long)mask) - 1;
                        mask &= mask - 1;
                        const u64 v = readlane64(kq, j);
                        if (v <= thr[qi]) continue;  // the ballot is older than the threshold
                        wave_insert(lst[qi], v, lane, kp);
                        thr[qi] = readlane64(lst[qi], kp - 1);
                    }
                }
            }
            ++ti;
            return;
        }
        // lane i < TR collects the score of tile row i, per query (SMALL: lane ti*TR + i)
        float sc[NQ];
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) sc[qi] = 0.0f;
        const int lane0 = SMALL ? ti * TR : 0;
        float part[SQ8 ? U : 1];  // sq8: the U rows' partial sums, their chains advanced in step
        if constexpr (SQ8) qr[0].template dot_tile<U>(x, part);
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int qi = 0; qi < NQ; ++qi) {
                float ps;
                if constexpr (SQ8) ps = part[u];
                else ps = qr[qi].dot(x[u]);
                const float gs = group_sum<L>(ps);                // valid in all L lanes of a group
                const float s = L2 ? -gs : gs;                    // (L2: the score is the negated distance)
                const float sel = pick_group<L>(s, lane);         // lane i <- group (i % R)
                if (lane / R == (SMALL ? ti * U : 0) + u) sc[qi] = sel;
            }
        }
        const long long tt = reverse ? NT - 1 - t : t;
        const long long row = tt * TR + (lane - lane0);
        t += W;
        if (t + (PF - 1) * W < NT) issue_loads(x, t + (PF - 1) * W, pb);  // overlaps the selection below
        const bool valid = lane >= lane0 && lane < lane0 + TR && row < n;
        ++ti;
        if constexpr (SMALL) {
#pragma unroll
            for (int qi = 0; qi < NQ; ++qi) {
                if (valid) {
                    if (S) S[qi * s_stride + row] = sc[qi];
                    lst[qi] = ls_make_key(sc[qi], (u32)row);  // this lane's one key of the launch
                }
            }
            return;
        }
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) {
            if (valid && S) S[qi * s_stride + row] = sc[qi];  // TR contiguous floats (S == nullptr: ls_api.hip mq_repair)
            const u64 key = valid ? ls_make_key(sc[qi], (u32)row) : 0ull;
            u64 mask = __ballot(key > thr[qi]);
            while (mask) {  // rare once the threshold has warmed up
                const int j = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const u64 v = readlane64(key, j);
                wave_insert(lst[qi], v, lane, kp);
                thr[qi] = readlane64(lst[qi], kp - 1);
            }
        }
    };
    while (t < NT) {  // buffers are named statically: PF calls per round
        tile_step(xb[0], 0);
        if constexpr (PF >= 2) tile_step(xb[1], 1);
        if constexpr (PF == 4) {
            tile_step(xb[2], 2);
            tile_step(xb[3], 3);
        }
    }

    LS_SSTAMP(2);
    // merge the 4 wave lists of every query -> this workgroup's best kprime keys + bound
    __shared__ u64 sm[NQ][LS_SCAN_WAVES * LS_KP_MAX];
    if constexpr (SMALL) {
        // every lane holds at most one key: its rank among the wave's keys by counting (non-zero
        // keys are unique; the "no row" lanes hold 0 and rank behind every real key)
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi) {
            const u64 mine = lst[qi];
            int rank = 0;
            for (int t2 = 0; t2 < ti; ++t2) {  // only the lanes that can hold a key: ti tiles of TR rows
#pragma unroll
                for (int r = 0; r < TR; ++r) rank += readlane64(mine, t2 * TR + r) > mine;
            }
            if (lane < LS_KP_MAX) sm[qi][wave * LS_KP_MAX + lane] = 0ull;
            if (mine != 0ull && rank < kp) sm[qi][wave * LS_KP_MAX + rank] = mine;
        }
    } else {
#pragma unroll
        for (int qi = 0; qi < NQ; ++qi)
            if (lane < LS_KP_MAX) sm[qi][wave * LS_KP_MAX + lane] = (lane < kp) ? lst[qi] : 0ull;
    }
    __syncthreads();
    LS_SSTAMP(3);
    for (int qi = wave; qi < NQ; qi += LS_SCAN_WAVES) {  // wave w ranks queries w, w+4, ..
        const u64 mine = sm[qi][lane];  // LS_SCAN_WAVES * LS_KP_MAX == 64 slots
        int rank = 0;
        if constexpr (SMALL || LS_SCAN_MERGE_FILLED) {  // only the kp slots each wave filled (the others hold 0)
            for (int w = 0; w < LS_SCAN_WAVES; ++w)
                for (int j = 0; j < kp; ++j) {
                    const int i = w * LS_KP_MAX + j;
                    const u64 o = sm[qi][i];
                    rank += (o > mine) || (o == mine && i < lane);
                }
        } else {
#pragma unroll 8
            for (int i = 0; i < LS_SCAN_WAVES * LS_KP_MAX; ++i) {
                const u64 o = sm[qi][i];
                rank += (o > mine) || (o == mine && i < lane);
            }
        }
        if (gran) {
            // same-launch selection: the keys are the whole hand-off - ONE 16-byte write-through
            // (sc1) store per key, {key, tag}: the selection workgroup recognises this launch's data
            // by the tag, so there is nothing to drain, no barrier and no counter behind the stores
            // (ls_fin_params::gran; rank-major: granule [rank][workgroup], plane kprime = bounds)
            if (rank <= kprime) {
                __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
                    (char*)gran + (long long)qi * g_stride * 16, 0, nblk * (kprime + 1) * 16, LS_BUF_RSRC_FLAGS);
                __builtin_amdgcn_raw_buffer_store_b128(u32x4{(u32)mine, (u32)(mine >> 32), tag, 0u}, rsrc,
                                                       (rank * nblk + bid) * 16, 0, LS_AUX_SC1);
            }
        } else {
            if (rank < kprime) cand[qi * c_stride + (long long)bid * kprime + rank] = mine;
            if (rank == kprime) bound[qi * b_stride + bid] = mine;
        }
    }
#ifdef LS_HANDOFF_TIMING
    if (threadIdx.x == 0) atomicMax(&g_ho[1], wall_clock64());
#endif
#ifdef LS_SCAN_TIMING
    LS_SSTAMP(4);
    if (bid == nblk / 2 && threadIdx.x == 0)
        for (int i = 0; i < 4; ++i) cand[c_stride - 8 + i] = stamp[i + 1] - stamp[i];
    if (threadIdx.x == 0 && NQ == 1) {  // every workgroup's start / end tick: slot 7 of S is unused
        unsigned long long* life = reinterpret_cast<unsigned long long*>(S + 7 * s_stride);
        life[2 * bid] = stamp[0];
        life[2 * bid + 1] = stamp[4];
    }
#endif
}
