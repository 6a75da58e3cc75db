// ls_scan.hip — the HBM-bound scan: one query against every corpus row (batch-1 path).
//
// Replaces the hot loop inside faiss `index.search(x, k)` for nq = 1, the only shape the
// reference ever issues (reference src/lean_explore/search/engine.py:250, nq = 1 at :238).
//
// Roofline: 2 flops per corpus element read, 0.5 FLOP/B for fp32 -> HBM bound. Algorithmic
// bytes per query = n * d * elem (corpus) + d*4 (query) + n*4 (score vector S) + candidates.
//
// Work decomposition (gfx950: 256 CUs, 64-lane waves)
//   - a row is `chunks` 16-byte chunks; L lanes share a row (lane `sub` takes chunks
//     sub, sub+L, ..), so one wave load instruction fetches 64/L whole rows as 64/L
//     contiguous segments of L*16 bytes: fully coalesced global_load_dwordx4.
//   - rows are dealt round-robin to waves in groups of R = 64/L rows; the four waves of a
//     workgroup take groups that are gridDim.x groups apart, so a run of adjacent, similar
//     rows (typical for a corpus ordered by module) is spread over many workgroups.
//   - U row groups are in flight per wave (U*V 16-byte loads per lane outstanding).
//   - dot product: per-lane fp32 FMA chain over its chunks, then an xor-butterfly over the L
//     lanes sharing the row.
//   - selection is fused: each wave keeps its best KP = k'+1 keys in lanes 0..KP-1 (sorted);
//     a wave-uniform threshold rejects almost every row with one 64-bit compare. The workgroup
//     merges its 4 lists and emits its best k' keys plus the (k'+1)-th as a bound. The finalize
//     kernel (ls_select.hip) proves the global top-k is contained in the emitted keys, or falls
//     back to an exact selection over the score vector S, which this kernel also writes.
#include "ls_select_dev.h"
#ifdef LS_SCAN_ABL_NOS  // timing ablation: no score vectors (results of unproven queries are wrong)
#define LS_SCAN_S(x) ((float*)nullptr)
#else
#define LS_SCAN_S(x) (x)
#endif

#include "ls_scan_kernel.h"


// ------------------------------------------------------------------------------------------

int ls_scan_blocks(int64_t n, const ls_geom& g, int32_t n_cu) {
    constexpr int bpc = 2;  // scan workgroups per CU
    const int64_t TR = (int64_t)scan_unroll(g.V) * (LS_WAVE / g.L);
    const int64_t NT = (n + TR - 1) / TR;
    // minimum tiles per wave. Small shards: fewer blocks -> fewer candidate keys for the
    // piggy-backed finalize, which bounds the launch there (N=25k: 18.6 -> 11.7 us/step)
    constexpr int tpw = 4;
    int64_t b = (NT + LS_SCAN_WAVES * tpw - 1) / (LS_SCAN_WAVES * tpw);
    const int64_t cap = (int64_t)n_cu * bpc;
    if (b > cap) {
        // Big shards: tiles are dealt round-robin to 4*b waves, so the launch ends with a partial
        // round in which only frac(NT / 4b) of the waves still have a tile - too few to keep HBM
        // busy. Measured on config 2 (25 000 tiles): 512 workgroups (12.2 rounds) 47.55 us,
        // 448 (13.95 rounds) 47.03 us; config 2' 123.2 vs 120.4 us (tools/scan_blocks_sweep.py).
        // Pick the count in [1.5, 2] workgroups per CU (multiples of the 8 XCDs) whose last round
        // is the fullest.
        int64_t best = cap;
        double best_fill = -1.0;
        for (int64_t c = cap; c >= cap * 3 / 4; c -= 8) {
            const double rounds = (double)NT / (double)(c * LS_SCAN_WAVES);
            double fill = rounds - (double)(int64_t)rounds;
            if (fill == 0.0) fill = 1.0;
            if (fill > best_fill + 0.02) {  // near-ties go to the larger count
                best_fill = fill;
                best = c;
            }
        }
        b = best;
    }
    if (b < 1) b = 1;
    return (int)b;
}

template <bool F16, int L, int V, int NQ>
static int launch_lvq(const void* corpus, int64_t n, const ls_geom& g, const ls_scan_args& a,
                      hipStream_t s) {
    constexpr int U = scan_unroll(V);
    size_t smem = 0;
    if (a.nfin > 0) {
        const ls_fin_params& fp = a.fin.p0;
        const int keff = (int)((long long)fp.k < fp.n ? fp.k : fp.n);
        smem = ls_fin_lds_bytes(fp.keys_cap, keff);
    }
    const int nfw = std::min(a.nfin, LS_FIN_WG_MAX);  // selection workgroups (jobs nfw.. are second rounds)
    // single-query launches in which no wave sees more than 64 rows rank once instead of inserting
    constexpr int TR = U * (LS_WAVE / L);
    const long long waves = (long long)a.blocks * LS_SCAN_WAVES;
    const long long tiles_per_wave = ((n + TR - 1) / TR + waves - 1) / waves;
    // (with two or more workgroups per CU the other one hides the latency: measured neutral at
    // N = 50 k, 3 % slower at 100 k, 6-11 % faster at 25 k and 10 k)
    const bool small = LS_SCAN_SMALL && NQ == 1 && tiles_per_wave * TR <= LS_SCAN_SMALL_ROWS &&
                       a.blocks <= LS_SCAN_SMALL_MAX_BLOCKS;
#define LS_SCAN_LAUNCH(SM)                                                                         \
    {                                                                                              \
        auto kern = ls_scan_kernel<F16, L, V, U, NQ, SM>;                                          \
        static ls_attr_once once;                                                                  \
        if (int rc = ls_set_max_dynamic_lds(once, (const void*)kern, LS_PIGGY_LDS_MAX)) return rc; \
        hipLaunchKernelGGL(kern, dim3(a.blocks + nfw), dim3(LS_SCAN_THREADS), smem, s,          \
                           (const f32x4*)corpus, (long long)n, g.chunks, a.d_q, g.d,               \
                           a.normalize ? 1 : 0, a.reverse ? 1 : 0, LS_SCAN_S(a.d_S), (long long)a.s_stride,   \
                           a.d_cand, (long long)a.c_stride, a.d_bound, (long long)a.b_stride,      \
                           a.kprime, nfw, a.fin, a.d_gran, (long long)a.g_stride, a.tag, a.d_qkeep);                          \
    }
    if constexpr (NQ == 1) {
        if (small) LS_SCAN_LAUNCH(true) else LS_SCAN_LAUNCH(false)
    } else {
        LS_SCAN_LAUNCH(false)
    }
#undef LS_SCAN_LAUNCH
    LS_HIP(hipGetLastError());
    return LS_OK;
}

template <bool F16, int L, int V>
static int launch_lv(const void* corpus, int64_t n, const ls_geom& g, const ls_scan_args& a,
                     hipStream_t s) {
    switch (a.nq) {
        case 1: return launch_lvq<F16, L, V, 1>(corpus, n, g, a, s);
        case 4: return launch_lvq<F16, L, V, 4>(corpus, n, g, a, s);
        case 8: return launch_lvq<F16, L, V, 8>(corpus, n, g, a, s);
    }
    ls_set_error("ls_launch_scan: unsupported queries per launch %d", a.nq);
    return LS_ERR_INVALID_ARG;
}

template <bool F16>
static int launch_dt(const void* corpus, int64_t n, const ls_geom& g, const ls_scan_args& a,
                     hipStream_t s) {
#define LS_CASE(LL, VV) \
    if (g.L == LL && g.V == VV) return launch_lv<F16, LL, VV>(corpus, n, g, a, s);
    LS_CASE(16, 1) LS_CASE(16, 2) LS_CASE(16, 3) LS_CASE(16, 4)
    LS_CASE(32, 3) LS_CASE(32, 4)
    LS_CASE(64, 3) LS_CASE(64, 4)
#undef LS_CASE
    ls_set_error("ls_launch_scan: unsupported row geometry L=%d V=%d", g.L, g.V);
    return LS_ERR_INVALID_ARG;
}

int ls_launch_scan(const void* d_corpus, int64_t n, const ls_geom& g, const ls_scan_args& a,
                   hipStream_t s) {
    if (n <= 0) return LS_OK;
    if (a.kprime < 1 || a.kprime + 1 > LS_KP_MAX) {
        ls_set_error("ls_launch_scan: kprime %d out of range", a.kprime);
        return LS_ERR_INVALID_ARG;
    }
    if (g.elem == 1) return ls_launch_scan_sq8(d_corpus, n, g, a, s);  // (ls_sq8_scan.hip)
    return g.elem == 2 ? launch_dt<true>(d_corpus, n, g, a, s) : launch_dt<false>(d_corpus, n, g, a, s);
}

// ---- subset scan (ls_subset.hip): one query over the m rows of an ascending row list ----------------------------
// The plain single-query launch with positions for rows: blocks, k' and the SMALL decision come from m (a.blocks,
// a.kprime are the caller's, planned from m); the dot products are the plain kernel's of the same geometry, so
// every score is bit-identical to the one the unfiltered scan gives that row.
template <bool F16, int L, int V>
static int launch_subset_lv(const void* corpus, const u32* list, int64_t m, const ls_geom& g, const ls_scan_args& a,
                            hipStream_t s) {
    constexpr int U = scan_unroll(V);
    constexpr int TR = U * (LS_WAVE / L);
    const long long waves = (long long)a.blocks * LS_SCAN_WAVES;
    const long long tiles_per_wave = ((m + TR - 1) / TR + waves - 1) / waves;
    const bool small = LS_SCAN_SMALL && tiles_per_wave * TR <= LS_SCAN_SMALL_ROWS && a.blocks <= LS_SCAN_SMALL_MAX_BLOCKS;
    auto kern = small ? ls_scan_kernel<F16, L, V, U, 1, true, const u32*> : ls_scan_kernel<F16, L, V, U, 1, false, const u32*>;
    hipLaunchKernelGGL(kern, dim3(a.blocks), dim3(LS_SCAN_THREADS), 0, s, (const f32x4*)corpus, (long long)m,
                       g.chunks, a.d_q, g.d, a.normalize ? 1 : 0, a.reverse ? 1 : 0, LS_SCAN_S(a.d_S),
                       (long long)a.s_stride, a.d_cand, (long long)a.c_stride, a.d_bound, (long long)a.b_stride,
                       a.kprime, 0, a.fin, (void*)nullptr, 0ll, 0u, (float*)nullptr, list);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

template <bool F16>
static int launch_subset_dt(const void* corpus, const u32* list, int64_t m, const ls_geom& g, const ls_scan_args& a,
                            hipStream_t s) {
#define LS_CASE(LL, VV) \
    if (g.L == LL && g.V == VV) return launch_subset_lv<F16, LL, VV>(corpus, list, m, g, a, s);
    LS_CASE(16, 1) LS_CASE(16, 2) LS_CASE(16, 3) LS_CASE(16, 4)
    LS_CASE(32, 3) LS_CASE(32, 4)
    LS_CASE(64, 3) LS_CASE(64, 4)
#undef LS_CASE
    ls_set_error("ls_launch_scan_subset: unsupported row geometry L=%d V=%d", g.L, g.V);
    return LS_ERR_INVALID_ARG;
}

int ls_launch_scan_subset(const void* d_corpus, const u32* d_list, int64_t m, const ls_geom& g, const ls_scan_args& a,
                          hipStream_t s) {
    if (m <= 0) return LS_OK;
    if (a.nq != 1 || a.nfin != 0 || a.kprime < 1 || a.kprime + 1 > LS_KP_MAX) {
        ls_set_error("ls_launch_scan_subset: one query, no riding jobs, kprime in range (nq %d kprime %d)", a.nq,
                     a.kprime);
        return LS_ERR_INVALID_ARG;
    }
    if (g.elem == 1) return ls_launch_scan_subset_sq8(d_corpus, d_list, m, g, a, s);
    return g.elem == 2 ? launch_subset_dt<true>(d_corpus, d_list, m, g, a, s)
                       : launch_subset_dt<false>(d_corpus, d_list, m, g, a, s);
}
