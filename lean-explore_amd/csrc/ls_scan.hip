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
#endif

#include "ls_scan_launch.h"

int ls_scan_blocks(int64_t n, const ls_geom& g, int32_t n_cu) { return ls_scan_blocks_lv(n, g.L, g.V, n_cu); }

template <bool F16>
static int launch_dt(const void* corpus, int64_t n, const ls_geom& g, const ls_scan_args& a, hipStream_t s) {
    return ls_geom_dispatch<false, true>("ls_launch_scan", g, [&](auto L, auto V) -> int {
        switch (a.nq) {
            case 1: return ls_scan_launch<F16, L(), V(), 1>(corpus, n, g, a, s);
            case 4: return ls_scan_launch<F16, L(), V(), 4>(corpus, n, g, a, s);
            case 8: return ls_scan_launch<F16, L(), V(), 8>(corpus, n, g, a, s);
        }
        ls_set_error("ls_launch_scan: unsupported queries per launch %d", a.nq);
        return LS_ERR_INVALID_ARG;
    });
}

int ls_launch_scan(const void* d_corpus, int64_t n, const ls_geom& g, const ls_scan_args& a,
                   hipStream_t s) {
    if (n <= 0) return LS_OK;
    if (a.kprime < 1 || a.kprime + 1 > LS_KP_MAX) {
        ls_set_error("ls_launch_scan: kprime %d out of range", a.kprime);
        return LS_ERR_INVALID_ARG;
    }
    if (a.l2) return ls_launch_scan_l2(d_corpus, n, g, a, s);          // (ls_l2_scan.hip)
    if (g.bf16) return ls_launch_scan_bf16(d_corpus, n, g, a, s);      // (ls_bf16_scan.hip)
    if (g.elem == 1) return ls_launch_scan_sq8(d_corpus, n, g, a, s);  // (ls_sq8_scan.hip)
    return g.elem == 2 ? launch_dt<true>(d_corpus, n, g, a, s) : launch_dt<false>(d_corpus, n, g, a, s);
}

// ---- subset scan (ls_subset.hip): one query over the m rows of an ascending row list ----------------------------
// The plain single-query launch with positions for rows: blocks, k' and the SMALL decision come from m (a.blocks,
// a.kprime are the caller's, planned from m); the dot products are the plain kernel's of the same geometry, so
// every score is bit-identical to the one the unfiltered scan gives that row.
template <bool F16>
static int launch_subset_dt(const void* corpus, const u32* list, int64_t m, const ls_geom& g, const ls_scan_args& a,
                            hipStream_t s) {
    return ls_geom_dispatch<false, true>("ls_launch_scan_subset", g, [&](auto L, auto V) -> int {
        return ls_scan_launch<F16, L(), V(), 1>(corpus, m, g, a, s, list);
    });
}

int ls_launch_scan_subset(const void* d_corpus, const u32* d_list, int64_t m, const ls_geom& g, const ls_scan_args& a,
                          hipStream_t s) {
    if (m <= 0) return LS_OK;
    if (a.nq != 1 || a.nfin != 0 || a.kprime < 1 || a.kprime + 1 > LS_KP_MAX) {
        ls_set_error("ls_launch_scan_subset: one query, no riding jobs, kprime in range (nq %d kprime %d)", a.nq,
                     a.kprime);
        return LS_ERR_INVALID_ARG;
    }
    if (a.l2) return ls_launch_scan_subset_l2(d_corpus, d_list, m, g, a, s);
    if (g.bf16) return ls_launch_scan_subset_bf16(d_corpus, d_list, m, g, a, s);
    if (g.elem == 1) return ls_launch_scan_subset_sq8(d_corpus, d_list, m, g, a, s);
    return g.elem == 2 ? launch_subset_dt<true>(d_corpus, d_list, m, g, a, s)
                       : launch_subset_dt<false>(d_corpus, d_list, m, g, a, s);
}
