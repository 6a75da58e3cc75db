// ls_mq.hip — small batches on an fp32 index: 2..32 queries share ONE pass over the corpus, with the
// inner products on the f32 matrix cores and BIT-IDENTICAL to the single-query scan kernel.
//
// Replaces faiss `index.search(x, k)` for the batch sizes between the reference's own call (nq = 1,
// reference src/lean_explore/search/engine.py:238-250 -> ls_scan.hip) and the big-batch MFMA paths: what
// a multi-client server produces when this library combines concurrent callers (engine.py:250 called
// from several MCP clients, mcp/server.py:147-151), small explicit batches, and the repairs of the
// batched paths. Until round 5 these ran the VALU scan in groups of 8 queries: 75 us (d = 384) /
// 180 us (d = 1024) per 8-query pass at N = 200 k against 47 / 124 us of HBM time, 16 queries two passes.
//
// Roofline: HBM for 2..16 queries (one MFMA B block, NB = 1): one pass reads the corpus once
// (n * d * 4 bytes); v_mfma_f32_16x16x4_f32 at 16 query columns needs n * d / 64 instructions of 32 cycles:
// 15.6 us (d = 384) / 41.7 us (d = 1024) of matrix time per SIMD-filled chip at N = 200 k, under the
// 47 / 124 us the HBM stream takes. 17..32 queries (NB = 2, round 6) double the matrix and VALU work per
// byte: ONE exact pass instead of two (68 us against 2 x 54 at d = 384, 168 against 2 x 138 at d = 1024),
// bound by instruction issue, not by HBM (section "Two B blocks" below).
//
// Same bits as ls_scan.hip. The scan kernel's fp32 order (ls_scan.hip QueryRegs::dot + group_sum;
// restated by oracle/flat_ip_ref.c ORDER_SCAN) is: lane `sub` of the L lanes sharing a row runs one
// fmaf chain over its chunks sub, sub+L, .., sub+(V-1)L (4 floats each, memory order), then a balanced
// xor tree over the L partial sums. tools/arith_probe.hip shows v_mfma_f32_16x16x4_f32 to be, bit for
// bit, acc = fmaf(a[k], b[k], acc) for k = 0, 1, 2, 3 in that order. So ONE MFMA whose K dimension is the
// four floats of chunk c advances chain (c mod L) by exactly the scan kernel's four fmafs - for 16 rows x
// 16 queries at once - and L accumulators per (row block, query block) hold the L chains; the tree is L-1
// vector adds. A query's scores, and therefore its results and their order, do not depend on whether it
// was served alone (scan) or in company (here): tests/test_mq_gpu.py, tests/test_concurrent_gpu.py and the
// zero-excuse parity checks (oracle.compare_kernel_order) assert array_equal.
//
// Work decomposition (one workgroup per CU: 4 waves, or 8 with two B blocks)
//   - a wave takes tiles of 16 consecutive rows, round-robin over all waves of the launch.
//   - MFMA operand layout: lane (i = lane % 16, kq = lane / 16) supplies A[row i][k = kq] and
//     B[k = kq][query i]. A lane loads ONE 16-byte chunk of its row per load instruction (chunk
//     cb + kq: the four lane groups cover four consecutive chunks = 64 contiguous bytes per row); a
//     4 x 4 transpose across the lane groups (2 x v_permlane32_swap + 2 x v_permlane16_swap on the four
//     registers) then leaves register m = element kq of chunk cb + m: four MFMA A operands for four
//     VALU instructions, no LDS round trip for the corpus. The loads stream through a static ring of P
//     "units" (1 KB per wave each), continuing into the wave's next tile. Round 6: P = 2 V units (6-8 KB
//     per wave in flight), HALF the scan kernel's depth - N = 200 k, 16 queries, d = 384, one box: P = 2 / 3 /
//     4 / 6 / 8 / 12 units: 68.6 / 59.9 / 55.5 / 53.1 / 54.6 / 57.2 us (d = 1024, P = 4 / 8 / 16: 150.7 / 140 /
//     142.8): 964 waves x 6 KB already cover HBM's latency, anything deeper only queues. (Requesting the wave's
//     whole first tile ahead of the query staging - 2 P units in flight during those 2.4-4 us - changed
//     nothing: 51.2 us either way.)
//   - chains are processed in groups of GC (16; 8 with two B blocks): group g = chains GC g..GC g+GC-1, their V
//     chunks each, then the group's add tree; the L / GC group sums meet on the upper levels of the same
//     tree as they complete (a binary counter of partial sums: log2 registers). The unit order inside a tile is
//     a compile-time permutation of the row's chunks; both halves of every 128-byte line are fetched by
//     consecutive units.
//   - B (the queries, normalised like the scan kernel's prologue: ls_wave_sumsq, one multiply per
//     element) lives in LDS query-major with a pitch of 2 (mod 32) floats: conflict-free staging writes
//     and fragment reads (mq_pitch).
//   - selection: the score block leaves lane (kq, query) with rows 4kq..4kq+3 of its query. Every lane
//     keeps the best M keys it has seen (branch-free compare-exchange chain; M = 3, 5 or 8, chosen by the
//     host from k / lanes so that a lane holding M of a query's top-k is a 1e-3 event). At the end the
//     four lane groups of a wave merge their lists in registers (top M of the union + the best key that
//     dropped out), the waves' lists meet in LDS (over the queries: they are dead by then), and the
//     workgroup emits its best k' of those keys (+ granule / bound exactly like the scan kernel:
//     finalize_body, the same-launch hand-off and the stand-alone finalize are shared unchanged).
//     bound = max(best key not emitted, best key dropped in a merge, every lane's M-th key): whatever the
//     workgroup saw and did not emit lies under it, so the proof in finalize_body holds; if it fails the
//     query is served again on the scan kernel, or - LS_FLAG_ASYNC-only calls - the rescue sweeps the score
//     vector S this kernel then writes like the scan does.
//
// Two B blocks (17..32 queries). Every A operand meets two 16-column B blocks: 8 MFMAs per 64-byte unit,
// 192 / 512 per tile (d = 384 / 1024) on 526 / 1265 other VALU instructions. A wave issues in order: eight
// back-to-back MFMAs hold it for 256 cycles, its lane swaps, adds and key inserts then run with the matrix
// pipe idle - one wave per SIMD took 82 / 197 us. Eight-wave workgroups (two waves per SIMD, <= 256 registers:
// 8 chains per group, no AGPR traffic; one shared copy of the queries, 131 KB at d = 1024) fill each other's
// gaps: 68 / 168 us, for 41 / 109 us of matrix time on the 224 CUs the launch uses (16 are left to the
// selection workgroups riding along). Measured and removed on the way (docs/EXPERIMENTS.md, round 6): a
// one-unit software pipeline (next unit's LDS reads and lane swaps under this unit's MFMAs: 75 vs 74 us, and
// 64 vs 55 us with one block), refills in bursts of 2 / 4 units (65 vs 59 us), 16 chains per group in 512
// registers (every tree add reads an AGPR back: 754 / 1745 VALU per tile).
#include "ls_mq_kernel.h"

#ifndef LS_MQ_KERNEL_ONLY  // (scratch builds that instantiate one kernel and look at its ISA)
#include "ls_mq_launch.h"
// ---- host side ------------------------------------------------------------------------------------
// a.nq = the real query count (2..32); a.blocks / a.kprime / a.mq_keys: ls_mq_make_plan for that count. A launch of
// 17..32 queries runs the two-block kernel in eight-wave workgroups that fill their CU (two waves per SIMD at up to 256
// registers, up to 131 KB of LDS); one block: a riding selection job's LDS stays under LS_PIGGY_LDS_MAX and so do 16
// queries of 4 KB rows.
int ls_launch_mq(const void* d_corpus, int64_t n, const ls_geom& g, const ls_scan_args& a, hipStream_t s) {
    if (n <= 0) return LS_OK;
    if (!ls_mq_args_ok(g, a, 4, 2 * LS_MQ_NQ, a.nq > LS_MQ_NQ ? LS_MQ_WAVES2 : LS_MQ_WAVES)) {
        ls_set_error("ls_launch_mq: bad arguments (elem %d nq %d kprime %d keys %d)", g.elem, a.nq, a.kprime, a.mq_keys);
        return LS_ERR_INVALID_ARG;
    }
    return ls_geom_dispatch<false, true>("ls_launch_mq", g, [&](auto l, auto v) {
        return ls_mq_dispatch<true>(a, [&](auto m, auto nb) {
            constexpr int L = decltype(l)::value, V = decltype(v)::value, M = decltype(m)::value, NB = decltype(nb)::value;
            constexpr int WPB = NB == 1 ? LS_MQ_WAVES : LS_MQ_WAVES2;
            return ls_mq_launch<ls_mq_kernel<L, V, M, NB, WPB>>("ls_launch_mq", WPB, mq_lds_bytes(g.chunks, M, NB, WPB),
                                                                NB == 1 ? LS_PIGGY_LDS_MAX : LS_MQ_LDS_MAX2,
                                                                (const mq_f32x4*)d_corpus, n, g, a, s);
        });
    });
}
#endif  // LS_MQ_KERNEL_ONLY
