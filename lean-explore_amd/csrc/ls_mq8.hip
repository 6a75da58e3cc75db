// ls_mq8.hip — small batches on an sq8 index (opt-in: ls_set_sq8_small_batch): 2..16 queries share ONE pass over the
// int8 codes, with the inner products on the f32 matrix cores and BIT-IDENTICAL to the single-query sq8 scan
// (ls_sq8_scan.hip). ls_mq.hip's sq8 sibling.
//
// Replaces faiss `index.search(x, k)` (reference src/lean_explore/search/engine.py:238-250) for what an sq8 index
// served with one launch per query: concurrent callers combined by ls_search, small explicit batches, 2..16-query
// pipelined device calls.
//
// Roofline: one pass reads n x row bytes once - 76.8 MB at N = 200 k, d = 384: ~14 us of HBM time - and
// v_mfma_f32_16x16x4_f32 at 16 query columns needs n * d / 64 instructions of 32 cycles: 15.6 us over 1024 SIMDs, the
// count ls_mq.hip's header derives for fp32. A quarter of ls_mq's bytes for the same matrix work: the pass is bound by
// the matrix pipe and the instructions that feed it, not by HBM. Measured (tools/sq8_small_batch_time.py, DESIGN.md
// 4.9b): 43.4 us for 2 queries, 44.9 us for 16 at that shape (16 single-query launches: 495 us), 104.7 us at d = 1024.
//
// Same bits as the sq8 scan - the invariant (include/leansearch_sq8.h, tests/sq8_ref.c; tests/test_mq8_gpu.py asserts
// array_equal). Chain `sub` of a row is ONE chain acc = fmaf((float)c, q', acc) from 0 over chunks sub, sub + L, ..,
// sub + (V-1) L - 16 codes each, in memory order - then the balanced xor tree over the L chains. A code converts to
// f32 exactly, and v_mfma_f32_16x16x4_f32 is, bit for bit, acc = fmaf(a[k], b[k], acc) for k = 0, 1, 2, 3 in that
// order (tools/arith_probe.hip; ls_mq.hip rests on it). So an MFMA whose K dimension is codes 4m..4m+3 of chunk c
// advances chain (c mod L) by exactly those four fmafs: four MFMAs (m = 0..3) cover one chunk. L accumulators hold
// the L chains (GC = L: 16, or 8 for the two 8-lane geometries); the tree is L-1 vector adds in the xor tree's
// pairing. The prepared query is q' = (q * inv) * step: two separately rounded multiplies, zeros past d, inv from
// ls_wave_sumsq's order - QuerySq8::load / scale / apply_step (ls_scan_dev.h).
//
// Operand path. Lane (i = lane % 16, kq = lane / 16) loads the 16-byte chunk cb + kq of row i of the wave's 16-row
// tile (nontemporal global_load_dwordx4: the four lane groups cover 64 contiguous bytes per row, as in ls_mq). The
// MFMA wants code 4m + kq of chunk cb + j in lane group kq:
//   1. a 4 x 4 byte transpose inside the lane (8 v_perm_b32): dword b then holds codes b, 4 + b, 8 + b, 12 + b;
//   2. ls_mq's 4 x 4 transpose across the lane groups (4 lane swaps): register j of group kq then holds codes
//      4m + kq, m = 0..3 (byte m), of chunk cb + j;
//   3. one sign-extending byte-select convert per MFMA (byte m, static).
// 28 VALU instructions per 16 MFMAs and unit; no LDS round trip for the corpus.
//
// Queries: f32 in LDS, query-major; the 16 floats of a chunk are permuted so that element 4m + kq sits at 4kq + m:
// lane (li, kq) gets the four B operands (m = 0..3) of a chunk with ONE ds_read_b128 at float 16 c + 4 kq of query li.
// Pitch between two queries: the row + 32 bytes (mq8_pitch).
//
// Work deal (16-row tiles, wave-major round-robin), the static load ring pinned by sched_barrier, key lists, merge,
// emit, riding selection jobs, score vectors, qkeep: ls_mq.hip's, shared through ls_mq_dev.h / ls_select_dev.h.
// Four waves per workgroup, one B block.
#include "ls_mq_dev.h"

#include <algorithm>

typedef u32 mq8_u32x4 __attribute__((ext_vector_type(4)));

#define LS_MQ8_WAVES 4
#ifndef LS_MQ8_P
#define LS_MQ8_P 0           // variant builds: ring depth in units (0: mq8_ring)
#endif

// mq8_pitch (ls_mq_plan.h), floats between two queries in LDS: the stored row + 8 (32 bytes). ds_read_b128 is served in four groups of 16
// lanes over 16 slots of 16 bytes - lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32: a group is
// (li, kq) for li in {0-3, 12-15} and (li, kq + 1) for li in 4..11, or the other way round. A stored row is a
// multiple of 512 bytes, so with a pitch of 2 slots (mod 16) lane (li, kq) of chunk c reads slot 2 li + kq + 4 c:
// li and li + 8 share 2 li (mod 16), and exactly one of the two is in 4..11 - one takes the even slot, the other
// the odd one: 16 lanes, 16 slots, no conflict. A staging write (ds_write_b32, 32 lanes at a time over 32 banks)
// covers 32 consecutive floats of one query - two whole chunks, permuted inside each - conflict-free under any
// pitch.
// units (4 chunks = 64 bytes per row; 1 KB per wave) in flight per lane: 8 KB per wave, 6 where 8 does not divide
// the row, the whole tile where it is shorter
__host__ __device__ constexpr int mq8_ring(int nu) {
    return (LS_MQ8_P > 0 && nu % LS_MQ8_P == 0) ? LS_MQ8_P : (nu <= 8 ? nu : (nu % 8 == 0 ? 8 : 6));
}

// 4 x 4 byte transpose inside a lane: in: byte j of dword b = code 4 b + j; out: byte m of dword b = code 4 m + b.
// (v_perm_b32 picks bytes of {first operand : second operand}: selectors 0-3 the second, 4-7 the first)
__device__ __forceinline__ mq8_u32x4 mq8_byte_transpose(const mq8_u32x4& w) {
    const u32 x01 = __builtin_amdgcn_perm(w[1], w[0], 0x06020400u);  // w0.0 w1.0 w0.2 w1.2
    const u32 y01 = __builtin_amdgcn_perm(w[1], w[0], 0x07030501u);  // w0.1 w1.1 w0.3 w1.3
    const u32 x23 = __builtin_amdgcn_perm(w[3], w[2], 0x06020400u);
    const u32 y23 = __builtin_amdgcn_perm(w[3], w[2], 0x07030501u);
    mq8_u32x4 t;
    t[0] = __builtin_amdgcn_perm(x23, x01, 0x05040100u);  // w0.0 w1.0 w2.0 w3.0
    t[1] = __builtin_amdgcn_perm(y23, y01, 0x05040100u);  // w0.1 w1.1 w2.1 w3.1
    t[2] = __builtin_amdgcn_perm(x23, x01, 0x07060302u);  // w0.2 w1.2 w2.2 w3.2
    t[3] = __builtin_amdgcn_perm(y23, y01, 0x07060302u);  // w0.3 w1.3 w2.3 w3.3
    return t;
}

// 4 x 4 transpose across the four 16-lane groups (ls_mq.hip's mq_transpose on raw dwords): in: lane group g,
// register m = T[m][g]; out: register m of lane group g = T[g][m]
__device__ __forceinline__ void mq8_transpose(const mq8_u32x4& x, u32 (&r)[4]) {
    const auto a = __builtin_amdgcn_permlane32_swap(x[0], x[2], false, false);  // rows 2,3 of r0 <-> rows 0,1 of r2
    const auto b = __builtin_amdgcn_permlane32_swap(x[1], x[3], false, false);
    const auto c = __builtin_amdgcn_permlane16_swap((u32)a[0], (u32)b[0], false, false);  // odd rows <-> even rows
    const auto e = __builtin_amdgcn_permlane16_swap((u32)a[1], (u32)b[1], false, false);
    r[0] = (u32)c[0];
    r[1] = (u32)c[1];
    r[2] = (u32)e[0];
    r[3] = (u32)e[1];
}

// L lanes per row x V chunks per lane (the sq8 scan's geometry: it names the chains); M = keys per lane and query.
template <int L, int V, int M>
__global__ __launch_bounds__(64 * LS_MQ8_WAVES, 2) void ls_mq8_kernel(
    const mq8_u32x4* __restrict__ corpus, long long n, const float* __restrict__ qraw, int d, int nq,
    int normalize, float* __restrict__ S, long long s_stride, u64* __restrict__ cand, long long c_stride,
    u64* __restrict__ bound, long long b_stride, int kprime, int nfin, ls_fin_batch fin,
    void* __restrict__ gran, long long g_stride, u32 tag, float* __restrict__ qkeep,
    const float* __restrict__ step) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_dyn[];
    constexpr int WPB = LS_MQ8_WAVES;
    // the first `nfin` workgroups run selection jobs (of the previous launch, or - same-launch hand-off -
    // of this launch's own queries), exactly as in ls_scan_kernel
    if ((int)blockIdx.x < nfin) {
        for (int j = blockIdx.x; j < fin.njobs; j += nfin) {  // (nfin workgroups share the fin.njobs jobs)
            if (j != (int)blockIdx.x) __syncthreads();
            finalize_body<64 * WPB>(ls_fin_job(fin, j), smem_dyn, threadIdx.x);
        }
        return;
    }
    constexpr int CH = L * V;              // 16-byte chunks per stored row
    constexpr int NU = CH / 4;             // load units per tile (4 chunks = 64 bytes per row each)
    constexpr int GC = L;                  // chains = accumulators (16, or 8): one group
    constexpr int P = mq8_ring(NU);        // units in flight per lane (1 KB per wave each)
    constexpr int DP = mq8_pitch(CH);      // floats between two queries in LDS
    constexpr int NQT = LS_MQ_NQ;          // query columns of the launch
    static_assert((L == 8 || L == 16) && CH % 4 == 0 && NU % P == 0 && CH <= 64, "geometry");
    const int bid = (int)blockIdx.x - nfin;
    const int nblk = (int)gridDim.x - nfin;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 15, kq = lane >> 4;

    float* Bs = reinterpret_cast<float*>(smem_dyn);   // [NQT queries][DP]
    // [NQT queries][WPB waves][M] key lists, then the bounds: behind the queries (no barrier needed)
    u64* Ks = reinterpret_cast<u64*>(smem_dyn + (size_t)NQT * DP * 4);

    // tiles of 16 rows, dealt round-robin to the waves of the launch, wave-major (ls_mq.hip)
    const long long W = (long long)nblk * WPB;
    const long long NT = (n + 15) / 16;
    long long t = (long long)wave * nblk + bid;

    // unit u of a tile -> first chunk: the lane's V rounds, then 4-chunk steps (chunk c feeds chain c mod L)
    auto unit_chunk = [](int u) constexpr -> int { return L * (u / (GC / 4)) + 4 * (u % (GC / 4)); };
    auto tile_ptr = [&](long long tile) -> const mq8_u32x4* {
        // (LS_CORPUS_PAD_ROWS zero rows follow row n-1: the ragged last tile needs no clamping)
        const long long tc = tile < NT ? tile : NT - 1;  // a prefetch past the wave's last tile re-reads it
        return corpus + (tc * 16 + li) * CH + kq;
    };

    // ---- queries -> LDS: q' = (q * inv) * step, exactly the sq8 scan's prologue: canonical wave sum of squares
    // (ls_wave_sumsq's order: lane l sums x[l], x[l+64], .. by fused multiply-adds, then the xor tree 32..1), one
    // correctly rounded 1/sqrt, one multiply per element, then one more by the step (0 past d). Wave w stages queries
    // w, w + 4, ..: only the launch's REAL queries are loaded, unused columns are written as zeros. All loads of a
    // wave are issued before the first is used, in FRONT of the corpus loads (vector memory returns in order).
    constexpr int EPL = CH * 16 / 64;      // elements per lane and query
    constexpr int QPW = NQT / WPB;         // queries per wave at most
    float xq[QPW][EPL];
    float st[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
        const int e = lane + 64 * i;
        st[i] = step[e < d ? e : d - 1];   // (unconditional loads; masked below)
    }
#pragma unroll
    for (int j = 0; j < QPW; ++j) {
        const int qi = WPB * j + wave;
        if (qi < nq) {  // (wave-uniform)
            const float* src = qraw + (long long)qi * d;
#pragma unroll
            for (int i = 0; i < EPL; ++i) {
                const int e = lane + 64 * i;
                xq[j][i] = src[e < d ? e : d - 1];
            }
        } else {
#pragma unroll
            for (int i = 0; i < EPL; ++i) xq[j][i] = 0.0f;
        }
    }
    // (a launch without score vectors keeps its raw queries for the repair: workgroup b copies query b)
    if (qkeep)
        for (int qq = bid; qq < nq; qq += nblk)
            for (int e = threadIdx.x; e < d; e += 64 * WPB) qkeep[(long long)qq * d + e] = qraw[(long long)qq * d + e];
    __builtin_amdgcn_sched_barrier(0);
    mq8_u32x4 ring[P];
    {
        const mq8_u32x4* p0 = tile_ptr(t);
#pragma unroll
        for (int u = 0; u < P; ++u) ring[u] = __builtin_nontemporal_load(p0 + unit_chunk(u));
    }
    __builtin_amdgcn_sched_barrier(0);
    // element e = lane + 64 i lies in chunk 4 i + lane / 16 at position lane % 16 = 4 m + kq: stored at 4 kq + m
    const int spos = 16 * (lane >> 4) + 4 * (lane & 3) + ((lane >> 2) & 3);
#pragma unroll
    for (int i = 0; i < EPL; ++i)
        if (lane + 64 * i >= d) st[i] = 0.0f;
#pragma unroll
    for (int j = 0; j < QPW; ++j) {
        const int qi = WPB * j + wave;
        if (qi >= nq) {  // (wave-uniform) an unused column
#pragma unroll
            for (int i = 0; i < EPL; ++i) Bs[qi * DP + lane + 64 * i] = 0.0f;
            continue;
        }
#pragma unroll
        for (int i = 0; i < EPL; ++i)
            if (lane + 64 * i >= d) xq[j][i] = 0.0f;
        float inv = 1.0f;
        if (normalize) {
            float ss = 0.0f;
#pragma unroll
            for (int i = 0; i < EPL; ++i) ss = fmaf(xq[j][i], xq[j][i], ss);  // (zeros past d add nothing)
            ss = ls_wave_xor_sum(ss);
            if (ss > 0.0f) inv = 1.0f / sqrtf(ss);
        }
#pragma unroll
        for (int i = 0; i < EPL; ++i) Bs[qi * DP + 64 * i + spos] = (xq[j][i] * inv) * st[i];  // (two rounded multiplies)
    }
    __syncthreads();

    // this lane's best rows (query li; rows 4kq.. of the wave's tiles), best first (mq_take_scores)
    float bs[1][M];
    u32 br[1][M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
        bs[0][i] = -FLT_MAX;
        br[0][i] = 0u;
    }

    while (t < NT) {
        const mq8_u32x4* pcur = tile_ptr(t);
        const mq8_u32x4* pnext = tile_ptr(t + W);
        mq_f32x4 acc[GC];
        // (the B fragments do not change from tile to tile: left alone, the compiler hoists all CH reads out of this
        // loop and spills them. An opaque copy of the lane's OFFSET per tile keeps every ds_read_b128 in front of its
        // MFMAs - the offset, not the pointer: an opaque pointer loses its LDS address space (ls_mq.hip).)
        int boff = li * DP + 4 * kq;
        asm volatile("" : "+v"(boff));
        const float* bf = Bs + boff;
#pragma unroll NU
        for (int u = 0; u < NU; ++u) {
            const mq8_u32x4 x = ring[u % P];
            // refill the slot: a later unit of this tile, or the head of the wave's next tile
            ring[u % P] = __builtin_nontemporal_load(u + P < NU ? pcur + unit_chunk(u + P) : pnext + unit_chunk(u + P - NU));
            // Nothing moves across this point: left alone, the scheduler sinks every refill down to its first use,
            // the waits become vmcnt(0) and each unit pays a full memory round trip (ls_mq.hip, same place)
            __builtin_amdgcn_sched_barrier(0);
            u32 a[4];
            mq8_transpose(mq8_byte_transpose(x), a);
            const int cb = unit_chunk(u);
            const int v = u / (GC / 4), j4 = u % (GC / 4);
            // chunk cb + j feeds chain 4 j4 + j. The four chains advance in step - m outside, j inside: every chain still
            // takes its codes 4m..4m+3 (k = kq) for m = 0, 1, 2, 3 in memory order, and no MFMA waits for the one
            // issued just before it
            mq_f32x4 bv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = *reinterpret_cast<const mq_f32x4*>(bf + 16 * (cb + j));
#pragma unroll
            for (int m = 0; m < 4; ++m) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    mq_f32x4 c;
                    if (v == 0 && m == 0) {
                        c[0] = 0.0f; c[1] = 0.0f; c[2] = 0.0f; c[3] = 0.0f;
                    } else {
                        c = acc[4 * j4 + j];
                    }
                    const float av = (float)(signed char)(a[j] >> (8 * m));
                    acc[4 * j4 + j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[j][m], c, 0, 0, 0);
                }
            }
        }
        // the chains are complete: xor tree 1, 2, 4 (, 8)
#pragma unroll
        for (int o = 1; o < GC; o <<= 1)
#pragma unroll
            for (int i = 0; i < GC; i += 2 * o) acc[i] = acc[i] + acc[i + o];

        const long long row0 = t * 16 + 4 * kq;  // rows t*16 + 4kq + 0..3 of query li: score vectors, key lists
        mq_take_scores<M>(acc[0], li, nq, S, s_stride, row0, t, n, bs[0], br[0]);
        t += W;
    }

    // ---- merge in registers, then in LDS; the workgroup emits its best k' keys + bound (ls_mq_dev.h)
    mq_merge_lists<M, 1, WPB>(bs, br, Ks, nq, lane, wave);
    __syncthreads();
    mq_rank_emit<M, 1, WPB>(Ks, nq, kprime, cand, c_stride, bound, b_stride, gran, g_stride, tag, bid, nblk);
}

#ifndef LS_MQ8_KERNEL_ONLY  // (scratch builds that instantiate a kernel or two and look at their resources / ISA)
#include "ls_mq_launch.h"
// ---- host side ------------------------------------------------------------------------------------
// a.nq = the real query count (1..16); a.blocks / a.kprime / a.mq_keys: ls_mq_make_plan (LS_MQ_SQ8); a.d_step set. The
// sq8 row lengths up to 64 chunks: 16 queries of 1 KB rows + their key lists stay under LS_PIGGY_LDS_MAX, like a riding
// selection job.
int ls_launch_mq8(const void* d_corpus, int64_t n, const ls_geom& g, const ls_scan_args& a, hipStream_t s) {
    if (n <= 0) return LS_OK;
    if (!ls_mq_args_ok(g, a, 1, LS_MQ_NQ, LS_MQ8_WAVES) || !a.d_step) {
        ls_set_error("ls_launch_mq8: bad arguments (elem %d nq %d blocks %d kprime %d keys %d)", g.elem, a.nq, a.blocks,
                     a.kprime, a.mq_keys);
        return LS_ERR_INVALID_ARG;
    }
    return ls_geom_dispatch<true, false>("ls_launch_mq8", g, [&](auto l, auto v) {
        return ls_mq_dispatch<false>(a, [&](auto m, auto) {
            constexpr int L = decltype(l)::value, V = decltype(v)::value, M = decltype(m)::value;
            return ls_mq_launch<ls_mq8_kernel<L, V, M>>("ls_launch_mq8", LS_MQ8_WAVES, mq8_lds_bytes(g.chunks, M),
                                                        LS_PIGGY_LDS_MAX, (const mq8_u32x4*)d_corpus, n, g, a, s, a.d_step);
        });
    });
}
#else
#ifndef LS_MQ8_ONLY_L
#define LS_MQ8_ONLY_L 8
#endif
#ifndef LS_MQ8_ONLY_V
#define LS_MQ8_ONLY_V 3
#endif
template __global__ void ls_mq8_kernel<LS_MQ8_ONLY_L, LS_MQ8_ONLY_V, 3>(const mq8_u32x4*, long long, const float*, int, int, int,
                                                                        float*, long long, u64*, long long, u64*, long long,
                                                                        int, int, ls_fin_batch, void*, long long, u32, float*,
                                                                        const float*);
template __global__ void ls_mq8_kernel<LS_MQ8_ONLY_L, LS_MQ8_ONLY_V, 8>(const mq8_u32x4*, long long, const float*, int, int, int,
                                                                        float*, long long, u64*, long long, u64*, long long,
                                                                        int, int, ls_fin_batch, void*, long long, u32, float*,
                                                                        const float*);
#endif  // LS_MQ8_KERNEL_ONLY
