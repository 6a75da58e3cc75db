// ls_mq16.hip — small batches on an fp16 index (opt-in: ls_set_f16_small_batch): 1..32 queries share ONE pass over
// the corpus, the inner products on the f16 matrix cores (v_mfma_f32_16x16x32_f16). ls_mq.hip's fp16 sibling.
//
// Replaces faiss `index.search(x, k)` (reference src/lean_explore/search/engine.py:238-250) for what an fp16 index
// served on the VALU scan in groups of 8 / 4 / 1 queries: concurrent callers combined by ls_search, small explicit
// batches, and every re-serve (retry / repair) of those and of the batched path.
//
// Roofline: HBM (or the Infinity Cache where the corpus fits it). One pass reads n x row bytes once; one MFMA
// consumes 1 KB of corpus per wave (16 rows x 64 bytes) against 16 query columns in 8 passes of the matrix pipe:
// N = 200 k, d = 384 (153.6 MB) is 150 k MFMAs per block of 16 queries, ~1 us over 1024 SIMDs. The VALU work is the
// key lists only (4 rows x M compare-exchange steps per tile and block).
//
// Operand path. For v_mfma_f32_16x16x32_f16 lane (i = lane % 16, kq = lane / 16) supplies A[row i][k = 8 kq .. 8 kq + 7]:
// eight consecutive halves of one row - exactly one 16-byte chunk of the stored row. So the lane LOADS its operand:
// chunk 4 u + kq of row i of the wave's 16-row tile is the A register group of K-step u, with no lane transpose
// (ls_mq.hip spends four swaps per unit on it) and no LDS round trip for the corpus. The four lane groups cover 64
// contiguous bytes per row and step. The loads (nontemporal, 16 bytes) stream through a static ring of P units
// (1 KB per wave each) that continues into the wave's next tile; the waits are counted. (Measured and removed: the
// same ring through buffer loads - a scalar descriptor per tile, the nontemporal policy on every load - was 12-17 %
// slower at every shape: docs/EXPERIMENTS.md.)
//
// Queries: normalised exactly like ls_scan.hip / ls_mq.hip (ls_wave_sumsq's order, one correctly rounded 1/sqrt,
// one multiply per element), rounded to fp16 (LS_DTYPE_F16: both operands fp16) and kept in LDS as halves,
// query-major. The B fragment of lane (query li, kq) at step u is the query's chunk 4 u + kq: one ds_read_b128.
// Pitch between two queries: the row + 16 bytes (mq16_pitch).
//
// Arithmetic order - the invariant (tests/test_mq16_gpu.py). A row's score is ONE fp32 accumulator: zero, then
// acc = MFMA(A_u, B_u, acc) for u = 0, 1, 2, .. in memory order; what the instruction does inside a step is the
// hardware's, the same for every lane, column and launch. Nothing else is added: the second B block has its own
// accumulator, no chains are interleaved (the dependent chain of 12 (d = 384) .. 64 MFMAs per tile is far under the
// time the tile's bytes take to arrive). So a score depends on the row and the query only - not on the number of
// queries in the launch, the column, one or two B blocks, the tile, wave or workgroup count, or on whether score
// vectors are written.
//
// Work deal, key lists, merge, emit, riding selection jobs, score vectors, qkeep: ls_mq.hip's, shared through
// ls_mq_dev.h. Always four waves per workgroup - also with two B blocks: the matrix pipe is nearly idle here, so the
// eight-wave form ls_mq needs (to fill MFMA issue gaps) has nothing to give and the launch geometry, the key-list
// plan and k' stay the same for every query count.
#include "ls_mq_dev.h"

#include <algorithm>

typedef _Float16 mq16_h8 __attribute__((ext_vector_type(8)));

#define LS_MQ16_WAVES 4
#ifndef LS_MQ16_P
#define LS_MQ16_P 0          // variant builds: ring depth in units (0: mq16_ring)
#endif

// mq16_pitch (ls_mq_plan.h), bytes between two queries in LDS: the stored row + 16. Stored rows are multiples of 256 bytes, so query li's chunk
// c lies in 16-byte slot (li + c) mod 16 of the 256-byte bank row. ds_read_b128 is served in four groups of 16 lanes
// (lanes 0-3, 12-15, 20-27 | 4-11, 16-19, 28-31 | ..): a group's reads are (li, kq = 0) for eight queries and
// (li, kq = 1) for the other eight: slots li + kq - fifteen distinct slots, one met twice: 2-way on one slot (5 LDS
// cycles instead of 4). The staging writes are 128 contiguous bytes per instruction.
// units (K-steps of 4 chunks; 1 KB per wave) in flight per lane: 8 KB per wave, 6 where 8 does not divide the row
__host__ __device__ constexpr int mq16_ring(int nu) {
    return (LS_MQ16_P > 0 && nu % LS_MQ16_P == 0) ? LS_MQ16_P : (nu <= 8 ? nu : (nu % 8 == 0 ? 8 : 6));
}

// queries a wave loads at a time while staging: the largest power of two with at most 64 registers of elements
__host__ __device__ constexpr int mq16_query_batch(int epl, int qpw) {
    int jb = 1;
    while (2 * jb <= qpw && 2 * jb * epl <= 64) jb *= 2;
    return jb;
}

// CH = 16-byte chunks per stored row; M = keys per lane and query; NB = MFMA B blocks (16 query columns each).
template <int CH, int M, int NB>
__global__ __launch_bounds__(64 * LS_MQ16_WAVES, 2) void ls_mq16_kernel(
    const mq16_h8* __restrict__ corpus, long long n, const float* __restrict__ qraw, int d, int nq,
    int normalize, float* __restrict__ S, long long s_stride, u64* __restrict__ cand, long long c_stride,
    u64* __restrict__ bound, long long b_stride, int kprime, int nfin, ls_fin_batch fin,
    void* __restrict__ gran, long long g_stride, u32 tag, float* __restrict__ qkeep) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_dyn[];
    constexpr int WPB = LS_MQ16_WAVES;
    // the first `nfin` workgroups run selection jobs (of the previous launch, or - same-launch hand-off -
    // of this launch's own queries), exactly as in ls_scan_kernel
    if ((int)blockIdx.x < nfin) {
        for (int j = blockIdx.x; j < fin.njobs; j += nfin) {  // (nfin workgroups share the fin.njobs jobs)
            if (j != (int)blockIdx.x) __syncthreads();
            finalize_body<64 * WPB>(ls_fin_job(fin, j), smem_dyn, threadIdx.x);
        }
        return;
    }
    constexpr int NU = CH / 4;             // K-steps per tile: 4 chunks = 32 halves = 64 bytes per row each
    constexpr int P = mq16_ring(NU);       // units in flight per lane
    constexpr int PB = mq16_pitch(CH);     // bytes between two queries in LDS
    constexpr int NQT = NB * LS_MQ_NQ;     // query columns of the launch
    static_assert(CH % 8 == 0 && NU % P == 0, "geometry");
    const int bid = (int)blockIdx.x - nfin;
    const int nblk = (int)gridDim.x - nfin;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 15, kq = lane >> 4;

    unsigned char* Bs = smem_dyn;          // [NQT queries][PB bytes]
    // [NQT queries][WPB waves][M] key lists, then the bounds. Two blocks: over the queries, once every wave is through
    // its tiles; one block: behind them (no barrier needed)
    u64* Ks = reinterpret_cast<u64*>(smem_dyn + (NB == 1 ? (size_t)NQT * PB : 0));

    // tiles of 16 rows, dealt round-robin to the waves of the launch, wave-major (ls_mq.hip)
    const long long W = (long long)nblk * WPB;
    const long long NT = (n + 15) / 16;
    long long t = (long long)wave * nblk + bid;
    auto tile_ptr = [&](long long tile) -> const mq16_h8* {
        // (LS_CORPUS_PAD_ROWS zero rows follow row n-1: the ragged last tile needs no clamping)
        const long long tc = tile < NT ? tile : NT - 1;  // a prefetch past the wave's last tile re-reads it
        return corpus + (tc * 16 + li) * CH + kq;
    };

    // ---- queries -> LDS as halves; normalised as in ls_scan_kernel / ls_mq_kernel: lane l sums x[l], x[l+64], .. by
    // fused multiply-adds, then the xor tree 32..1 (ls_wave_sumsq's order), one correctly rounded 1/sqrt, one multiply
    // per element, then the rounding to fp16. Wave w stages queries w, w + 4, ..: only the launch's REAL queries are
    // loaded, unused columns are written as zeros (a live query's row padding is zero too). The loads go out JB queries
    // at a time (<= 64 registers), the first batch in FRONT of the corpus loads: vector memory returns in order.
    constexpr int EPL = CH * 8 / 64;       // elements per lane and query
    constexpr int QPW = NQT / WPB;         // queries per wave at most
    constexpr int JB = mq16_query_batch(EPL, QPW);
    static_assert(QPW % JB == 0, "query batches");
    // (a launch without score vectors keeps its raw queries for the repair: workgroup b copies query b)
    if (qkeep)
        for (int qq = bid; qq < nq; qq += nblk)
            for (int e = threadIdx.x; e < d; e += 64 * WPB) qkeep[(long long)qq * d + e] = qraw[(long long)qq * d + e];
    mq16_h8 ring[P];
#pragma unroll
    for (int j0 = 0; j0 < QPW; j0 += JB) {
        float xq[JB][EPL];
#pragma unroll
        for (int j = 0; j < JB; ++j) {
            const int qi = WPB * (j0 + j) + wave;
            if (qi < nq) {  // (wave-uniform)
                const float* src = qraw + (long long)qi * d;
#pragma unroll
                for (int i = 0; i < EPL; ++i) {
                    const int e = lane + 64 * i;
                    xq[j][i] = src[e < d ? e : d - 1];  // (unconditional loads; masked below)
                }
            } else {
#pragma unroll
                for (int i = 0; i < EPL; ++i) xq[j][i] = 0.0f;
            }
        }
        if (j0 == 0) {
            __builtin_amdgcn_sched_barrier(0);
            const mq16_h8* p0 = tile_ptr(t);
#pragma unroll
            for (int u = 0; u < P; ++u) ring[u] = __builtin_nontemporal_load(p0 + 4 * u);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int j = 0; j < JB; ++j) {
            const int qi = WPB * (j0 + j) + wave;
            _Float16* dst = reinterpret_cast<_Float16*>(Bs + qi * PB);
            if (qi >= nq) {  // (wave-uniform) an unused column
#pragma unroll
                for (int i = 0; i < EPL; ++i) dst[lane + 64 * i] = (_Float16)0.0f;
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
            for (int i = 0; i < EPL; ++i) dst[lane + 64 * i] = (_Float16)(xq[j][i] * inv);
        }
    }
    __syncthreads();

    // this lane's best rows (queries li, 16 + li; rows 4kq.. of the wave's tiles), best first (mq_take_scores)
    float bs[NB][M];
    u32 br[NB][M];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < M; ++i) {
            bs[b][i] = -FLT_MAX;
            br[b][i] = 0u;
        }

    while (t < NT) {
        const mq16_h8* pcur = tile_ptr(t);
        const mq16_h8* pnext = tile_ptr(t + W);
        mq_f32x4 acc[NB];
        // (the B fragments do not change from tile to tile: left alone, the compiler hoists all reads out of this
        // loop and spills them. An opaque copy of the lane's byte OFFSET per tile keeps every ds_read_b128 in front of
        // its MFMA - the offset, not the pointer: an opaque pointer loses its LDS address space (ls_mq.hip).
        // One base per B block: block 1 lies 16 x PB bytes up, past the 64 KB an offset field reaches for 4 KB rows.)
        const unsigned char* bf[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            int boff = (b * LS_MQ_NQ + li) * PB + kq * 16;
            asm volatile("" : "+v"(boff));
            bf[b] = Bs + boff;
        }
#pragma unroll NU
        for (int u = 0; u < NU; ++u) {
            const mq16_h8 a = ring[u % P];
            // refill the slot: a later unit of this tile, or the head of the wave's next tile
            if (u + P < NU)
                ring[u % P] = __builtin_nontemporal_load(pcur + 4 * (u + P));
            else
                ring[u % P] = __builtin_nontemporal_load(pnext + 4 * (u + P - NU));
            // Nothing moves across this point: left alone, the scheduler sinks every refill down to its first use,
            // the waits become vmcnt(0) and each unit pays a full memory round trip (ls_mq.hip, same place)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const mq16_h8 bv = *reinterpret_cast<const mq16_h8*>(bf[b] + 64 * u);
                mq_f32x4 c;
                if (u == 0) {
                    c[0] = 0.0f; c[1] = 0.0f; c[2] = 0.0f; c[3] = 0.0f;
                } else {
                    c = acc[b];
                }
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bv, c, 0, 0, 0);  // the row's ONE chain, step u
            }
        }
        const long long row0 = t * 16 + 4 * kq;
#pragma unroll
        for (int b = 0; b < NB; ++b)  // rows t*16 + 4kq + 0..3 of query 16 b + li: score vectors, key lists
            mq_take_scores<M>(acc[b], LS_MQ_NQ * b + li, nq, S, s_stride, row0, t, n, bs[b], br[b]);
        t += W;
    }

    // ---- merge in registers, then in LDS; the workgroup emits its best k' keys + bound (ls_mq_dev.h)
    if (NB == 2) __syncthreads();        // (the key lists overwrite the queries: every wave is through its tiles)
    mq_merge_lists<M, NB, WPB>(bs, br, Ks, nq, lane, wave);
    __syncthreads();
    mq_rank_emit<M, NB, WPB>(Ks, nq, kprime, cand, c_stride, bound, b_stride, gran, g_stride, tag, bid, nblk);
}

#ifndef LS_MQ16_KERNEL_ONLY  // (scratch builds that instantiate a kernel or two and look at their resources / ISA)
#include "ls_mq_launch.h"
// ---- host side ------------------------------------------------------------------------------------
// a.nq = the real query count (1..32); a.blocks / a.kprime / a.mq_keys: ls_mq_make_plan for that count. The kernel is
// instantiated by row length: the fp16 geometries of ls_pick_geom are exactly the stored lengths 16..256 chunks = L x V.
// One block: 16 queries of 4 KB rows + their key lists stay under LS_PIGGY_LDS_MAX, like a riding selection job.
int ls_launch_mq16(const void* d_corpus, int64_t n, const ls_geom& g, const ls_scan_args& a, hipStream_t s) {
    if (n <= 0) return LS_OK;
    if (!ls_mq_args_ok(g, a, 2, 2 * LS_MQ_NQ, LS_MQ16_WAVES)) {
        ls_set_error("ls_launch_mq16: bad arguments (elem %d nq %d blocks %d kprime %d keys %d)", g.elem, a.nq, a.blocks,
                     a.kprime, a.mq_keys);
        return LS_ERR_INVALID_ARG;
    }
    if (g.chunks != g.L * g.V) {
        ls_set_error("ls_launch_mq16: unsupported row length (%d chunks)", g.chunks);
        return LS_ERR_INVALID_ARG;
    }
    return ls_geom_dispatch<false, true>("ls_launch_mq16", g, [&](auto l, auto v) {
        return ls_mq_dispatch<true>(a, [&](auto m, auto nb) {
            constexpr int CH = decltype(l)::value * decltype(v)::value, M = decltype(m)::value, NB = decltype(nb)::value;
            return ls_mq_launch<ls_mq16_kernel<CH, M, NB>>("ls_launch_mq16", LS_MQ16_WAVES, mq16_lds_bytes(g.chunks, M, NB),
                                                           NB == 1 ? LS_PIGGY_LDS_MAX : LS_MQ16_LDS_MAX2,
                                                           (const mq16_h8*)d_corpus, n, g, a, s);
        });
    });
}
#else
#ifndef LS_MQ16_ONLY_CH
#define LS_MQ16_ONLY_CH 48
#endif
template __global__ void ls_mq16_kernel<LS_MQ16_ONLY_CH, 3, 1>(const mq16_h8*, long long, const float*, int, int, int, float*,
                                                              long long, u64*, long long, u64*, long long, int, int,
                                                              ls_fin_batch, void*, long long, u32, float*);
template __global__ void ls_mq16_kernel<LS_MQ16_ONLY_CH, 8, 2>(const mq16_h8*, long long, const float*, int, int, int, float*,
                                                              long long, u64*, long long, u64*, long long, int, int,
                                                              ls_fin_batch, void*, long long, u32, float*);
#endif  // LS_MQ16_KERNEL_ONLY
