// ls_scan_dev.h — device code the row scans share: the query registers with their per-lane fmaf / fdot2 chain (dot),
// the xor tree over the L lanes of a row (group_sum) and the score hand-out (pick_group). ls_scan.hip (plain and
// row-list scan) and ls_ivf.hip (probed-list scan) call the SAME functions of the same (F16, L, V): that is what makes
// a row's score bit-identical on every one of them. The sq8 kernels (ls_sq8_scan.hip, ls_sq8_ivf.hip) are the same
// templates with QuerySq8 in QueryRegs' place.
#pragma once
#include "ls_select_dev.h"

#include <hip/hip_fp16.h>

#include <algorithm>
#include <type_traits>

typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));  // one 16-byte chunk

// NOTE: never __builtin_bit_cast an ext-vector ELEMENT expression (x.y): clang reads the first
// lane. Copy the element to a scalar first.
__device__ __forceinline__ h2_t as_h2(float f) { return __builtin_bit_cast(h2_t, f); }

template <bool F16, int V>
struct QueryRegs;

template <int V>
struct QueryRegs<false, V> {
    static constexpr int SMALL_PF = 4;  // tile buffers of a SMALL launch (ls_scan_kernel.h)
    float4 q[V];
    // raw query (d floats, any alignment) -> zero-padded registers; returns this lane's sum of squares
    __device__ __forceinline__ float load(const float* qp, int d, int sub, int L) {
        float ss = 0.0f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int e = 4 * (sub + L * v);
            q[v].x = e + 0 < d ? qp[e + 0] : 0.0f;
            q[v].y = e + 1 < d ? qp[e + 1] : 0.0f;
            q[v].z = e + 2 < d ? qp[e + 2] : 0.0f;
            q[v].w = e + 3 < d ? qp[e + 3] : 0.0f;
            ss = fmaf(q[v].x, q[v].x, ss);
            ss = fmaf(q[v].y, q[v].y, ss);
            ss = fmaf(q[v].z, q[v].z, ss);
            ss = fmaf(q[v].w, q[v].w, ss);
        }
        return ss;
    }
    __device__ __forceinline__ void scale(float f) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            q[v].x *= f; q[v].y *= f; q[v].z *= f; q[v].w *= f;
        }
    }
    __device__ __forceinline__ float dot(const f32x4 (&x)[V]) const {
        float acc = 0.0f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float a = x[v].x, b = x[v].y, c = x[v].z, e = x[v].w;
            acc = fmaf(a, q[v].x, acc);
            acc = fmaf(b, q[v].y, acc);
            acc = fmaf(c, q[v].z, acc);
            acc = fmaf(e, q[v].w, acc);
        }
        return acc;
    }
};

template <int V>
struct QueryRegs<true, V> {
    static constexpr int SMALL_PF = 4;
    h2_t q[V][4];
    float f[V][8];  // fp32 staging, dead after scale()
    __device__ __forceinline__ float load(const float* qp, int d, int sub, int L) {
        float ss = 0.0f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int e = 8 * (sub + L * v);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                f[v][j] = e + j < d ? qp[e + j] : 0.0f;
                ss = fmaf(f[v][j], f[v][j], ss);
            }
        }
        return ss;
    }
    // scale, then round the query to fp16 (LS_DTYPE_F16 semantics: both operands are fp16)
    __device__ __forceinline__ void scale(float s) {
#pragma unroll
        for (int v = 0; v < V; ++v)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                q[v][j] = h2_t{(_Float16)(f[v][2 * j] * s), (_Float16)(f[v][2 * j + 1] * s)};
    }
    __device__ __forceinline__ float dot(const f32x4 (&x)[V]) const {
        float acc = 0.0f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float a = x[v].x, b = x[v].y, c = x[v].z, e = x[v].w;
            acc = __builtin_amdgcn_fdot2(as_h2(a), q[v][0], acc, false);
            acc = __builtin_amdgcn_fdot2(as_h2(b), q[v][1], acc, false);
            acc = __builtin_amdgcn_fdot2(as_h2(c), q[v][2], acc, false);
            acc = __builtin_amdgcn_fdot2(as_h2(e), q[v][3], acc, false);
        }
        return acc;
    }
};

// ---- LS_DTYPE_SQ8: a 16-byte chunk holds 16 int8 codes; the query stays f32, pre-multiplied by the
// per-dimension step: q'_i = (q_i * inv) * step_i, two rounded multiplies. A code converts to f32 exactly, so a lane's
// partial sum is ONE fmaf chain over exact operands, in memory order (tests/sq8_ref.c restates it).
// The kernels take the step vector as a trailing argument of this type: the scan and IVF kernel templates end in a
// parameter pack, and a pack that holds it selects QuerySq8 (the f32 / fp16 instantiations never see it).
struct ls_sq8_arg {
    const float* p;  // [d]
};
template <typename... X>
struct ls_pack_sq8 : std::bool_constant<(std::is_same_v<X, ls_sq8_arg> || ...)> {};
__device__ __forceinline__ const float* ls_pack_step() { return nullptr; }
template <typename X0, typename... X>
__device__ __forceinline__ const float* ls_pack_step(X0 x0, X... x) {
    if constexpr (std::is_same_v<X0, ls_sq8_arg>) return x0.p;
    else return ls_pack_step(x...);
}
template <int V>
struct QuerySq8 {
    // SMALL keeps SMALL_PF tiles in flight: next to 16 * V query registers there is room for four tiles of 1-chunk
    // lanes, two of 2- and 3-chunk lanes, one of 4-chunk lanes (two spilled 80-144 bytes per lane)
    static constexpr int SMALL_PF = V == 1 ? 4 : (V == 4 ? 1 : 2);
    float q[V][16];
    __device__ __forceinline__ float load(const float* qp, int d, int sub, int L) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int e = 16 * (sub + L * v);
#pragma unroll
            for (int j = 0; j < 16; ++j) q[v][j] = e + j < d ? qp[e + j] : 0.0f;
        }
        return 0.0f;
    }
    __device__ __forceinline__ void scale(float f) {
#pragma unroll
        for (int v = 0; v < V; ++v)
#pragma unroll
            for (int j = 0; j < 16; ++j) q[v][j] *= f;
    }
    __device__ __forceinline__ void apply_step(const float* step, int d, int sub, int L) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int e = 16 * (sub + L * v);
#pragma unroll
            for (int j = 0; j < 16; ++j) q[v][j] *= e + j < d ? step[e + j] : 0.0f;
        }
    }
    __device__ __forceinline__ float dot(const f32x4 (&x)[V]) const {
        float acc = 0.0f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float a = x[v].x, b = x[v].y, c = x[v].z, e = x[v].w;
            int w[4] = {__builtin_bit_cast(int, a), __builtin_bit_cast(int, b), __builtin_bit_cast(int, c),
                        __builtin_bit_cast(int, e)};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                asm("" : "+v"(w[i]));  // (see dot_tile)
#pragma unroll
                for (int j = 0; j < 4; ++j)  // byte j of word i: code 4 * i + j of the chunk (sign-extending convert)
                    acc = fmaf((float)(signed char)(w[i] >> (8 * j)), q[v][4 * i + j], acc);
            }
        }
        return acc;
    }
    // dot() of the U rows of a tile, the U chains advancing in step (each chain is dot()'s, term by term: the same
    // bits). Written code by code so that only U converted codes are live at a time: left to itself the scheduler
    // converts a whole tile (16 * V * U floats) ahead of the chains.
    template <int U>
    __device__ __forceinline__ void dot_tile(const f32x4 (&x)[U][V], float (&acc)[U]) const {
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = 0.0f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int w[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const float f = i == 0 ? x[u][v].x : (i == 1 ? x[u][v].y : (i == 2 ? x[u][v].z : x[u][v].w));
                    w[u] = __builtin_bit_cast(int, f);
                    // (the word becomes opaque here: otherwise its four shifted copies are computed as soon as the
                    // load lands and carried - four registers for one - until the chain gets to them)
                    asm("" : "+v"(w[u]));
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        acc[u] = fmaf((float)(signed char)(w[u] >> (8 * j)), q[v][4 * i + j], acc[u]);
                }
            }
        }
    }
};
// ---- LS_METRIC_L2 (include/leansearch_l2.h): the same rows, the same lanes, another arithmetic. A lane's
// partial sum is ONE chain from 0 over its elements in memory order: t = x_i - q_i (one rounded f32 subtraction), then
// acc = fmaf(t, t, acc); the kernel negates the row's sum once, after group_sum (tests/l2_ref.c restates it). An empty
// tag type at the end of the kernel's pack (after the row list, if any) selects QueryL2.
struct ls_l2_arg {};
template <typename... X>
struct ls_pack_l2 : std::bool_constant<(std::is_same_v<X, ls_l2_arg> || ...)> {};

template <bool F16, int V>
struct QueryL2;

template <int V>
struct QueryL2<false, V> {
    static constexpr int SMALL_PF = 4;
    float4 q[V];
    __device__ __forceinline__ float load(const float* qp, int d, int sub, int L) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int e = 4 * (sub + L * v);
            q[v].x = e + 0 < d ? qp[e + 0] : 0.0f;
            q[v].y = e + 1 < d ? qp[e + 1] : 0.0f;
            q[v].z = e + 2 < d ? qp[e + 2] : 0.0f;
            q[v].w = e + 3 < d ? qp[e + 3] : 0.0f;
        }
        return 0.0f;
    }
    // q_i * f as a ROUNDED value: the build contracts across statements (-ffp-contract=fast), and x - q * f must not
    // become fma(-q, f, x). The product is made opaque before anything can subtract it.
    __device__ __forceinline__ void scale(float f) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float a = q[v].x * f, b = q[v].y * f, c = q[v].z * f, e = q[v].w * f;
            asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(e));
            q[v].x = a; q[v].y = b; q[v].z = c; q[v].w = e;
        }
    }
    __device__ __forceinline__ float dot(const f32x4 (&x)[V]) const {
        float acc = 0.0f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float a = x[v].x - q[v].x, b = x[v].y - q[v].y, c = x[v].z - q[v].z, e = x[v].w - q[v].w;
            acc = fmaf(a, a, acc);
            acc = fmaf(b, b, acc);
            acc = fmaf(c, c, acc);
            acc = fmaf(e, e, acc);
        }
        return acc;
    }
};

template <int V>
struct QueryL2<true, V> {
    static constexpr int SMALL_PF = 4;
    float q[V][8];  // raw, then (scale) scaled, rounded to fp16 and widened again: exact f32 copies of the fp16 query
    __device__ __forceinline__ float load(const float* qp, int d, int sub, int L) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int e = 8 * (sub + L * v);
#pragma unroll
            for (int j = 0; j < 8; ++j) q[v][j] = e + j < d ? qp[e + j] : 0.0f;
        }
        return 0.0f;
    }
    __device__ __forceinline__ void scale(float s) {
#pragma unroll
        for (int v = 0; v < V; ++v)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                float p = q[v][j] * s;  // a rounded f32 product, THEN the conversion: the barrier keeps the two from
                asm volatile("" : "+v"(p));  // being selected as one mixed-precision instruction
                q[v][j] = (float)(_Float16)p;
            }
    }
    __device__ __forceinline__ float dot(const f32x4 (&x)[V]) const {
        float acc = 0.0f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float w[4] = {x[v].x, x[v].y, x[v].z, x[v].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const h2_t h = as_h2(w[i]);
                const float a = (float)h.x - q[v][2 * i], b = (float)h.y - q[v][2 * i + 1];
                acc = fmaf(a, a, acc);
                acc = fmaf(b, b, acc);
            }
        }
        return acc;
    }
};

// ---- several L2 queries per corpus pass (include/leansearch_l2_batch.h): TWO queries' chains advance
// together as float2 operations, t2 = {x, x} - {q_a, q_b}, acc2 = fma(t2, t2, acc2) (v_pk_add_f32 with negation,
// v_pk_fma_f32). Each half is the IEEE operation of QueryL2::dot on the same operands in the same order, so a query's
// partial sum is QueryL2's bit for bit. Registers per query: 4 * V, the inner product's figure - f32 as {q_a, q_b}
// pairs, fp16 as one register of two halves {q_a, q_b} per element (widened at use; QueryL2<true, V>'s widened copy
// would take 8 * V). prepare() is QueryL2's load() and scale() per element: the product q_i * inv is rounded to f32
// behind the same barrier, then (fp16) rounded once to fp16.
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <bool F16, int V>
struct QueryL2Pair;

template <int V>
struct QueryL2Pair<false, V> {
    f32x2 q[V][4];
    __device__ __forceinline__ void prepare(const float* qa, const float* qb, float inva, float invb, int d, int sub, int L) {
#pragma unroll
        for (int v = 0; v < V; ++v)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = 4 * (sub + L * v) + j;
                float a = (e < d ? qa[e] : 0.0f) * inva, b = (e < d ? qb[e] : 0.0f) * invb;
                asm volatile("" : "+v"(a), "+v"(b));  // (rounded products: see QueryL2<false, V>::scale)
                q[v][j] = f32x2{a, b};
            }
    }
    __device__ __forceinline__ void dot(const f32x4 (&x)[V], float& sa, float& sb) const {
        f32x2 acc = {0.0f, 0.0f};
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float w[4] = {x[v].x, x[v].y, x[v].z, x[v].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x2 t = f32x2{w[j], w[j]} - q[v][j];
                acc = __builtin_elementwise_fma(t, t, acc);
            }
        }
        sa = acc.x;
        sb = acc.y;
    }
};

template <int V>
struct QueryL2Pair<true, V> {
    h2_t q[V][8];  // element j of the chunk: {q_a, q_b}, scaled and rounded to fp16
    __device__ __forceinline__ void prepare(const float* qa, const float* qb, float inva, float invb, int d, int sub, int L) {
#pragma unroll
        for (int v = 0; v < V; ++v)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int e = 8 * (sub + L * v) + j;
                float a = (e < d ? qa[e] : 0.0f) * inva, b = (e < d ? qb[e] : 0.0f) * invb;
                asm volatile("" : "+v"(a), "+v"(b));  // (a rounded f32 product, THEN the conversion: QueryL2<true, V>::scale)
                q[v][j] = h2_t{(_Float16)a, (_Float16)b};
            }
    }
    __device__ __forceinline__ void dot(const f32x4 (&x)[V], float& sa, float& sb) const {
        f32x2 acc = {0.0f, 0.0f};
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float w[4] = {x[v].x, x[v].y, x[v].z, x[v].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const h2_t h = as_h2(w[i]);
                // (the row's widened halves are common to every pair of the launch: the compiler converts them once)
                const float xe[2] = {(float)h.x, (float)h.y};
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    // The query halves are widened HERE, at every use: written as plain conversions they are loop
                    // invariants, hoisted out of the tile loop into 8 * V registers per query (8 queries of 3-chunk
                    // lanes: 1200 bytes of scratch per lane). v_cvt_f32_f16 is exact, the conversion the compiler emits.
                    // The statement names the chain's accumulator as well (untouched): the widening then sits between
                    // this chain's previous step and this one, and the scheduler cannot widen a whole query up front.
                    const u32 qh = __builtin_bit_cast(u32, q[v][2 * i + j]);
                    f32x2 qw;
                    asm("v_cvt_f32_f16_e32 %0, %3\n\t"
                        "v_cvt_f32_f16_sdwa %1, %3 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1"
                        : "=&v"(qw.x), "=v"(qw.y), "+v"(acc)
                        : "v"(qh));
                    const f32x2 t = f32x2{xe[j], xe[j]} - qw;
                    acc = __builtin_elementwise_fma(t, t, acc);
                }
            }
        }
        sa = acc.x;
        sb = acc.y;
    }
};

// ---- LS_DTYPE_BF16 (include/leansearch_bf16.h): a 16-byte chunk holds 8 bfloat16 elements, element 2 * i
// in the low half of word i. bf16 -> f32 is a 16-bit shift, so a stored element converts exactly; the query stays f32,
// prepared as for an fp32 index (one rounded multiply by the norm's inverse). A lane's partial sum is ONE fmaf chain from
// 0 over exact operands, in memory order (tests/bf16_ref.c restates it). An empty tag type at the end of the kernel's
// pack (after the row list, if any) selects QueryBf16; F16 is false and unused.
struct ls_bf16_arg {};
template <typename... X>
struct ls_pack_bf16 : std::bool_constant<(std::is_same_v<X, ls_bf16_arg> || ...)> {};

template <int V>
struct QueryBf16 {
    static constexpr int SMALL_PF = 4;
    float q[V][8];
    __device__ __forceinline__ float load(const float* qp, int d, int sub, int L) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int e = 8 * (sub + L * v);
#pragma unroll
            for (int j = 0; j < 8; ++j) q[v][j] = e + j < d ? qp[e + j] : 0.0f;
        }
        return 0.0f;
    }
    __device__ __forceinline__ void scale(float s) {
#pragma unroll
        for (int v = 0; v < V; ++v)
#pragma unroll
            for (int j = 0; j < 8; ++j) q[v][j] *= s;
    }
    __device__ __forceinline__ float dot(const f32x4 (&x)[V]) const {
        float acc = 0.0f;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float w[4] = {x[v].x, x[v].y, x[v].z, x[v].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                u32 u = __builtin_bit_cast(u32, w[i]);
                // (the word becomes opaque here: otherwise its two widened halves are computed as soon as the load lands
                // and carried - two registers for one - until the chain gets to them; QuerySq8::dot_tile)
                asm("" : "+v"(u));
                acc = fmaf(__builtin_bit_cast(float, u << 16), q[v][2 * i], acc);
                acc = fmaf(__builtin_bit_cast(float, u & 0xffff0000u), q[v][2 * i + 1], acc);
            }
        }
        return acc;
    }
};

template <bool F16, int V, bool SQ8, bool L2 = false, bool BF16 = false>
using scan_query_t = std::conditional_t<
    BF16, QueryBf16<V>, std::conditional_t<SQ8, QuerySq8<V>, std::conditional_t<L2, QueryL2<F16, V>, QueryRegs<F16, V>>>>;

// Sum over the L lanes that share a row, result in every lane of the group. Pure VALU: DPP
// inside 16-lane rows (quad_perm xor 1 / xor 2, row_half_mirror, row_mirror), then gfx950's
// v_permlane16_swap / v_permlane32_swap across rows. (ds_bpermute-based shuffles go through the
// LDS crossbar, which becomes the bottleneck when 8 queries share one corpus pass.)
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    const int moved = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true);
    return v + __builtin_bit_cast(float, moved);
}
template <int L>
__device__ __forceinline__ float group_sum(float v) {
    v = dpp_add<0xB1>(v);   // quad_perm [1,0,3,2]: + lane ^ 1
    v = dpp_add<0x4E>(v);   // quad_perm [2,3,0,1]: + lane ^ 2
    v = dpp_add<0x141>(v);  // row_half_mirror: + the other quad of each 8
    if (L >= 16) v = dpp_add<0x140>(v);  // row_mirror: + the other half of each 16 (L = 8, sq8 only: 8 lanes per row)
    if (L >= 32) {          // rows 0<->1, 2<->3
        const unsigned u = __builtin_bit_cast(unsigned, v);
        const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
        v = __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
    }
    if (L >= 64) {          // lanes 0-31 <-> 32-63
        const unsigned u = __builtin_bit_cast(unsigned, v);
        const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
        v = __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
    }
    return v;
}

// ---- several queries per corpus pass: reduce-SCATTER instead of U*NQ full reductions ------------
// A lane holds P = U*NQ partial dot products (row step u, query qi), pair index j = u*NQ + qi. The
// single-query path sums each of them over the L lanes of a row with its own butterfly (5-6
// cross-lane adds per pair, every lane ends with every sum) and then picks the lane that keeps it:
// ~13 VALU instructions per pair, more than the 12 FMAs that produced it. Here each butterfly step
// HALVES the live pairs instead: at bit b a lane keeps the pairs whose bit b equals its own and
// hands the others to its partner (lane ^ (1 << b)), so P pairs cost P - 1 cross-lane adds in
// total and lane `sub` ends with pair j = sub (P == L). The steps run over the same bits in the
// same order (1, 2, 4, .., L/2) and add the same two operands as group_sum, so every sum is
// BIT-IDENTICAL to the one the single-query kernel computes: a query's scores do not depend on
// the group it rides in.
template <int B>
__device__ __forceinline__ float xor_lane(float v) {  // value of lane ^ B
    if constexpr (B == 1)
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));
    else if constexpr (B == 2)
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true));
    else
        return __shfl_xor(v, B, 64);  // few of these per tile (the live pairs are down to <= P/4)
}
template <int L, int B, int LIVE, int P>
struct rs_step {
    static __device__ __forceinline__ void run(float (&p)[P], int sub) {
        if constexpr (B < L) {
            if constexpr (LIVE > 1) {
                const bool hi = (sub & B) != 0;
#pragma unroll
                for (int c = 0; c < LIVE / 2; ++c) {
                    const float lo_v = p[2 * c], hi_v = p[2 * c + 1];
                    const float keep = hi ? hi_v : lo_v, send = hi ? lo_v : hi_v;
                    p[c] = keep + xor_lane<B>(send);
                }
                rs_step<L, 2 * B, LIVE / 2, P>::run(p, sub);
            } else {  // one pair left but lanes to spare: plain butterfly, both partners keep the sum
                p[0] = p[0] + xor_lane<B>(p[0]);
                rs_step<L, 2 * B, 1, P>::run(p, sub);
            }
        }
    }
};
__host__ __device__ constexpr int ls_ilog2(int v) { return v <= 1 ? 0 : 1 + ls_ilog2(v / 2); }

// value of group (lane % R) delivered to every lane: R scalar reads + a select chain, no LDS
template <int L>
__device__ __forceinline__ float pick_group(float s, int lane) {
    constexpr int R = LS_WAVE / L;
    float out = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, s), 0));
#pragma unroll
    for (int r = 1; r < R; ++r) {
        const float vr =
            __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, s), r * L));
        out = (lane % R) == r ? vr : out;
    }
    return out;
}
