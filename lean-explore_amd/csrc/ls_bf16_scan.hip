// ls_bf16_scan.hip — LS_DTYPE_BF16 (include/leansearch_bf16.h): the scan kernel's bf16 instantiations
// (plain and row-list scan, NQ = 1, the eight 2-byte geometries, SMALL and not; the IVF ones are in ls_bf16_ivf.hip), the
// encode / decode / bits kernels and the flat entry points of the header. A translation unit of its own: the build stays
// parallel and ls_scan.hip's instantiations keep their code.
#include "ls_scan_launch.h"

#include "ls_index.h"
#include "../../include/leansearch_bf16.h"

// ---- scan launches -------------------------------------------------------------------------------------------------
int ls_launch_scan_bf16(const void* d_corpus, int64_t n, const ls_geom& g, const ls_scan_args& a, hipStream_t s) {
    if (a.nq != 1 || !g.bf16 || a.l2) {
        ls_set_error("ls_launch_scan: a bf16 launch serves one inner-product query over bf16 rows (nq %d)", a.nq);
        return LS_ERR_INVALID_ARG;
    }
    return ls_geom_dispatch<false, true>("ls_launch_scan", g, [&](auto L, auto V) -> int {
        return ls_scan_launch<false, L(), V(), 1>(d_corpus, n, g, a, s, ls_bf16_arg{});
    });
}

int ls_launch_scan_subset_bf16(const void* d_corpus, const u32* d_list, int64_t m, const ls_geom& g, const ls_scan_args& a,
                               hipStream_t s) {
    if (!g.bf16 || a.l2) {
        ls_set_error("ls_launch_scan_subset: a bf16 launch serves the inner product over bf16 rows");
        return LS_ERR_INVALID_ARG;
    }
    return ls_geom_dispatch<false, true>("ls_launch_scan_subset", g, [&](auto L, auto V) -> int {
        return ls_scan_launch<false, L(), V(), 1>(d_corpus, m, g, a, s, d_list, ls_bf16_arg{});
    });
}

// ---- encode, decode, bits ------------------------------------------------------------------------------------------
// f32 bit pattern -> bf16 bits, round to nearest even (include/leansearch_bf16.h restates it; lean_explore_amd/bf16.py too)
__device__ __forceinline__ u32 ls_bf16_bits(u32 u) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x0040u;  // NaN stays NaN, quiet
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
// One thread per 16-byte chunk of the stored layout. inexact (optional): += the elements whose stored value differs
// from the f32 handed in (NaN never counts; the zero padding is exact) - summed over the wave, ONE atomicAdd per wave.
__global__ __launch_bounds__(256) void ls_bf16_encode_kernel(const float* __restrict__ src, uint4* __restrict__ dst, long long n,
                                                             int d, int chunks, unsigned long long* __restrict__ inexact) {
    const long long total = n * chunks;
    u32 bad = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / chunks;
        const int c = (int)(i - r * chunks);
        const float* p = src + r * d;
        u32 w[4];
#pragma unroll
        for (int wi = 0; wi < 4; ++wi) {
            u32 o = 0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int j = c * 8 + wi * 2 + h;
                const u32 u = j < d ? __builtin_bit_cast(u32, p[j]) : 0u;
                const u32 b = ls_bf16_bits(u);
                bad += (b << 16) != u && (u & 0x7fffffffu) <= 0x7f800000u;
                o |= b << (16 * h);
            }
            w[wi] = o;
        }
        dst[i] = uint4{w[0], w[1], w[2], w[3]};
    }
    if (inexact) {  // (wave-uniform; every lane of the wave is here: the loop above has no early exit)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, LS_WAVE);
        if ((threadIdx.x & (LS_WAVE - 1)) == 0 && bad) atomicAdd(inexact, (unsigned long long)bad);
    }
}
// stored rows -> f32 [n, d] (bits << 16, exact), or the bits themselves as uint16 [n, d]
template <typename T>
__global__ __launch_bounds__(256) void ls_bf16_decode_kernel(const unsigned short* __restrict__ src, T* __restrict__ dst,
                                                             long long n, int d, int chunks) {
    const long long total = n * d;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / d;
        const int j = (int)(i - r * d);
        const unsigned short b = src[r * (long long)chunks * 8 + j];
        if constexpr (std::is_same_v<T, float>) dst[i] = __builtin_bit_cast(float, (u32)b << 16);
        else dst[i] = b;
    }
}

static unsigned bf16_grid(long long total) {
    long long blocks = (total + 255) / 256;
    return (unsigned)(blocks > 65536 ? 65536 : (blocks < 1 ? 1 : blocks));
}
int ls_launch_bf16_encode(const float* d_src, void* d_dst, int64_t n, const ls_geom& g, unsigned long long* d_inexact,
                          hipStream_t s) {
    if (n <= 0) return LS_OK;
    hipLaunchKernelGGL(ls_bf16_encode_kernel, dim3(bf16_grid((long long)n * g.chunks)), dim3(256), 0, s, d_src, (uint4*)d_dst,
                       (long long)n, g.d, g.chunks, d_inexact);
    LS_HIP(hipGetLastError());
    return LS_OK;
}
int ls_launch_bf16_decode(const void* d_src, float* d_dst, int64_t n, const ls_geom& g, hipStream_t s) {
    if (n <= 0) return LS_OK;
    hipLaunchKernelGGL((ls_bf16_decode_kernel<float>), dim3(bf16_grid((long long)n * g.d)), dim3(256), 0, s,
                       (const unsigned short*)d_src, d_dst, (long long)n, g.d, g.chunks);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// ---- include/leansearch_bf16.h (the flat handle's entry points) ----------------------------------------------------------
static int bf16_check_handle(const ls_index* ix, const char* who) {
    if (!ix || ix->group || ix->dtype != LS_DTYPE_BF16) {
        ls_set_error("%s: not a bf16 index", who);
        return LS_ERR_INVALID_ARG;
    }
    return LS_OK;
}

// (the caller holds the handle's ls_quiesce or owns the handle outright; its device is made current)
int ls_i_bf16_inexact(ls_index* ix, int64_t* out) {
    unsigned long long c = 0;
    LS_HIP(hipSetDevice(ix->device));
    LS_HIP(hipStreamSynchronize(ix->own_stream));
    LS_HIP(hipMemcpy(&c, ix->d_bf16_inexact, sizeof(c), hipMemcpyDeviceToHost));
    *out = (int64_t)c;
    return LS_OK;
}

extern "C" {

int ls_bf16_inexact(ls_index* ix, int64_t* out) {
    if (int rc = bf16_check_handle(ix, "ls_bf16_inexact")) return rc;
    if (!out) {
        ls_set_error("ls_bf16_inexact: out is null");
        return LS_ERR_INVALID_ARG;
    }
    ls_quiesce lk(ix);
    return ls_i_bf16_inexact(ix, out);
}

int ls_bf16_rows(ls_index* ix, int64_t row0, int64_t count, uint16_t* out) {
    if (int rc = bf16_check_handle(ix, "ls_bf16_rows")) return rc;
    if (row0 < 0 || count < 0 || row0 + count > ix->n || (count > 0 && !out)) {
        ls_set_error("ls_bf16_rows: bad argument");
        return LS_ERR_INVALID_ARG;
    }
    if (count == 0) return LS_OK;
    ls_quiesce lk(ix);
    LS_HIP(hipSetDevice(ix->device));
    const ls_geom& g = ix->g;
    const int64_t slab = std::max<int64_t>(1, (int64_t)(256ll << 20) / ((int64_t)g.d * 2));
    unsigned short* stage = nullptr;
    LS_HIP(hipMalloc((void**)&stage, (size_t)std::min(slab, count) * g.d * sizeof(unsigned short)));
    int rc = LS_OK;
    for (int64_t r0 = 0; rc == LS_OK && r0 < count; r0 += slab) {
        const int64_t nr = std::min(slab, count - r0);
        hipLaunchKernelGGL((ls_bf16_decode_kernel<unsigned short>), dim3(bf16_grid((long long)nr * g.d)), dim3(256), 0,
                           ix->own_stream, (const unsigned short*)ix->d_corpus + (size_t)(row0 + r0) * g.chunks * 8, stage,
                           (long long)nr, g.d, g.chunks);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ix->own_stream) != hipSuccess ||
            hipMemcpy(out + r0 * g.d, stage, (size_t)nr * g.d * sizeof(unsigned short), hipMemcpyDeviceToHost) != hipSuccess) {
            ls_set_error("ls_bf16_rows: HIP copy/launch failed");
            rc = LS_ERR_HIP;
        }
    }
    (void)hipFree(stage);
    return rc;
}

}  // extern "C"
