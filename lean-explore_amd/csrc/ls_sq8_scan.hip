// ls_sq8_scan.hip — LS_DTYPE_SQ8 (include/leansearch_sq8.h): the scan kernel's sq8 instantiations (plain
// and row-list scan, NQ = 1, ten geometries; the IVF ones are in ls_sq8_ivf.hip), the encode / decode / training
// kernels and the four entry points of the header. A translation unit of its own: the build stays parallel and
// ls_scan.hip's instantiations keep their code.
#include "ls_scan_launch.h"

#include "../../include/leansearch_sq8.h"

#include <cmath>
#include <vector>

// ---- scan launches -------------------------------------------------------------------------------------------------
int ls_launch_scan_sq8(const void* d_corpus, int64_t n, const ls_geom& g, const ls_scan_args& a, hipStream_t s) {
    if (a.nq != 1 || !a.d_step) {
        ls_set_error("ls_launch_scan: an sq8 launch serves one query and needs the step (nq %d)", a.nq);
        return LS_ERR_INVALID_ARG;
    }
    return ls_geom_dispatch<true, true>("ls_launch_scan", g, [&](auto L, auto V) -> int {
        return ls_scan_launch<false, L(), V(), 1>(d_corpus, n, g, a, s, ls_sq8_arg{a.d_step});
    });
}

int ls_launch_scan_subset_sq8(const void* d_corpus, const u32* d_list, int64_t m, const ls_geom& g, const ls_scan_args& a,
                              hipStream_t s) {
    if (!a.d_step) {
        ls_set_error("ls_launch_scan_subset: an sq8 launch needs the step");
        return LS_ERR_INVALID_ARG;
    }
    return ls_geom_dispatch<true, true>("ls_launch_scan_subset", g, [&](auto L, auto V) -> int {
        return ls_scan_launch<false, L(), V(), 1>(d_corpus, m, g, a, s, d_list, ls_sq8_arg{a.d_step});
    });
}

// ---- training, encode, decode ----------------------------------------------------------------------------------------
// max |x| over the finite values of every column. Non-negative floats order like their bit patterns and a maximum
// does not depend on the order it is taken in: one atomicMax per (thread, column), deterministic.
__global__ __launch_bounds__(256) void ls_sq8_absmax_kernel(const float* __restrict__ src, long long n, int d,
                                                            u32* __restrict__ absmax) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= d) return;
    u32 m = 0;
    for (long long r = blockIdx.y; r < n; r += gridDim.y) {
        const u32 a = __builtin_bit_cast(u32, src[r * d + col]) & 0x7fffffffu;
        if (a < 0x7f800000u && a > m) m = a;  // (inf and NaN do not train the step)
    }
    if (m) atomicMax(absmax + col, m);
}
__global__ __launch_bounds__(256) void ls_sq8_step_kernel(const u32* __restrict__ absmax, int d, float* __restrict__ step) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= d) return;
    const float a = __builtin_bit_cast(float, absmax[col]);
    step[col] = a > 0.0f ? a / 127.0f : 1.0f;
}
__device__ __forceinline__ int ls_sq8_code(float x, float step) {
    if (x != x) return 0;
    const float r = rintf(x / step);  // correctly rounded division, ties to even
    return (int)fminf(fmaxf(r, -127.0f), 127.0f);
}
// one thread per 16-byte chunk of the stored layout
__global__ __launch_bounds__(256) void ls_sq8_encode_kernel(const float* __restrict__ src, uint4* __restrict__ dst, long long n,
                                                            int d, int chunks, const float* __restrict__ step) {
    const long long total = n * chunks;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / chunks;
        const int c = (int)(i - r * chunks);
        const float* p = src + r * d;
        u32 w[4];
#pragma unroll
        for (int wi = 0; wi < 4; ++wi) {
            u32 o = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int j = c * 16 + wi * 4 + b;
                const int code = j < d ? ls_sq8_code(p[j], step[j]) : 0;
                o |= ((u32)code & 0xffu) << (8 * b);
            }
            w[wi] = o;
        }
        dst[i] = uint4{w[0], w[1], w[2], w[3]};
    }
}
// stored codes -> f32 [n, d]: (float)c * step (WITH_STEP), or the codes themselves as int8 [n, d]
template <bool WITH_STEP, typename T>
__global__ __launch_bounds__(256) void ls_sq8_decode_kernel(const signed char* __restrict__ src, T* __restrict__ dst,
                                                            long long n, int d, int chunks, const float* __restrict__ step) {
    const long long total = n * d;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / d;
        const int j = (int)(i - r * d);
        const signed char c = src[r * (long long)chunks * 16 + j];
        if constexpr (WITH_STEP) dst[i] = (float)c * step[j];
        else dst[i] = c;
    }
}

static unsigned sq8_grid(long long total) {
    long long blocks = (total + 255) / 256;
    return (unsigned)(blocks > 65536 ? 65536 : (blocks < 1 ? 1 : blocks));
}
int ls_launch_sq8_encode(const float* d_src, void* d_dst, int64_t n, const ls_geom& g, const float* d_step, hipStream_t s) {
    if (n <= 0) return LS_OK;
    hipLaunchKernelGGL(ls_sq8_encode_kernel, dim3(sq8_grid((long long)n * g.chunks)), dim3(256), 0, s, d_src, (uint4*)d_dst,
                       (long long)n, g.d, g.chunks, d_step);
    LS_HIP(hipGetLastError());
    return LS_OK;
}
int ls_launch_sq8_decode(const void* d_src, float* d_dst, int64_t n, const ls_geom& g, const float* d_step, hipStream_t s) {
    if (n <= 0) return LS_OK;
    hipLaunchKernelGGL((ls_sq8_decode_kernel<true, float>), dim3(sq8_grid((long long)n * g.d)), dim3(256), 0, s,
                       (const signed char*)d_src, d_dst, (long long)n, g.d, g.chunks, d_step);
    LS_HIP(hipGetLastError());
    return LS_OK;
}
int ls_launch_sq8_absmax(const float* d_src, int64_t n, int32_t d, u32* d_absmax, hipStream_t s) {
    if (n <= 0) return LS_OK;
    const unsigned gy = (unsigned)std::min<int64_t>(n, 1024);
    hipLaunchKernelGGL(ls_sq8_absmax_kernel, dim3((unsigned)((d + 255) / 256), gy), dim3(256), 0, s, d_src, (long long)n, d,
                       d_absmax);
    LS_HIP(hipGetLastError());
    return LS_OK;
}
int ls_launch_sq8_step(const u32* d_absmax, int32_t d, float* d_step, hipStream_t s) {
    hipLaunchKernelGGL(ls_sq8_step_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, s, d_absmax, d, d_step);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// ---- include/leansearch_sq8.h ----------------------------------------------------------------------------------------
extern "C" {

int ls_create_sq8(ls_index** out, const float* corpus, int64_t n, int32_t d, const float* step, int32_t device) {
    return ls_i_create(out, corpus, false, n, d, LS_DTYPE_SQ8, step, device, "ls_create_sq8");
}

int ls_sq8_geom(int32_t d, int32_t* chunks, int32_t* L, int32_t* V) {
    ls_geom g;
    if (ls_pick_geom(d, LS_DTYPE_SQ8, &g) != LS_OK) {
        ls_set_error("ls_sq8_geom: unsupported d=%d (a stored row is at most 4096 bytes)", d);
        return LS_ERR_INVALID_ARG;
    }
    if (chunks) *chunks = g.chunks;
    if (L) *L = g.L;
    if (V) *V = g.V;
    return LS_OK;
}

static int sq8_check_handle(const ls_index* ix, const char* who) {
    if (!ix || ix->group || ix->dtype != LS_DTYPE_SQ8) {
        ls_set_error("%s: not an sq8 index", who);
        return LS_ERR_INVALID_ARG;
    }
    return LS_OK;
}

int ls_sq8_step(ls_index* ix, float* out) {
    if (int rc = sq8_check_handle(ix, "ls_sq8_step")) return rc;
    if (!out) {
        ls_set_error("ls_sq8_step: out is null");
        return LS_ERR_INVALID_ARG;
    }
    ls_quiesce lk(ix);
    LS_HIP(hipSetDevice(ix->device));
    LS_HIP(hipMemcpy(out, ix->d_sq8_step, sizeof(float) * (size_t)ix->g.d, hipMemcpyDeviceToHost));
    return LS_OK;
}

int ls_sq8_codes(ls_index* ix, int64_t row0, int64_t count, int8_t* out) {
    if (int rc = sq8_check_handle(ix, "ls_sq8_codes")) return rc;
    if (row0 < 0 || count < 0 || row0 + count > ix->n || (count > 0 && !out)) {
        ls_set_error("ls_sq8_codes: bad argument");
        return LS_ERR_INVALID_ARG;
    }
    if (count == 0) return LS_OK;
    ls_quiesce lk(ix);
    LS_HIP(hipSetDevice(ix->device));
    const ls_geom& g = ix->g;
    const int64_t slab = std::max<int64_t>(1, (int64_t)(256ll << 20) / g.d);
    signed char* stage = nullptr;
    LS_HIP(hipMalloc((void**)&stage, (size_t)std::min(slab, count) * g.d));
    int rc = LS_OK;
    for (int64_t r0 = 0; rc == LS_OK && r0 < count; r0 += slab) {
        const int64_t nr = std::min(slab, count - r0);
        hipLaunchKernelGGL((ls_sq8_decode_kernel<false, signed char>), dim3(sq8_grid((long long)nr * g.d)), dim3(256), 0,
                           ix->own_stream, (const signed char*)ix->d_corpus + (size_t)(row0 + r0) * g.chunks * 16, stage,
                           (long long)nr, g.d, g.chunks, (const float*)nullptr);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ix->own_stream) != hipSuccess ||
            hipMemcpy(out + r0 * g.d, stage, (size_t)nr * g.d, hipMemcpyDeviceToHost) != hipSuccess) {
            ls_set_error("ls_sq8_codes: HIP copy/launch failed");
            rc = LS_ERR_HIP;
        }
    }
    (void)hipFree(stage);
    return rc;
}

}  // extern "C"
