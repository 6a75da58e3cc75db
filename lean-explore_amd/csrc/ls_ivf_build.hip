// ls_ivf_build.hip — building an IVF-flat index on the GPU (include/leansearch_ivf_build.h): the two steps of a Lloyd
// iteration as one kernel each, fp32 rows only.
//
//   assign  ls_ivf_assign_kernel<L, V, U>: rows x centroids -> the list of every row. Rows and centroids are in the
//           padded row layout of an fp32 index. A wave takes tiles of U * 64/L rows round-robin (ls_ivf_build_plan.h),
//           loads a tile ONCE into registers (16-byte nt loads, L lanes per row) and walks all nlist centroids for it.
//           The centroids are read through L2 with plain cacheable loads, a batch ahead of the batch being scored: the
//           whole centroid matrix (nlist < 8192 rows, 1.8 MB at the reference's 447 x 1024) stays L2-resident, every
//           wave of a CU walks it in the same order, so the CU's L1 serves most of the repeats, and no wave ever waits
//           for another one (no barrier, no LDS). The score of (row, centroid) is ls_scan_dev.h's own
//           QueryRegs<false, V>::dot + group_sum<L> with the ROW in the query registers - the role it has in
//           ls_search(centroid index, row, k = 1) - so the bits are that search's. Per row the running maximum of
//           ls_make_key(score, list) is kept: highest score, lowest list among equals, no key for NaN / <= -FLT_MAX; a
//           row without a key goes to list 0.
//           The body is ls_ivf_assign_kernel.h's, shared with the L2 form (ls_ivf_assign_l2_kernel of ls_l2_ivf.hip:
//           QueryL2 registers, the score negated once behind group_sum; include/leansearch_ivf_l2.h).
//   means   ls_ivf_means_kernel: one workgroup per list, thread t owns 16-byte chunk t of the row. The workgroup walks
//           assign[0, n) in blocks of 256, compacts its members in ascending row order (ballot + mbcnt, wave counts in
//           LDS) and adds the members' chunks to four float64 accumulators per thread, strictly in that order; loads
//           are issued LS_IVFB_MEANS_AHEAD rows ahead of their adds. Nothing but adds, one divide and conversions.
#include "ls_ivf_assign_kernel.h"

#include "../../include/leansearch_ivf_l2.h"

#include <cstdlib>
#include <mutex>
#include <vector>

template <int L, int V, int U>
__global__ __launch_bounds__(LS_SCAN_THREADS) void ls_ivf_assign_kernel(const f32x4* __restrict__ rows, long long n,
                                                                         const f32x4* __restrict__ cent, int nlist,
                                                                         int* __restrict__ assign) {
    ls_ivf_assign_body<L, V, U, false>(rows, n, cent, nlist, assign);
}

__global__ __launch_bounds__(LS_IVFB_MEANS_BLOCK) void ls_ivf_means_kernel(const f32x4* __restrict__ rows, long long n,
                                                                            int chunks, int d,
                                                                            const int* __restrict__ assign,
                                                                            const f32x4* __restrict__ cent,
                                                                            double* __restrict__ out) {
    constexpr int WAVES = LS_IVFB_MEANS_BLOCK / LS_WAVE;
    __shared__ int wcnt[2][WAVES];               // members per wave of the block (two generations: two barriers a step)
    __shared__ u32 mem[2][LS_IVFB_MEANS_BLOCK];  // the block's members, ascending
    const int list = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & (LS_WAVE - 1);
    const int wave = tid / LS_WAVE;
    const bool mine = tid < chunks;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    long long count = 0;
    const long long steps = ls_ivfb_means_steps(n);
    for (long long s = 0; s < steps; ++s) {
        const int p = (int)(s & 1);
        const long long r = ls_ivfb_means_row(s, tid);
        const bool m = r < n && assign[r] == list;
        const u64 bal = __ballot(m);
        const int before = __builtin_amdgcn_mbcnt_hi((u32)(bal >> 32), __builtin_amdgcn_mbcnt_lo((u32)bal, 0u));
        if (lane == 0) wcnt[p][wave] = __popcll(bal);
        __syncthreads();
        int base = 0, total = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const int c = wcnt[p][w];
            base += w < wave ? c : 0;
            total += c;
        }
        if (m) mem[p][base + before] = (u32)r;
        __syncthreads();
        if (mine) {
            for (int j = 0; j < total; j += LS_IVFB_MEANS_AHEAD) {
                f32x4 x[LS_IVFB_MEANS_AHEAD];
#pragma unroll
                for (int i = 0; i < LS_IVFB_MEANS_AHEAD; ++i) {
                    x[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    if (j + i < total) x[i] = __builtin_nontemporal_load(rows + (long long)mem[p][j + i] * chunks + tid);
                }
#pragma unroll
                for (int i = 0; i < LS_IVFB_MEANS_AHEAD; ++i)
                    if (j + i < total) {  // ascending rows, one add each
                        a0 += (double)x[i].x;
                        a1 += (double)x[i].y;
                        a2 += (double)x[i].z;
                        a3 += (double)x[i].w;
                    }
            }
        }
        count += total;
    }
    if (mine) {
        const f32x4 c = cent[(long long)list * chunks + tid];
        const double cnt = (double)count;
        const double v[4] = {count > 0 ? a0 / cnt : (double)c.x, count > 0 ? a1 / cnt : (double)c.y,
                             count > 0 ? a2 / cnt : (double)c.z, count > 0 ? a3 / cnt : (double)c.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = 4 * tid + i;
            if (e < d) out[(long long)list * d + e] = v[i];
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------
static int ivfb_launch_assign(const ls_geom& g, const void* d_rows, int64_t n, const void* d_cent, int32_t nlist,
                              int32_t* d_assign, int32_t n_cu, bool l2, hipStream_t s) {
    if (n <= 0) return LS_OK;
    if (l2) return ls_ivf_launch_assign_l2(g, d_rows, n, d_cent, nlist, d_assign, n_cu, s);  // (ls_l2_ivf.hip)
    return ls_geom_dispatch<false, true>("ls_ivf_assign", g, [&](auto L, auto V) -> int {
        const int blocks = ls_ivfb_blocks(n, L(), V(), n_cu);
        hipLaunchKernelGGL((ls_ivf_assign_kernel<L(), V(), scan_unroll(V())>), dim3(blocks), dim3(LS_SCAN_THREADS), 0, s,
                           (const f32x4*)d_rows, (long long)n, (const f32x4*)d_cent, nlist, d_assign);
        LS_HIP(hipGetLastError());
        return LS_OK;
    });
}

// host fp32 [m, d] -> the padded row layout at d_dst, on stream s (d_stage: m * d floats, used when a row is padded)
static int ivfb_upload(const float* h, int64_t m, const ls_geom& g, void* d_dst, float* d_stage, hipStream_t s) {
    if (m <= 0) return LS_OK;
    const size_t bytes = sizeof(float) * (size_t)m * g.d;
    if (g.d_pad == g.d) {
        LS_HIP(hipMemcpyAsync(d_dst, h, bytes, hipMemcpyHostToDevice, s));
        return LS_OK;
    }
    LS_HIP(hipMemcpyAsync(d_stage, h, bytes, hipMemcpyHostToDevice, s));
    return ls_launch_convert(d_stage, d_dst, m, g, s);
}

static int64_t ivfb_step_rows() {
    int64_t step = 1 << 16;
    if (const char* e = getenv("LS_IVF_ASSIGN_STEP")) {
        const long long v = atoll(e);
        if (v >= 1) step = v;
    }
    return step;
}

// the shape checks every entry point shares (`who` names the call in the message); fills g
static int ivfb_check_shape(const char* who, int64_t n, int32_t d, int32_t nlist, ls_geom* g) {
    if (n < 0 || n >= 0x7fffffffll || d <= 0) {
        ls_set_error("%s: bad shape n=%lld d=%d", who, (long long)n, d);
        return LS_ERR_INVALID_ARG;
    }
    if (nlist < 1 || nlist > LS_IVFB_MAX_NLIST) {
        ls_set_error("%s: nlist = %d (1 <= nlist < %d)", who, nlist, LS_IVFB_MAX_NLIST + 1);
        return LS_ERR_INVALID_ARG;
    }
    if (ls_pick_geom(d, LS_DTYPE_F32, g) != LS_OK) {
        ls_set_error("%s: unsupported d=%d (max stored row is 4096 bytes)", who, d);
        return LS_ERR_INVALID_ARG;
    }
    return LS_OK;
}

struct ls_ivf_trainer {
    std::mutex mu;  // calls on one trainer are serialised
    int32_t device = 0, d = 0, nlist = 0, n_cu = 256;
    int64_t n = 0;
    bool l2 = false;  // ls_ivf_trainer_create_l2: the assignment is the L2 form's
    ls_geom g{};
    hipStream_t stream = nullptr;
    void* d_rows = nullptr;      // [max(n, 1)] padded rows
    void* d_cent = nullptr;      // [nlist] padded rows
    float* d_stage = nullptr;    // raw floats: an upload step of rows, or the centroids (padded geometries only)
    int32_t* d_assign = nullptr;  // [max(n, 1)]
    double* d_means = nullptr;   // [nlist, d]
    std::vector<int32_t> h_assign;
    bool assigned = false;
    hipEvent_t ev[4] = {};  // around the last assign kernel, around the last means kernel
    bool timed_assign = false, timed_means = false;
};

static void ivfb_free(ls_ivf_trainer* t) {
    if (!t) return;
    ls_device_guard guard;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    for (void* p : {t->d_rows, t->d_cent, (void*)t->d_stage, (void*)t->d_assign, (void*)t->d_means}) (void)hipFree(p);
    for (hipEvent_t e : t->ev)
        if (e) (void)hipEventDestroy(e);
    if (t->stream) (void)hipStreamDestroy(t->stream);
    delete t;
}

static int ivfb_n_cu(int32_t device) {
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cu > 0) return cu;
    return 256;
}

static int ivfb_trainer_init(ls_ivf_trainer* t, const float* rows) {
    const ls_geom& g = t->g;
    const size_t row_bytes = (size_t)g.chunks * 16;
    const int64_t step = std::min<int64_t>(ivfb_step_rows(), std::max<int64_t>(t->n, 1));
    LS_HIP(hipSetDevice(t->device));
    t->n_cu = ivfb_n_cu(t->device);
    LS_HIP(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    for (hipEvent_t& e : t->ev) LS_HIP(hipEventCreate(&e));
    LS_HIP(hipMalloc(&t->d_rows, row_bytes * (size_t)std::max<int64_t>(t->n, 1)));
    LS_HIP(hipMalloc(&t->d_cent, row_bytes * (size_t)t->nlist));
    LS_HIP(hipMalloc((void**)&t->d_assign, sizeof(int32_t) * (size_t)std::max<int64_t>(t->n, 1)));
    LS_HIP(hipMalloc((void**)&t->d_means, sizeof(double) * (size_t)t->nlist * g.d));
    if (g.d_pad != g.d)
        LS_HIP(hipMalloc((void**)&t->d_stage, sizeof(float) * (size_t)std::max<int64_t>(step, t->nlist) * g.d));
    for (int64_t r0 = 0; r0 < t->n; r0 += step) {
        const int64_t m = std::min(step, t->n - r0);
        if (int rc = ivfb_upload(rows + r0 * g.d, m, g, (char*)t->d_rows + (size_t)r0 * row_bytes, t->d_stage, t->stream))
            return rc;
        LS_HIP(hipStreamSynchronize(t->stream));  // (the stage is reused; the caller's rows are read before we return)
    }
    return LS_OK;
}

static int ivfb_trainer_create(const char* who, bool l2, ls_ivf_trainer** out, const float* rows, int64_t n, int32_t d,
                               int32_t nlist, int32_t device) {
    if (!out) {
        ls_set_error("%s: out is null", who);
        return LS_ERR_INVALID_ARG;
    }
    *out = nullptr;
    ls_geom g;
    if (int rc = ivfb_check_shape(who, n, d, nlist, &g)) return rc;
    if (n > 0 && !rows) {
        ls_set_error("%s: rows is null (n=%lld)", who, (long long)n);
        return LS_ERR_INVALID_ARG;
    }
    if (int rc = ls_i_check_device(device)) return rc;
    ls_device_guard guard;
    ls_ivf_trainer* t = new ls_ivf_trainer();
    t->device = device;
    t->n = n;
    t->d = d;
    t->nlist = nlist;
    t->l2 = l2;
    t->g = g;
    const int rc = ivfb_trainer_init(t, rows);
    if (rc != LS_OK) {
        ivfb_free(t);
        return rc;
    }
    *out = t;
    return LS_OK;
}

// the list of every row of a host array, one launch per upload step (ls_ivf_assign, ls_ivf_assign_l2)
static int ivfb_assign(const char* who, bool l2, const float* rows, int64_t n, int32_t d, const float* centroids,
                       int32_t nlist, int32_t* out_assign, int32_t device) {
    ls_geom g;
    if (int rc = ivfb_check_shape(who, n, d, nlist, &g)) return rc;
    if (!centroids || (n > 0 && (!rows || !out_assign))) {
        ls_set_error("%s: null argument (n=%lld)", who, (long long)n);
        return LS_ERR_INVALID_ARG;
    }
    if (int rc = ls_i_check_device(device)) return rc;
    if (n == 0) return LS_OK;
    ls_device_guard guard;
    const size_t row_bytes = (size_t)g.chunks * 16;
    const int64_t step = std::min<int64_t>(ivfb_step_rows(), n);
    hipStream_t s = nullptr;
    void *d_rows = nullptr, *d_cent = nullptr;
    float* d_stage = nullptr;
    int32_t* d_assign = nullptr;
    auto run = [&]() -> int {
        LS_HIP(hipSetDevice(device));
        const int n_cu = ivfb_n_cu(device);
        LS_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        LS_HIP(hipMalloc(&d_rows, row_bytes * (size_t)step));
        LS_HIP(hipMalloc(&d_cent, row_bytes * (size_t)nlist));
        LS_HIP(hipMalloc((void**)&d_assign, sizeof(int32_t) * (size_t)step));
        if (g.d_pad != g.d) LS_HIP(hipMalloc((void**)&d_stage, sizeof(float) * (size_t)std::max<int64_t>(step, nlist) * g.d));
        if (int rc = ivfb_upload(centroids, nlist, g, d_cent, d_stage, s)) return rc;
        for (int64_t r0 = 0; r0 < n; r0 += step) {  // one launch per upload step
            const int64_t m = std::min(step, n - r0);
            if (int rc = ivfb_upload(rows + r0 * g.d, m, g, d_rows, d_stage, s)) return rc;
            if (int rc = ivfb_launch_assign(g, d_rows, m, d_cent, nlist, d_assign, n_cu, l2, s)) return rc;
            LS_HIP(hipMemcpyAsync(out_assign + r0, d_assign, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, s));
            LS_HIP(hipStreamSynchronize(s));
        }
        return LS_OK;
    };
    const int rc = run();
    if (s) (void)hipStreamSynchronize(s);
    for (void* p : {d_rows, d_cent, (void*)d_stage, (void*)d_assign}) (void)hipFree(p);
    if (s) (void)hipStreamDestroy(s);
    return rc;
}

extern "C" {

int ls_ivf_trainer_create(ls_ivf_trainer** out, const float* rows, int64_t n, int32_t d, int32_t nlist, int32_t device) {
    return ivfb_trainer_create("ls_ivf_trainer_create", false, out, rows, n, d, nlist, device);
}

int ls_ivf_trainer_create_l2(ls_ivf_trainer** out, const float* rows, int64_t n, int32_t d, int32_t nlist,
                             int32_t device) {
    return ivfb_trainer_create("ls_ivf_trainer_create_l2", true, out, rows, n, d, nlist, device);
}

int ls_ivf_trainer_assign(ls_ivf_trainer* t, const float* centroids, int32_t* out_assign, int64_t* out_counts) {
    if (!t || !centroids) {
        ls_set_error("ls_ivf_trainer_assign: %s is null", !t ? "the trainer" : "centroids");
        return LS_ERR_INVALID_ARG;
    }
    if (int rc = ls_i_check_device(t->device)) return rc;
    std::lock_guard<std::mutex> lk(t->mu);
    ls_device_guard guard;
    LS_HIP(hipSetDevice(t->device));
    if (int rc = ivfb_upload(centroids, t->nlist, t->g, t->d_cent, t->d_stage, t->stream)) return rc;
    LS_HIP(hipEventRecord(t->ev[0], t->stream));
    if (int rc = ivfb_launch_assign(t->g, t->d_rows, t->n, t->d_cent, t->nlist, t->d_assign, t->n_cu, t->l2, t->stream)) return rc;
    LS_HIP(hipEventRecord(t->ev[1], t->stream));
    t->timed_assign = true;
    t->h_assign.resize((size_t)t->n);
    if (t->n > 0)
        LS_HIP(hipMemcpyAsync(t->h_assign.data(), t->d_assign, sizeof(int32_t) * (size_t)t->n, hipMemcpyDeviceToHost,
                              t->stream));
    LS_HIP(hipStreamSynchronize(t->stream));
    t->assigned = true;
    if (out_assign) std::copy(t->h_assign.begin(), t->h_assign.end(), out_assign);
    if (out_counts) {
        std::fill(out_counts, out_counts + t->nlist, (int64_t)0);
        for (int32_t a : t->h_assign) out_counts[a]++;
    }
    return LS_OK;
}

int ls_ivf_trainer_means(ls_ivf_trainer* t, double* out_means) {
    if (!t || !out_means) {
        ls_set_error("ls_ivf_trainer_means: %s is null", !t ? "the trainer" : "out_means");
        return LS_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lk(t->mu);
    if (!t->assigned) {
        ls_set_error("ls_ivf_trainer_means: no assignment yet (call ls_ivf_trainer_assign first)");
        return LS_ERR_INVALID_ARG;
    }
    if (int rc = ls_i_check_device(t->device)) return rc;
    ls_device_guard guard;
    LS_HIP(hipSetDevice(t->device));
    LS_HIP(hipEventRecord(t->ev[2], t->stream));
    hipLaunchKernelGGL(ls_ivf_means_kernel, dim3(t->nlist), dim3(LS_IVFB_MEANS_BLOCK), 0, t->stream,
                       (const f32x4*)t->d_rows, (long long)t->n, t->g.chunks, t->g.d, (const int*)t->d_assign,
                       (const f32x4*)t->d_cent, t->d_means);
    LS_HIP(hipGetLastError());
    LS_HIP(hipEventRecord(t->ev[3], t->stream));
    t->timed_means = true;
    LS_HIP(hipMemcpyAsync(out_means, t->d_means, sizeof(double) * (size_t)t->nlist * t->g.d, hipMemcpyDeviceToHost,
                          t->stream));
    LS_HIP(hipStreamSynchronize(t->stream));
    return LS_OK;
}

int ls_ivf_trainer_last_kernel_ms(ls_ivf_trainer* t, float* assign_ms, float* means_ms) {
    if (!t) {
        ls_set_error("ls_ivf_trainer_last_kernel_ms: the trainer is null");
        return LS_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> lk(t->mu);
    ls_device_guard guard;
    float a = 0.0f, m = 0.0f;
    if (t->timed_assign || t->timed_means) LS_HIP(hipSetDevice(t->device));
    if (t->timed_assign) LS_HIP(hipEventElapsedTime(&a, t->ev[0], t->ev[1]));
    if (t->timed_means) LS_HIP(hipEventElapsedTime(&m, t->ev[2], t->ev[3]));
    if (assign_ms) *assign_ms = a;
    if (means_ms) *means_ms = m;
    return LS_OK;
}

void ls_ivf_trainer_destroy(ls_ivf_trainer* t) {
    if (!t) return;
    { std::lock_guard<std::mutex> lk(t->mu); }
    ivfb_free(t);
}

int ls_ivf_assign(const float* rows, int64_t n, int32_t d, const float* centroids, int32_t nlist, int32_t* out_assign,
                  int32_t device) {
    return ivfb_assign("ls_ivf_assign", false, rows, n, d, centroids, nlist, out_assign, device);
}

int ls_ivf_assign_l2(const float* rows, int64_t n, int32_t d, const float* centroids, int32_t nlist, int32_t* out_assign,
                     int32_t device) {
    return ivfb_assign("ls_ivf_assign_l2", true, rows, n, d, centroids, nlist, out_assign, device);
}

}  // extern "C"
