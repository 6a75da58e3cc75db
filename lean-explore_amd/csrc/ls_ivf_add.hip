// ls_ivf_add.hip — the device side of ls_ivf_add (include/leansearch_ivf_add.h; the call itself: ls_ivf.hip).
//
//   merge  ls_ivf_merge_kernel writes the new list-major storage from two sources in STORED format: the handle's
//          current rows and the new rows (converted and uploaded once, as a flat index of the handle's dtype - and, for
//          sq8, step). src[s] names the source of destination storage row s (ls_ivf_add_plan.h): below n_old an old
//          storage row, else new row src[s] - n_old. The bytes are copied as stored - 16-byte chunks, one lane per
//          chunk -, so ONE instantiation serves every dtype and row geometry, and no old row is ever re-encoded. The
//          lane that moves chunk 0 of a row also writes ids_new[s], the row's original number. Every stored row is read
//          once and written once: nontemporal both ways. The zero pad rows behind the last row are the new index's
//          own (written when its rows are reserved).
//   shift  ls_ivf_subset_shift_kernel adds shift[l] to the storage rows srow[soff[l] .. soff[l + 1]) of one existing
//          subset of the handle: its rows keep their order inside a list, the lists moved apart.
//
// Both kernels take every index from ls_ivf_add_plan.h; 64-bit row and chunk offsets throughout.
#include "ls_common.h"
#include "ls_ivf_add_plan.h"

__global__ __launch_bounds__(LS_IVFA_THREADS) void ls_ivf_merge_kernel(
    const u32x4* __restrict__ old_rows, const u32x4* __restrict__ new_rows, u32x4* __restrict__ dst,
    const u32* __restrict__ src, const u32* __restrict__ ids_old, u32* __restrict__ ids_new, u32 n_old, long long n_new,
    int chunks) {
    const int lane = threadIdx.x & (LS_IVFA_WAVE - 1);
    const int TR = ls_ivf_add_tile_rows(chunks);
    const int lr = ls_ivf_add_lane_row(lane, chunks), c0 = ls_ivf_add_lane_chunk(lane, chunks);
    if (lr >= TR) return;  // (rows that do not fill the wave: the lanes past the last whole row)
    const long long W = (long long)gridDim.x * (LS_IVFA_THREADS / LS_IVFA_WAVE);
    const long long gw = (long long)blockIdx.x * (LS_IVFA_THREADS / LS_IVFA_WAVE) + threadIdx.x / LS_IVFA_WAVE;
    const long long NT = ls_ivf_add_tiles(n_new, chunks);
    for (long long t = gw; t < NT; t += W) {
        const long long s = t * TR + lr;
        if (s >= n_new) continue;
        const u32 from = src[s];
        const u32x4* p = from < n_old ? old_rows + (long long)from * chunks : new_rows + (long long)(from - n_old) * chunks;
        u32x4* q = dst + s * chunks;
        for (int c = c0; c < chunks; c += LS_IVFA_WAVE) __builtin_nontemporal_store(__builtin_nontemporal_load(p + c), q + c);
        if (c0 == 0) ids_new[s] = ls_ivf_add_id(from, n_old, ids_old);
    }
}

#define LS_IVFA_SHIFT_THREADS 256

// workgroup l (grid-strided over the lists): srow[soff[l] .. soff[l + 1]) += shift[l]
__global__ __launch_bounds__(LS_IVFA_SHIFT_THREADS) void ls_ivf_subset_shift_kernel(const u32* __restrict__ soff,
                                                                                   const u32* __restrict__ shift,
                                                                                   u32* __restrict__ srow, int nlist) {
    for (int l = blockIdx.x; l < nlist; l += gridDim.x) {
        const u32 add = shift[l];
        if (!add) continue;
        const u32 b = soff[l], e = soff[l + 1];
        for (long long j = (long long)b + threadIdx.x; j < e; j += LS_IVFA_SHIFT_THREADS) srow[j] += add;
    }
}

int ls_launch_ivf_merge(const void* d_old, const void* d_new, void* d_dst, const u32* d_src, const u32* d_ids_old,
                        u32* d_ids_new, int64_t n_old, int64_t n_new, const ls_geom& g, int32_t n_cu, hipStream_t s) {
    if (n_old < 0 || n_new < n_old || n_new >= 0xffffffffll || g.chunks < 1 || n_cu < 1 || !d_dst || !d_src || !d_ids_new ||
        (n_old > 0 && (!d_old || !d_ids_old)) || (n_new > n_old && !d_new)) {
        ls_set_error("ls_launch_ivf_merge: bad arguments (n_old %lld n_new %lld chunks %d)", (long long)n_old,
                     (long long)n_new, g.chunks);
        return LS_ERR_INVALID_ARG;
    }
    if (n_new == 0) return LS_OK;
    const int blocks = ls_ivf_add_blocks(n_new, g.chunks, n_cu);
    hipLaunchKernelGGL(ls_ivf_merge_kernel, dim3((unsigned)blocks), dim3(LS_IVFA_THREADS), 0, s, (const u32x4*)d_old,
                       (const u32x4*)d_new, (u32x4*)d_dst, d_src, d_ids_old, d_ids_new, (u32)n_old, (long long)n_new,
                       (int)g.chunks);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

int ls_launch_ivf_subset_shift(const u32* d_soff, const u32* d_shift, u32* d_srow, int nlist, hipStream_t s) {
    if (!d_soff || !d_shift || !d_srow || nlist < 1) {
        ls_set_error("ls_launch_ivf_subset_shift: bad arguments (nlist %d)", nlist);
        return LS_ERR_INVALID_ARG;
    }
    hipLaunchKernelGGL(ls_ivf_subset_shift_kernel, dim3((unsigned)std::min(nlist, 4096)), dim3(LS_IVFA_SHIFT_THREADS), 0, s,
                       d_soff, d_shift, d_srow, nlist);
    LS_HIP(hipGetLastError());
    return LS_OK;
}
