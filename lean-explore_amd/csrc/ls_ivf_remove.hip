// ls_ivf_remove.hip — the device side of ls_ivf_remove (include/leansearch_ivf_remove.h; the call itself: ls_ivf.hip).
//
//   compact  ls_ivf_compact_kernel writes the new list-major storage from the old one in STORED format: destination
//            storage row s takes the bytes of old storage row src[s] (ls_ivf_remove_plan.h). 16-byte chunks, one lane
//            per chunk, ls_ivf_add_plan.h's tile deal, so ONE instantiation serves every dtype and row geometry and no
//            row is ever decoded. Every surviving stored row is read once and written once: nontemporal both ways. The
//            new ids (storage row -> new original row) are the plan's and are uploaded, not written here. The zero pad
//            rows behind the last row are the new index's own (written when its rows are reserved).
//   count    ls_ivf_subset_count_kernel: one workgroup per list (grid-strided) counts the positions j of an existing
//            subset's segment [soff[l], soff[l + 1]) whose storage row survives (dst_of[srow[j]] != LS_IVFR_GONE).
//   scatter  ls_ivf_subset_scatter_kernel walks the same segments in the same steps and writes the survivors, in order,
//            at soff_new[l] + rank: srow_new = dst_of[srow[j]], sid_new = ids_new[srow_new]. The rank is an ordered
//            block prefix: the wave's ballot and a popcount below the lane, the waves' totals through LDS, the
//            survivors of the earlier steps in a register. Order inside a list stays ascending.
//
// Every index comes from ls_ivf_remove_plan.h; 64-bit row, chunk and position offsets throughout.
#include "ls_common.h"
#include "ls_ivf_remove_plan.h"

__global__ __launch_bounds__(LS_IVFA_THREADS) void ls_ivf_compact_kernel(const u32x4* __restrict__ old_rows,
                                                                         u32x4* __restrict__ dst,
                                                                         const u32* __restrict__ src, long long n_new,
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
        const u32x4* p = old_rows + (long long)src[s] * chunks;
        u32x4* q = dst + s * chunks;
        for (int c = c0; c < chunks; c += LS_IVFA_WAVE) __builtin_nontemporal_store(__builtin_nontemporal_load(p + c), q + c);
    }
}

// does position j of the segment that ends at e survive, and where does its row go
static __device__ __forceinline__ u32 ivfr_dst(const u32* __restrict__ srow, const u32* __restrict__ dst_of, long long j,
                                               u32 e) {
    return j < (long long)e ? dst_of[srow[j]] : LS_IVFR_GONE;
}

__global__ __launch_bounds__(LS_IVFR_THREADS) void ls_ivf_subset_count_kernel(const u32* __restrict__ soff,
                                                                              const u32* __restrict__ srow,
                                                                              const u32* __restrict__ dst_of,
                                                                              u32* __restrict__ counts, int nlist) {
    __shared__ u32 totals[LS_IVFR_WAVES];
    const int tid = threadIdx.x, lane = tid & (LS_IVFA_WAVE - 1), w = tid / LS_IVFA_WAVE;
    for (int l = blockIdx.x; l < nlist; l += gridDim.x) {
        const u32 b = soff[l], e = soff[l + 1];
        const u32 steps = ls_ivf_remove_steps(e - b);
        u32 mine = 0;  // (wave-uniform: survivors this wave has seen)
        for (u32 i = 0; i < steps; ++i)
            mine += (u32)__popcll(__ballot(ivfr_dst(srow, dst_of, ls_ivf_remove_pos(b, i, tid), e) != LS_IVFR_GONE));
        if (lane == 0) totals[w] = mine;
        __syncthreads();
        if (tid == 0) counts[l] = ls_ivf_remove_step_total(totals);
        __syncthreads();  // (totals is written again for the workgroup's next list)
    }
}

__global__ __launch_bounds__(LS_IVFR_THREADS) void ls_ivf_subset_scatter_kernel(
    const u32* __restrict__ soff, const u32* __restrict__ srow, const u32* __restrict__ dst_of,
    const u32* __restrict__ ids_new, const u32* __restrict__ soff_new, u32* __restrict__ srow_new,
    u32* __restrict__ sid_new, int nlist) {
    __shared__ u32 totals[LS_IVFR_WAVES];
    const int tid = threadIdx.x, lane = tid & (LS_IVFA_WAVE - 1), w = tid / LS_IVFA_WAVE;
    for (int l = blockIdx.x; l < nlist; l += gridDim.x) {
        const u32 b = soff[l], e = soff[l + 1];
        const u32 steps = ls_ivf_remove_steps(e - b);
        const u32 room = soff_new[l + 1] - soff_new[l];
        long long base = soff_new[l];  // where the step's first survivor goes
        u32 done = 0;                  // survivors of the earlier steps
        for (u32 i = 0; i < steps; ++i) {
            const u32 to = ivfr_dst(srow, dst_of, ls_ivf_remove_pos(b, i, tid), e);
            const unsigned long long ballot = __ballot(to != LS_IVFR_GONE);
            if (lane == 0) totals[w] = (u32)__popcll(ballot);
            __syncthreads();
            const u32 rank = done + ls_ivf_remove_wave_base(totals, w) + ls_ivf_remove_lane_rank(ballot, lane);
            // (rank < room whenever soff_new was made from the count kernel's counts of the same arrays)
            if (to != LS_IVFR_GONE && rank < room) {
                srow_new[base + rank] = to;
                sid_new[base + rank] = ids_new[to];
            }
            done += ls_ivf_remove_step_total(totals);
            __syncthreads();  // (totals is written again in the next step)
        }
    }
}

int ls_launch_ivf_compact(const void* d_old, void* d_dst, const u32* d_src, int64_t n_new, const ls_geom& g, int32_t n_cu,
                          hipStream_t s) {
    if (n_new < 0 || n_new >= 0xffffffffll || g.chunks < 1 || n_cu < 1 || (n_new > 0 && (!d_old || !d_dst || !d_src))) {
        ls_set_error("ls_launch_ivf_compact: bad arguments (n_new %lld chunks %d)", (long long)n_new, g.chunks);
        return LS_ERR_INVALID_ARG;
    }
    if (n_new == 0) return LS_OK;
    const int blocks = ls_ivf_add_blocks(n_new, g.chunks, n_cu);
    hipLaunchKernelGGL(ls_ivf_compact_kernel, dim3((unsigned)blocks), dim3(LS_IVFA_THREADS), 0, s, (const u32x4*)d_old,
                       (u32x4*)d_dst, d_src, (long long)n_new, (int)g.chunks);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

int ls_launch_ivf_subset_count(const u32* d_soff, const u32* d_srow, const u32* d_dst_of, u32* d_counts, int nlist,
                               hipStream_t s) {
    if (!d_soff || !d_srow || !d_dst_of || !d_counts || nlist < 1) {
        ls_set_error("ls_launch_ivf_subset_count: bad arguments (nlist %d)", nlist);
        return LS_ERR_INVALID_ARG;
    }
    hipLaunchKernelGGL(ls_ivf_subset_count_kernel, dim3((unsigned)ls_ivf_remove_groups(nlist)), dim3(LS_IVFR_THREADS), 0, s,
                       d_soff, d_srow, d_dst_of, d_counts, nlist);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

int ls_launch_ivf_subset_scatter(const u32* d_soff, const u32* d_srow, const u32* d_dst_of, const u32* d_ids_new,
                                 const u32* d_soff_new, u32* d_srow_new, u32* d_sid_new, int nlist, hipStream_t s) {
    if (!d_soff || !d_srow || !d_dst_of || !d_ids_new || !d_soff_new || !d_srow_new || !d_sid_new || nlist < 1) {
        ls_set_error("ls_launch_ivf_subset_scatter: bad arguments (nlist %d)", nlist);
        return LS_ERR_INVALID_ARG;
    }
    hipLaunchKernelGGL(ls_ivf_subset_scatter_kernel, dim3((unsigned)ls_ivf_remove_groups(nlist)), dim3(LS_IVFR_THREADS), 0,
                       s, d_soff, d_srow, d_dst_of, d_ids_new, d_soff_new, d_srow_new, d_sid_new, nlist);
    LS_HIP(hipGetLastError());
    return LS_OK;
}
