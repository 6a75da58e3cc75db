// ls_rows.hip — the device side of every call that changes the rows of a built handle: ls_ivf_add and ls_ivf_remove
// (ls_ivf_mutate.hip) and ls_remove (ls_remove.hip). DESIGN.md 4.7d.
//
//   move     ls_rows_move_kernel writes `rows` destination rows in STORED format: row s takes source row src[s] - of `a`
//            when src[s] < n_a, else row src[s] - n_a of `b`. The bytes are copied as stored - 16-byte chunks, one lane
//            per chunk -, so one body serves every dtype, row geometry and caller, and no row is ever decoded or
//            re-encoded. The lane that moves chunk 0 of a row also writes ids_dst[s], the row's original number
//            (ls_ivf_add_id). Every stored row is read once and written once: nontemporal both ways. A caller with one
//            source passes b = ids_a = ids_dst = nullptr and n_a = 0xffffffff, which no src value reaches. ONE body,
//            TWO instantiations: the second source and the ids are a template flag, because the flat removal's
//            move_ms measured 0.5 to 1 % above the parent's spread with the select and the null check in its loop
//            (profiles/ab/rows_refactor.txt); with the flag off the compiler emits the one-source copy as before.
//   count    ls_list_count_kernel: a list of positions cut into segments - [seg_off[g], seg_off[g + 1]) where seg_off is
//            given (an IVF subset: one segment per inverted list), else LS_RM_SEG positions each (a flat subset) -; a
//            workgroup per segment (grid-strided) counts the positions j whose row survives
//            (dst_of[list[j]] != LS_ROWS_GONE).
//   scatter  ls_list_scatter_kernel walks the same segments in the same steps and writes the survivors, in order, at
//            out_off[g] + rank: list_new = dst_of[list[j]] and, where sid_new is set, sid_new = ids_new[list_new]. The
//            rank is an ordered block prefix: the wave's ballot and a popcount below the lane, the waves' totals
//            through LDS, the survivors of the earlier steps in a register. Order inside a segment stays ascending.
//   shift    ls_ivf_subset_shift_kernel adds shift[l] to the storage rows srow[soff[l] .. soff[l + 1]) of one existing
//            IVF subset: its rows keep their order inside a list, the lists moved apart.
//   dst      ls_remove_dst_kernel scatters a survivor list src into dst_of[old row] = new row.
//
// Every index comes from ls_rows_plan.h; 64-bit row, chunk and position offsets throughout.
#include "ls_common.h"
#include "ls_ivf_add_plan.h"
#include "ls_remove_plan.h"

template <bool TWO>
__global__ __launch_bounds__(LS_ROWS_THREADS) void ls_rows_move_kernel(
    const u32x4* __restrict__ a, const u32x4* __restrict__ b, u32x4* __restrict__ dst, const u32* __restrict__ src,
    const u32* __restrict__ ids_a, u32* __restrict__ ids_dst, u32 n_a, long long rows, int chunks) {
    const int lane = threadIdx.x & (LS_ROWS_WAVE - 1);
    const int TR = ls_rows_tile_rows(chunks);
    const int lr = ls_rows_lane_row(lane, chunks), c0 = ls_rows_lane_chunk(lane, chunks);
    if (lr >= TR) return;  // (rows that do not fill the wave: the lanes past the last whole row)
    const long long W = (long long)gridDim.x * (LS_ROWS_THREADS / LS_ROWS_WAVE);
    const long long gw = (long long)blockIdx.x * (LS_ROWS_THREADS / LS_ROWS_WAVE) + threadIdx.x / LS_ROWS_WAVE;
    const long long NT = ls_rows_tiles(rows, chunks);
    for (long long t = gw; t < NT; t += W) {
        const long long s = t * TR + lr;
        if (s >= rows) continue;
        const u32 from = src[s];
        const u32x4* p = !TWO || from < n_a ? a + (long long)from * chunks : b + (long long)(from - n_a) * chunks;
        u32x4* q = dst + s * chunks;
        for (int c = c0; c < chunks; c += LS_ROWS_WAVE) __builtin_nontemporal_store(__builtin_nontemporal_load(p + c), q + c);
        if (TWO && c0 == 0) ids_dst[s] = ls_ivf_add_id(from, n_a, ids_a);
    }
}

// segment g of a list of m positions: [b, e)
static __device__ __forceinline__ void list_segment(const u32* __restrict__ seg_off, u32 m, int g, u32& b, u32& e) {
    if (seg_off) {
        b = seg_off[g];
        e = seg_off[g + 1];
    } else {
        b = (u32)g * LS_RM_SEG;
        e = (u32)min((long long)m, ((long long)g + 1) * LS_RM_SEG);
    }
}

// does position j of the segment that ends at e survive, and where does its row go
static __device__ __forceinline__ u32 list_dst(const u32* __restrict__ list, const u32* __restrict__ dst_of, long long j,
                                               u32 e) {
    return j < (long long)e ? dst_of[list[j]] : LS_ROWS_GONE;
}

__global__ __launch_bounds__(LS_LIST_THREADS) void ls_list_count_kernel(const u32* __restrict__ seg_off,
                                                                        const u32* __restrict__ list, u32 m,
                                                                        const u32* __restrict__ dst_of,
                                                                        u32* __restrict__ counts, int nseg) {
    __shared__ u32 totals[LS_LIST_WAVES];
    const int tid = threadIdx.x, lane = tid & (LS_ROWS_WAVE - 1), w = tid / LS_ROWS_WAVE;
    for (int g = blockIdx.x; g < nseg; g += gridDim.x) {
        u32 b, e;
        list_segment(seg_off, m, g, b, e);
        const u32 steps = ls_list_steps(e - b);
        u32 mine = 0;  // (wave-uniform: survivors this wave has seen)
        for (u32 i = 0; i < steps; ++i)
            mine += (u32)__popcll(__ballot(list_dst(list, dst_of, ls_list_pos(b, i, tid), e) != LS_ROWS_GONE));
        if (lane == 0) totals[w] = mine;
        __syncthreads();
        if (tid == 0) counts[g] = ls_list_step_total(totals);
        __syncthreads();  // (totals is written again for the workgroup's next segment)
    }
}

__global__ __launch_bounds__(LS_LIST_THREADS) void ls_list_scatter_kernel(
    const u32* __restrict__ seg_off, const u32* __restrict__ list, u32 m, const u32* __restrict__ dst_of,
    const u32* __restrict__ ids_new, const u32* __restrict__ out_off, u32* __restrict__ list_new,
    u32* __restrict__ sid_new, int nseg) {
    __shared__ u32 totals[LS_LIST_WAVES];
    const int tid = threadIdx.x, lane = tid & (LS_ROWS_WAVE - 1), w = tid / LS_ROWS_WAVE;
    for (int g = blockIdx.x; g < nseg; g += gridDim.x) {
        u32 b, e;
        list_segment(seg_off, m, g, b, e);
        const u32 steps = ls_list_steps(e - b);
        const u32 room = out_off[g + 1] - out_off[g];
        long long base = out_off[g];  // where the segment's first survivor goes
        u32 done = 0;                 // survivors of the earlier steps
        for (u32 i = 0; i < steps; ++i) {
            const u32 to = list_dst(list, dst_of, ls_list_pos(b, i, tid), e);
            const unsigned long long ballot = __ballot(to != LS_ROWS_GONE);
            if (lane == 0) totals[w] = (u32)__popcll(ballot);
            __syncthreads();
            const u32 rank = done + ls_list_wave_base(totals, w) + ls_list_lane_rank(ballot, lane);
            // (rank < room whenever out_off was made from the count kernel's counts of the same arrays)
            if (to != LS_ROWS_GONE && rank < room) {
                list_new[base + rank] = to;
                if (sid_new) sid_new[base + rank] = ids_new[to];
            }
            done += ls_list_step_total(totals);
            __syncthreads();  // (totals is written again in the next step)
        }
    }
}

#define LS_IVF_SHIFT_THREADS 256

// workgroup l (grid-strided over the lists): srow[soff[l] .. soff[l + 1]) += shift[l]
__global__ __launch_bounds__(LS_IVF_SHIFT_THREADS) void ls_ivf_subset_shift_kernel(const u32* __restrict__ soff,
                                                                                  const u32* __restrict__ shift,
                                                                                  u32* __restrict__ srow, int nlist) {
    for (int l = blockIdx.x; l < nlist; l += gridDim.x) {
        const u32 add = shift[l];
        if (!add) continue;
        const u32 b = soff[l], e = soff[l + 1];
        for (long long j = (long long)b + threadIdx.x; j < e; j += LS_IVF_SHIFT_THREADS) srow[j] += add;
    }
}

// dst_of[src[s]] = s for the survivors s < n_new (dst_of was filled with LS_ROWS_GONE)
__global__ __launch_bounds__(256) void ls_remove_dst_kernel(const u32* __restrict__ src, long long n_new,
                                                            u32* __restrict__ dst_of) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s < n_new) dst_of[src[s]] = (u32)s;
}

int ls_launch_rows_move(const void* d_a, const void* d_b, void* d_dst, const u32* d_src, const u32* d_ids_a,
                        u32* d_ids_dst, int64_t n_a, int64_t rows, const ls_geom& g, int32_t n_cu, hipStream_t s) {
    // One source (d_b null): n_a is the sentinel 0xffffffff and no ids are written. Every handle refuses n >= 2^32 - 1
    // rows, so every src value is below it and names a row of d_a. Two sources: src values below n_a name d_a, the
    // others d_b, and d_ids_dst is written.
    const bool one = !d_b;
    if (rows < 0 || rows >= 0xffffffffll || g.chunks < 1 || n_cu < 1 || (rows > 0 && (!d_dst || !d_src)) ||
        (one ? n_a != 0xffffffffll || (rows > 0 && !d_a) || d_ids_a || d_ids_dst
             : n_a < 0 || n_a > rows || (n_a > 0 && (!d_a || !d_ids_a)) || !d_ids_dst)) {
        ls_set_error("ls_launch_rows_move: bad arguments (n_a %lld rows %lld chunks %d)", (long long)n_a, (long long)rows,
                     g.chunks);
        return LS_ERR_INVALID_ARG;
    }
    if (rows == 0) return LS_OK;
    const int blocks = ls_rows_blocks(rows, g.chunks, n_cu);
    hipLaunchKernelGGL(one ? ls_rows_move_kernel<false> : ls_rows_move_kernel<true>, dim3((unsigned)blocks),
                       dim3(LS_ROWS_THREADS), 0, s, (const u32x4*)d_a, (const u32x4*)d_b, (u32x4*)d_dst, d_src, d_ids_a,
                       d_ids_dst, (u32)n_a, (long long)rows, (int)g.chunks);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

// what the count and the scatter launch share: a list of m < 2^32 positions in nseg segments
static bool list_args_ok(const u32* d_seg_off, const u32* d_list, int64_t m, const u32* d_dst_of, int64_t nseg) {
    return d_list && d_dst_of && m >= 0 && m < 0xffffffffll && nseg >= 1 && nseg <= 0x7fffffffll &&
           (d_seg_off || nseg == ls_remove_segs(m));
}

int ls_launch_list_count(const u32* d_seg_off, const u32* d_list, int64_t m, const u32* d_dst_of, u32* d_counts,
                         int64_t nseg, hipStream_t s) {
    if (!list_args_ok(d_seg_off, d_list, m, d_dst_of, nseg) || !d_counts) {
        ls_set_error("ls_launch_list_count: bad arguments (m %lld nseg %lld)", (long long)m, (long long)nseg);
        return LS_ERR_INVALID_ARG;
    }
    hipLaunchKernelGGL(ls_list_count_kernel, dim3((unsigned)ls_list_groups(nseg)), dim3(LS_LIST_THREADS), 0, s, d_seg_off,
                       d_list, (u32)m, d_dst_of, d_counts, (int)nseg);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

int ls_launch_list_scatter(const u32* d_seg_off, const u32* d_list, int64_t m, const u32* d_dst_of, const u32* d_ids_new,
                           const u32* d_out_off, u32* d_list_new, u32* d_sid_new, int64_t nseg, hipStream_t s) {
    if (!list_args_ok(d_seg_off, d_list, m, d_dst_of, nseg) || !d_out_off || !d_list_new || (d_sid_new && !d_ids_new)) {
        ls_set_error("ls_launch_list_scatter: bad arguments (m %lld nseg %lld)", (long long)m, (long long)nseg);
        return LS_ERR_INVALID_ARG;
    }
    hipLaunchKernelGGL(ls_list_scatter_kernel, dim3((unsigned)ls_list_groups(nseg)), dim3(LS_LIST_THREADS), 0, s,
                       d_seg_off, d_list, (u32)m, d_dst_of, d_ids_new, d_out_off, d_list_new, d_sid_new, (int)nseg);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

int ls_launch_ivf_subset_shift(const u32* d_soff, const u32* d_shift, u32* d_srow, int nlist, hipStream_t s) {
    if (!d_soff || !d_shift || !d_srow || nlist < 1) {
        ls_set_error("ls_launch_ivf_subset_shift: bad arguments (nlist %d)", nlist);
        return LS_ERR_INVALID_ARG;
    }
    hipLaunchKernelGGL(ls_ivf_subset_shift_kernel, dim3((unsigned)std::min(nlist, 4096)), dim3(LS_IVF_SHIFT_THREADS), 0, s,
                       d_soff, d_shift, d_srow, nlist);
    LS_HIP(hipGetLastError());
    return LS_OK;
}

int ls_launch_remove_dst(const u32* d_src, int64_t n_new, u32* d_dst_of, hipStream_t s) {
    if (!d_src || !d_dst_of || n_new < 1 || n_new >= 0xffffffffll) {
        ls_set_error("ls_launch_remove_dst: bad arguments (n_new %lld)", (long long)n_new);
        return LS_ERR_INVALID_ARG;
    }
    hipLaunchKernelGGL(ls_remove_dst_kernel, dim3((unsigned)((n_new + 255) / 256)), dim3(256), 0, s, d_src,
                       (long long)n_new, d_dst_of);
    LS_HIP(hipGetLastError());
    return LS_OK;
}
