// ls_rows_plan.h — how ls_rows.hip's kernels deal their work, for every call that moves stored rows of a built handle
// (ls_ivf_add, ls_ivf_remove, ls_remove). Plain inline functions (no HIP): the kernels and their launchers take every
// index from here, and the host checks under tests/ (ivf_add_plan_check.cpp, ivf_remove_plan_check.cpp,
// remove_plan_check.cpp, mutation_chain_check.cpp) walk the same functions thread by thread. Where the rows GO is the
// callers' own: ls_ivf_add_plan.h, ls_ivf_remove_plan.h, ls_remove_plan.h.
//
// Deal of the row mover. A stored row is `chunks` 16-byte chunks and one lane moves one chunk. A wave takes
// ls_rows_tile_rows(chunks) rows at a time (as many whole rows as fit its 64 lanes, one for wider rows: lane i then
// moves chunks i, i + 64, ...); wave gw of W takes tiles gw, gw + W, ... as the scan kernels do.
//
// Deal of the list compaction. A list of positions is cut into segments; workgroup b of G takes segments b, b + G, ...
// and walks a segment in steps of LS_LIST_THREADS positions, thread t of step i looking at position begin +
// i * LS_LIST_THREADS + t. A position survives when the row it names maps to something other than LS_ROWS_GONE. Inside
// a step the survivors are ranked in thread order: a wave's ballot gives the lane's rank among its wave
// (ls_list_lane_rank), the waves' totals - through LDS - the wave's base (ls_list_wave_base), and the survivors of the
// earlier steps the step's base. The count kernel adds the same ballots' popcounts up.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LS_ROWS_HD __host__ __device__
#else
#define LS_ROWS_HD
#endif

#define LS_ROWS_WAVE 64
#define LS_ROWS_THREADS 256    // threads of a row-mover workgroup (4 waves)
#define LS_ROWS_WG_PER_CU 8    // workgroups per CU a row-mover launch has at most
#define LS_ROWS_GONE 0xffffffffu  // "this row is removed" in a row -> destination table
#define LS_LIST_THREADS 256    // threads of a compaction workgroup (4 waves)
#define LS_LIST_WAVES (LS_LIST_THREADS / LS_ROWS_WAVE)
#define LS_LIST_MAX_GROUPS 4096  // workgroups of a compaction launch at most (grid-strided over the segments)

// row r of a bitmap of nbytes bytes in ls_subset_create's layout; rows past a short bitmap are not selected
static inline bool ls_rows_bit(const uint8_t* bitmap, int64_t nbytes, int64_t r) {
    const int64_t b = r >> 3;
    return b < nbytes && ((bitmap[b] >> (r & 7)) & 1);
}

// ---- the row mover's deal ---------------------------------------------------------------------------------------------
static constexpr LS_ROWS_HD int ls_rows_tile_rows(int chunks) { return chunks >= LS_ROWS_WAVE ? 1 : LS_ROWS_WAVE / chunks; }
static constexpr LS_ROWS_HD long long ls_rows_tiles(long long rows, int chunks) {
    return (rows + ls_rows_tile_rows(chunks) - 1) / ls_rows_tile_rows(chunks);
}
// lane -> (row of the tile, first chunk); a lane whose row is >= ls_rows_tile_rows(chunks) idles
static constexpr LS_ROWS_HD int ls_rows_lane_row(int lane, int chunks) { return chunks >= LS_ROWS_WAVE ? 0 : lane / chunks; }
static constexpr LS_ROWS_HD int ls_rows_lane_chunk(int lane, int chunks) { return chunks >= LS_ROWS_WAVE ? lane : lane % chunks; }
// workgroups: one wave per tile until every CU holds LS_ROWS_WG_PER_CU of them
static inline int ls_rows_blocks(long long rows, int chunks, int n_cu) {
    const long long waves = LS_ROWS_THREADS / LS_ROWS_WAVE;
    const long long need = (ls_rows_tiles(rows, chunks) + waves - 1) / waves;
    const long long cap = (long long)n_cu * LS_ROWS_WG_PER_CU;
    return (int)(need < 1 ? 1 : (need > cap ? cap : need));
}

// ---- the list compaction's deal -----------------------------------------------------------------------------------------
// workgroups of a launch over `segs` segments
static inline int ls_list_groups(long long segs) { return (int)(segs < 1 ? 1 : (segs > LS_LIST_MAX_GROUPS ? LS_LIST_MAX_GROUPS : segs)); }
// steps a segment of `len` positions takes
static constexpr LS_ROWS_HD uint32_t ls_list_steps(uint32_t len) { return (len + LS_LIST_THREADS - 1) / LS_LIST_THREADS; }
// the position thread `tid` looks at in step `step` of the segment that begins at `begin` (64-bit: begin + len < 2^32,
// the last step may reach past it)
static constexpr LS_ROWS_HD long long ls_list_pos(uint32_t begin, uint32_t step, int tid) {
    return (long long)begin + (long long)step * LS_LIST_THREADS + tid;
}
// survivors of the lane's wave in the lanes below it (ballot: bit i = lane i survives)
static inline LS_ROWS_HD uint32_t ls_list_lane_rank(unsigned long long ballot, int lane) {
    return (uint32_t)__builtin_popcountll(ballot & ((1ull << lane) - 1ull));
}
// survivors of the step in the waves below wave w (totals: [LS_LIST_WAVES] survivors of every wave of the step)
static inline LS_ROWS_HD uint32_t ls_list_wave_base(const uint32_t* totals, int w) {
    uint32_t b = 0;
    for (int i = 0; i < LS_LIST_WAVES; ++i) b += i < w ? totals[i] : 0u;
    return b;
}
static inline LS_ROWS_HD uint32_t ls_list_step_total(const uint32_t* totals) {
    uint32_t b = 0;
    for (int i = 0; i < LS_LIST_WAVES; ++i) b += totals[i];
    return b;
}
