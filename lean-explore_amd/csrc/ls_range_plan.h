// ls_range_plan.h — how ls_range.hip's kernels deal their work (include/leansearch_range.h). Plain inline functions
// (no HIP): the kernels and their launchers take every index from here, and tests/range_plan_check.cpp walks the same
// functions thread by thread over a host model of count -> offsets -> emit.
//
// A score vector of n floats is cut into slabs of LS_RANGE_SLAB rows; one workgroup of LS_RANGE_THREADS threads serves
// one (slab, query), thread t looking at the LS_RANGE_VEC rows ls_range_row0(slab, t) + c, c = 0 .. 3 (one 16-byte
// load). A hit's rank inside its slab counts the hits before it in (thread, component) order, which is row order:
//   rank = hits of the waves below its wave (through LDS)       ls_range_wave_base
//        + hits of the lanes below its lane (four ballots)      ls_range_lane_rank
//        + hits of its own thread at lower components           ls_range_comp_rank
// The count kernel adds the same ballots' popcounts up (ls_range_wave_total). The offsets kernel turns a query's slab
// counts into 64-bit exclusive offsets, thread t owning the contiguous slabs ls_range_seg(nslab, t); a hit's slot in
// its query's segment of the result is offset of its slab + rank: dense, and ascending in the row.
//
// A call's queries are served in groups of up to LS_RANGE_GROUP (the score vectors of one scratch generation):
// group j covers queries [j * LS_RANGE_GROUP, ...) - ls_range_groups / ls_range_group_size.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LS_RANGE_HD __host__ __device__
#else
#define LS_RANGE_HD
#endif

#define LS_RANGE_WAVE 64
#define LS_RANGE_THREADS 256  // threads of a count / emit workgroup (4 waves)
#define LS_RANGE_WAVES (LS_RANGE_THREADS / LS_RANGE_WAVE)
#define LS_RANGE_VEC 4        // floats of one 16-byte load
#define LS_RANGE_SLAB (LS_RANGE_THREADS * LS_RANGE_VEC)  // rows one workgroup covers: 1024
#define LS_RANGE_GROUP 8      // queries (score vectors) one group of launches serves
#define LS_RANGE_OFF_THREADS 256  // threads of the offsets workgroup

// ---- grids ------------------------------------------------------------------------------------------------------------
static constexpr LS_RANGE_HD long long ls_range_slabs(long long n) { return (n + LS_RANGE_SLAB - 1) / LS_RANGE_SLAB; }
// floats a score vector of n rows is allocated with (and the distance to the next one): a 16-byte load that starts at a
// row below n, a multiple of LS_RANGE_VEC, ends inside it
static constexpr LS_RANGE_HD long long ls_range_stride(long long n) { return (n + 63) / 64 * 64; }
// the first row thread `tid` of the workgroup of `slab` looks at
static constexpr LS_RANGE_HD long long ls_range_row0(long long slab, int tid) {
    return slab * LS_RANGE_SLAB + (long long)tid * LS_RANGE_VEC;
}

// ---- a call's queries in groups ---------------------------------------------------------------------------------------
static constexpr LS_RANGE_HD long long ls_range_groups(long long nq) { return (nq + LS_RANGE_GROUP - 1) / LS_RANGE_GROUP; }
static constexpr LS_RANGE_HD int ls_range_group_size(long long nq, long long group) {
    return (int)(nq - group * LS_RANGE_GROUP < LS_RANGE_GROUP ? nq - group * LS_RANGE_GROUP : LS_RANGE_GROUP);
}

// ---- the predicate ----------------------------------------------------------------------------------------------------
// strictly above the radius, not NaN (both comparisons are false for one), and above -FLT_MAX: the library's "never
// returned" rule. Plain comparisons: radius = -inf lets every valid row through, +inf and NaN none.
static inline LS_RANGE_HD bool ls_range_hit(float s, float radius) { return s > radius && s > -3.402823466e+38f; }

// ---- ranks ------------------------------------------------------------------------------------------------------------
// ballot[c]: bit i = lane i of the wave hits at component c
static inline LS_RANGE_HD uint32_t ls_range_wave_total(const unsigned long long* ballot) {
    uint32_t t = 0;
    for (int c = 0; c < LS_RANGE_VEC; ++c) t += (uint32_t)__builtin_popcountll(ballot[c]);
    return t;
}
static inline LS_RANGE_HD uint32_t ls_range_lane_rank(const unsigned long long* ballot, int lane) {
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t r = 0;
    for (int c = 0; c < LS_RANGE_VEC; ++c) r += (uint32_t)__builtin_popcountll(ballot[c] & below);
    return r;
}
// hits of the lane's own thread at the components below c
static inline LS_RANGE_HD uint32_t ls_range_comp_rank(const unsigned long long* ballot, int lane, int c) {
    uint32_t r = 0;
    for (int j = 0; j < LS_RANGE_VEC; ++j) r += j < c ? (uint32_t)((ballot[j] >> lane) & 1ull) : 0u;
    return r;
}
// hits of the waves below wave w (totals: [LS_RANGE_WAVES] hits of every wave of the workgroup)
static inline LS_RANGE_HD uint32_t ls_range_wave_base(const uint32_t* totals, int w) {
    uint32_t b = 0;
    for (int i = 0; i < LS_RANGE_WAVES; ++i) b += i < w ? totals[i] : 0u;
    return b;
}
static inline LS_RANGE_HD uint32_t ls_range_slab_total(const uint32_t* totals) {
    uint32_t b = 0;
    for (int i = 0; i < LS_RANGE_WAVES; ++i) b += totals[i];
    return b;
}

// ---- the offsets kernel's deal ----------------------------------------------------------------------------------------
// slabs [begin, end) of thread `tid`: contiguous, so the threads' partial sums scan in slab order
static constexpr LS_RANGE_HD long long ls_range_seg_len(long long nslab) {
    return (nslab + LS_RANGE_OFF_THREADS - 1) / LS_RANGE_OFF_THREADS;
}
static constexpr LS_RANGE_HD long long ls_range_seg_begin(long long nslab, int tid) {
    return (long long)tid * ls_range_seg_len(nslab) < nslab ? (long long)tid * ls_range_seg_len(nslab) : nslab;
}
static constexpr LS_RANGE_HD long long ls_range_seg_end(long long nslab, int tid) {
    return ls_range_seg_begin(nslab, tid) + ls_range_seg_len(nslab) < nslab
               ? ls_range_seg_begin(nslab, tid) + ls_range_seg_len(nslab)
               : nslab;
}
