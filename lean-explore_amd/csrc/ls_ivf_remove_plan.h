// ls_ivf_remove_plan.h — where the rows of an IVF handle go when ls_ivf_remove (include/leansearch_ivf_remove.h) drops
// the rows a bitmap selects, and how ls_ivf_remove.hip's kernels deal their work. Plain inline functions (no HIP):
// ls_ivf.hip and the kernels take every index from here, and tests/ivf_remove_plan_check.cpp compiles this header alone
// to compare it with a from-scratch counting sort of the surviving assignment.
//
// Placement. Storage is list after list, ascending by original row inside a list. Survivors are renumbered densely -
// old original row r becomes r - (removed rows below r) - and the renumbering is monotone, so list l of the new storage
// is the surviving rows of its old storage rows [off_old[l], off_old[l + 1]) in their order:
//   n_new        surviving rows
//   assign_new   [n_new] the list of every survivor, under its new number
//   sizes        [nlist] rows of every list after the removal
//   off_new      [nlist + 1] first storage row of every list (off_new[nlist] = n_new)
//   src[s]       the OLD storage row destination storage row s holds
//   ids_new[s]   the NEW original row of destination storage row s
//   dst_of[t]    the destination storage row of old storage row t, or LS_IVFR_GONE when its row is removed
//
// Deal of the row kernel: ls_ivf_add_plan.h's tile deal (one lane per 16-byte chunk; as many whole rows as fit a wave,
// one strided row from 64 chunks on; wave gw of W takes tiles gw, gw + W, ...).
//
// Deal of the subset kernels. An existing subset holds, per list l, the storage rows srow[soff[l] .. soff[l + 1])
// ascending. Workgroup b of G takes lists b, b + G, ...; a list's segment is walked in steps of LS_IVFR_THREADS
// positions, thread t of step i looking at position soff[l] + i * LS_IVFR_THREADS + t. A position survives when
// dst_of[srow[position]] != LS_IVFR_GONE. Inside a step the survivors are ranked in thread order: a wave's ballot gives
// the lane's rank among its wave (ls_ivf_remove_lane_rank), the waves' totals - through LDS - the wave's base
// (ls_ivf_remove_wave_base), and the survivors of the earlier steps the step's base. The count kernel adds the same
// ballots' popcounts up.
#pragma once
#include <cstdint>
#include <vector>

#include "ls_ivf_add_plan.h"

#define LS_IVFR_GONE 0xffffffffu
#define LS_IVFR_THREADS 256  // threads of a subset-kernel workgroup (4 waves)
#define LS_IVFR_WAVES (LS_IVFR_THREADS / LS_IVFA_WAVE)
#define LS_IVFR_MAX_GROUPS 4096  // workgroups of a subset-kernel launch at most (grid-strided over the lists)

struct ls_ivf_remove_plan {
    int64_t n_new = 0;
    std::vector<int32_t> assign_new;  // [n_new]
    std::vector<int64_t> sizes;       // [nlist]
    std::vector<uint32_t> off_new;    // [nlist + 1]
    std::vector<uint32_t> src;        // [n_new]
    std::vector<uint32_t> ids_new;    // [n_new]
    std::vector<uint32_t> dst_of;     // [n_old]
};

// row r of a bitmap of nbytes bytes in ls_subset_create's layout; rows past a short bitmap are not selected
static inline bool ls_ivf_remove_bit(const uint8_t* bitmap, int64_t nbytes, int64_t r) {
    const int64_t b = r >> 3;
    return b < nbytes && ((bitmap[b] >> (r & 7)) & 1);
}

// rows the bitmap selects below n (bits at r >= n are ignored)
static inline int64_t ls_ivf_remove_count(const uint8_t* bitmap, int64_t nbytes, int64_t n) {
    int64_t m = 0;
    const int64_t covered = n < nbytes * 8 ? n : nbytes * 8;
    for (int64_t r = 0; r < covered; ++r) m += ls_ivf_remove_bit(bitmap, nbytes, r) ? 1 : 0;
    return m;
}

// assign: [n] of the handle, every entry in [0, nlist); off_old: [nlist + 1] (off_old[nlist] = n).
static inline void ls_ivf_remove_plan_make(const int32_t* assign, int64_t n, int32_t nlist, const uint32_t* off_old,
                                           const uint8_t* bitmap, int64_t nbytes, ls_ivf_remove_plan& p) {
    p.sizes.assign((size_t)nlist, 0);
    p.n_new = 0;
    for (int64_t r = 0; r < n; ++r)
        if (!ls_ivf_remove_bit(bitmap, nbytes, r)) {
            p.sizes[(size_t)assign[r]]++;
            p.n_new++;
        }
    p.off_new.assign((size_t)nlist + 1, 0);
    for (int32_t l = 0; l < nlist; ++l) p.off_new[(size_t)l + 1] = p.off_new[(size_t)l] + (uint32_t)p.sizes[(size_t)l];
    p.assign_new.resize((size_t)p.n_new);
    p.src.resize((size_t)p.n_new);
    p.ids_new.resize((size_t)p.n_new);
    p.dst_of.assign((size_t)n, LS_IVFR_GONE);
    // one ascending pass over the old original rows: `seen[l]` rows of list l lie before r, so r sits at old storage row
    // off_old[l] + seen[l]; `at[l]` is where the list's next survivor goes; `r_new` survivors lie before r
    std::vector<uint32_t> seen((size_t)nlist, 0), at(p.off_new.begin(), p.off_new.end() - 1);
    int64_t r_new = 0;
    for (int64_t r = 0; r < n; ++r) {
        const size_t l = (size_t)assign[r];
        const uint32_t t = off_old[l] + seen[l]++;
        if (ls_ivf_remove_bit(bitmap, nbytes, r)) continue;
        const uint32_t s = at[l]++;
        p.src[s] = t;
        p.ids_new[s] = (uint32_t)r_new;
        p.dst_of[t] = s;
        p.assign_new[(size_t)r_new++] = (int32_t)l;
    }
}

// ---- the subset kernels' deal ---------------------------------------------------------------------------------------
// workgroups of a launch over nlist lists
static inline int ls_ivf_remove_groups(int nlist) { return nlist < 1 ? 1 : (nlist > LS_IVFR_MAX_GROUPS ? LS_IVFR_MAX_GROUPS : nlist); }
// steps a segment of `len` positions takes
static constexpr LS_IVFA_HD uint32_t ls_ivf_remove_steps(uint32_t len) { return (len + LS_IVFR_THREADS - 1) / LS_IVFR_THREADS; }
// the position thread `tid` looks at in step `step` of the segment that begins at `begin` (64-bit: begin + len < 2^32,
// the last step may reach past it)
static constexpr LS_IVFA_HD long long ls_ivf_remove_pos(uint32_t begin, uint32_t step, int tid) {
    return (long long)begin + (long long)step * LS_IVFR_THREADS + tid;
}
// survivors of the lane's wave in the lanes below it (ballot: bit i = lane i survives)
static inline LS_IVFA_HD uint32_t ls_ivf_remove_lane_rank(unsigned long long ballot, int lane) {
    return (uint32_t)__builtin_popcountll(ballot & ((1ull << lane) - 1ull));
}
// survivors of the step in the waves below wave w (totals: [LS_IVFR_WAVES] survivors of every wave of the step)
static inline LS_IVFA_HD uint32_t ls_ivf_remove_wave_base(const uint32_t* totals, int w) {
    uint32_t b = 0;
    for (int i = 0; i < LS_IVFR_WAVES; ++i) b += i < w ? totals[i] : 0u;
    return b;
}
static inline LS_IVFA_HD uint32_t ls_ivf_remove_step_total(const uint32_t* totals) {
    uint32_t b = 0;
    for (int i = 0; i < LS_IVFR_WAVES; ++i) b += totals[i];
    return b;
}
