// ls_ivf_remove_plan.h — where the rows of an IVF handle go when ls_ivf_remove (include/leansearch_ivf_remove.h) drops
// the rows a bitmap selects. Plain inline functions (no HIP): ls_ivf_mutate.hip takes every index from here, and
// tests/ivf_remove_plan_check.cpp compiles this header alone to compare it with a from-scratch counting sort of the
// surviving assignment. The deals of the row mover and of the subsets' compaction (one segment per list: soff[l] ..
// soff[l + 1]): ls_rows_plan.h.
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
//   dst_of[t]    the destination storage row of old storage row t, or LS_ROWS_GONE when its row is removed
#pragma once
#include <cstdint>
#include <vector>

#include "ls_rows_plan.h"

struct ls_ivf_remove_plan {
    int64_t n_new = 0;
    std::vector<int32_t> assign_new;  // [n_new]
    std::vector<int64_t> sizes;       // [nlist]
    std::vector<uint32_t> off_new;    // [nlist + 1]
    std::vector<uint32_t> src;        // [n_new]
    std::vector<uint32_t> ids_new;    // [n_new]
    std::vector<uint32_t> dst_of;     // [n_old]
};

// rows the bitmap selects below n (bits at r >= n are ignored)
static inline int64_t ls_ivf_remove_count(const uint8_t* bitmap, int64_t nbytes, int64_t n) {
    int64_t m = 0;
    const int64_t covered = n < nbytes * 8 ? n : nbytes * 8;
    for (int64_t r = 0; r < covered; ++r) m += ls_rows_bit(bitmap, nbytes, r) ? 1 : 0;
    return m;
}

// assign: [n] of the handle, every entry in [0, nlist); off_old: [nlist + 1] (off_old[nlist] = n).
static inline void ls_ivf_remove_plan_make(const int32_t* assign, int64_t n, int32_t nlist, const uint32_t* off_old,
                                           const uint8_t* bitmap, int64_t nbytes, ls_ivf_remove_plan& p) {
    p.sizes.assign((size_t)nlist, 0);
    p.n_new = 0;
    for (int64_t r = 0; r < n; ++r)
        if (!ls_rows_bit(bitmap, nbytes, r)) {
            p.sizes[(size_t)assign[r]]++;
            p.n_new++;
        }
    p.off_new.assign((size_t)nlist + 1, 0);
    for (int32_t l = 0; l < nlist; ++l) p.off_new[(size_t)l + 1] = p.off_new[(size_t)l] + (uint32_t)p.sizes[(size_t)l];
    p.assign_new.resize((size_t)p.n_new);
    p.src.resize((size_t)p.n_new);
    p.ids_new.resize((size_t)p.n_new);
    p.dst_of.assign((size_t)n, LS_ROWS_GONE);
    // one ascending pass over the old original rows: `seen[l]` rows of list l lie before r, so r sits at old storage row
    // off_old[l] + seen[l]; `at[l]` is where the list's next survivor goes; `r_new` survivors lie before r
    std::vector<uint32_t> seen((size_t)nlist, 0), at(p.off_new.begin(), p.off_new.end() - 1);
    int64_t r_new = 0;
    for (int64_t r = 0; r < n; ++r) {
        const size_t l = (size_t)assign[r];
        const uint32_t t = off_old[l] + seen[l]++;
        if (ls_rows_bit(bitmap, nbytes, r)) continue;
        const uint32_t s = at[l]++;
        p.src[s] = t;
        p.ids_new[s] = (uint32_t)r_new;
        p.dst_of[t] = s;
        p.assign_new[(size_t)r_new++] = (int32_t)l;
    }
}
