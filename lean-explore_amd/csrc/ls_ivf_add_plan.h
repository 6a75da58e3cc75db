// ls_ivf_add_plan.h — where the rows of an IVF handle go when ls_ivf_add (include/leansearch_ivf_add.h) merges n_add
// new rows into it. Plain inline functions (no HIP): ls_ivf_mutate.hip and ls_rows.hip's row mover take every index
// from here, and tests/ivf_add_plan_check.cpp compiles this header alone to compare it with a from-scratch counting
// sort of the concatenated assignment. The row mover's deal: ls_rows_plan.h.
//
// Placement. Storage is list after list, ascending by original row inside a list. New rows carry the original rows
// n_old .. n_old + n_add - 1, all above the old ones, so list l of the new storage is its old rows [off_old[l],
// off_old[l + 1]) in their order followed by its new rows in call order:
//   off_new[l]  first storage row of list l                       (off_new[nlist] = n_old + n_add)
//   src[s]      what destination storage row s holds: a value below n_old is that OLD storage row, any other value
//               is new row src[s] - n_old of the call
//   shift[l]    off_new[l] - off_old[l] >= 0: how far the old rows of list l move (an existing subset's storage rows)
// The original row of destination s needs no table of its own: ls_ivf_add_id below, from src[s] and the old ids.
#pragma once
#include <cstdint>
#include <vector>

#include "ls_rows_plan.h"

struct ls_ivf_add_plan {
    std::vector<uint32_t> off_new;  // [nlist + 1]
    std::vector<uint32_t> src;      // [n_old + n_add]
    std::vector<int64_t> sizes;     // [nlist] rows of every list after the add
    std::vector<uint32_t> shift;    // [nlist]
};

// off_old: [nlist + 1] of the handle (off_old[nlist] = n_old); assign_add: [n_add], every entry in [0, nlist) (the
// caller has checked them); n_old + n_add < 2^32 - 1.
static inline void ls_ivf_add_plan_make(const uint32_t* off_old, int32_t nlist, const int32_t* assign_add, int64_t n_add,
                                        ls_ivf_add_plan& p) {
    const int64_t n_old = off_old[nlist];
    p.sizes.assign((size_t)nlist, 0);
    for (int32_t l = 0; l < nlist; ++l) p.sizes[(size_t)l] = (int64_t)off_old[l + 1] - off_old[l];
    for (int64_t j = 0; j < n_add; ++j) p.sizes[(size_t)assign_add[j]]++;
    p.off_new.assign((size_t)nlist + 1, 0);
    for (int32_t l = 0; l < nlist; ++l) p.off_new[(size_t)l + 1] = p.off_new[(size_t)l] + (uint32_t)p.sizes[(size_t)l];
    p.shift.resize((size_t)nlist);
    p.src.resize((size_t)(n_old + n_add));
    std::vector<uint32_t> at((size_t)nlist);  // where the next new row of every list goes
    for (int32_t l = 0; l < nlist; ++l) {
        const uint32_t cnt = off_old[l + 1] - off_old[l];
        p.shift[(size_t)l] = p.off_new[(size_t)l] - off_old[l];
        for (uint32_t j = 0; j < cnt; ++j) p.src[(size_t)p.off_new[(size_t)l] + j] = off_old[l] + j;
        at[(size_t)l] = p.off_new[(size_t)l] + cnt;
    }
    for (int64_t j = 0; j < n_add; ++j) p.src[at[(size_t)assign_add[j]]++] = (uint32_t)(n_old + j);
}

// original row of the destination storage row whose source is `src` (ids_old: storage row -> original row, [n_old])
static inline LS_ROWS_HD uint32_t ls_ivf_add_id(uint32_t src, uint32_t n_old, const uint32_t* ids_old) {
    return src < n_old ? ids_old[src] : src;
}
