// ls_ivf_subset_plan.h — the host side of an IVF subset (include/leansearch_ivf_subset.h): a bitmap over ORIGINAL rows
// compacted list after list, in storage order. Plain inline functions over the handle's host tables (assign[n] and the
// lists' storage offsets off[nlist + 1]); no HIP, so a host program compiles them alone (tests/ivf_subset_check.cpp).
//
//   soff[nlist + 1]  offsets of the lists in the compacted arrays (a prefix of the selected rows per list)
//   srow[m]          storage row of every selected row, list after list; inside a list original-row ascending - which
//                    is storage-row ascending, the storage order of a list being original-row order
//   sid[m]           original row of every selected row, in the same order
//   top_rows[p]      the sum of the p largest selected-list sizes: the host's bound of the rows p probed lists can hold
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <vector>

struct ls_ivf_subset_plan {
    int64_t m = 0;
    std::vector<uint32_t> soff, srow, sid;
    std::vector<int64_t> top_rows;
};

// row r of a bitmap of nbytes bytes in ls_subset_create's layout; rows past a short bitmap are not selected
inline bool ls_ivf_subset_bit(const uint8_t* bitmap, int64_t nbytes, int64_t r) {
    const int64_t b = r >> 3;
    return b < nbytes && ((bitmap[b] >> (r & 7)) & 1);
}

// counts[l] = selected rows of list l (bits at r >= n are ignored); returns their sum
inline int64_t ls_ivf_subset_count(const int32_t* assign, int64_t n, int32_t nlist, const uint8_t* bitmap, int64_t nbytes,
                                   std::vector<int64_t>& counts) {
    counts.assign((size_t)nlist, 0);
    int64_t m = 0;
    const int64_t covered = std::min<int64_t>(n, nbytes * 8);
    for (int64_t r = 0; r < covered; ++r)
        if (ls_ivf_subset_bit(bitmap, nbytes, r)) {
            counts[(size_t)assign[r]]++;
            ++m;
        }
    return m;
}

// top[p] = sum of the p largest of counts, p = 0 .. nlist
inline void ls_ivf_subset_top_rows(const std::vector<int64_t>& counts, std::vector<int64_t>& top) {
    std::vector<int64_t> sorted(counts);
    std::sort(sorted.begin(), sorted.end(), std::greater<int64_t>());
    top.assign(sorted.size() + 1, 0);
    for (size_t p = 0; p < sorted.size(); ++p) top[p + 1] = top[p] + sorted[p];
}

// off[nlist + 1]: first storage row of every list of the handle (the counting sort of assign, ascending original row
// inside a list - ls_ivf.hip ivf_build)
inline void ls_ivf_subset_compact(const int32_t* assign, int64_t n, int32_t nlist, const uint32_t* off,
                                  const uint8_t* bitmap, int64_t nbytes, ls_ivf_subset_plan& out) {
    std::vector<int64_t> counts;
    out.m = ls_ivf_subset_count(assign, n, nlist, bitmap, nbytes, counts);
    ls_ivf_subset_top_rows(counts, out.top_rows);
    out.soff.assign((size_t)nlist + 1, 0);
    for (int32_t l = 0; l < nlist; ++l) out.soff[(size_t)l + 1] = out.soff[(size_t)l] + (uint32_t)counts[(size_t)l];
    out.srow.assign((size_t)out.m, 0);
    out.sid.assign((size_t)out.m, 0);
    if (out.m == 0) return;
    // one ascending pass over the original rows: `seen[l]` rows of list l lie before r, so r sits at storage row
    // off[l] + seen[l]; `at[l]` is where the list's next selected row goes
    std::vector<uint32_t> seen((size_t)nlist, 0), at(out.soff.begin(), out.soff.end() - 1);
    for (int64_t r = 0; r < n; ++r) {
        const size_t l = (size_t)assign[r];
        const uint32_t s = off[l] + seen[l]++;
        if (ls_ivf_subset_bit(bitmap, nbytes, r)) {
            const uint32_t x = at[l]++;
            out.srow[x] = s;
            out.sid[x] = (uint32_t)r;
        }
    }
}
