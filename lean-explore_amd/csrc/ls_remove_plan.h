// ls_remove_plan.h — where the rows of a flat handle go when ls_remove (include/leansearch_remove.h) drops the rows a
// bitmap selects. Plain inline functions (no HIP): ls_remove.hip and ls_shard.hip take every index from here, and
// tests/remove_plan_check.cpp compiles this header alone to hold it to a sequential model.
//
// Placement. Survivors are renumbered densely: old row r becomes r - (removed rows below r). With
//   n_new    surviving rows
//   r0       the first removed row (n_old when none is removed): rows below r0 keep their place
//   src[s]   the old row of new row s, ascending, src[s] >= s, src[s] == s for s < r0
// the corpus is compacted IN PLACE through a staging buffer of R rows, slab after slab of destination rows from r0
// upwards. Slab j covers the destination rows [a_j, a_j + c_j), a_j = r0 + j * R, c_j = min(R, n_new - a_j):
//   gather      staging row i takes the stored bytes of old row src[a_j + i]
//   write-back  rows [a_j, a_j + c_j) of the corpus take the staging rows
// Why no row is read after it was overwritten:
//   - src[s] >= s (s survivors lie below new row s, each at its own old row below src[s]), and src ascends, so slab j
//     reads only old rows >= src[a_j] >= a_j;
//   - the slabs before j wrote only rows < a_j;
//   - inside a slab the gather precedes the write-back in stream order, and the gather writes the staging buffer only.
// So every read of slab j sees the bytes the row had before the call.
//
// The deals of the row mover (over the rows of one slab) and of the subsets' compaction: ls_rows_plan.h. An existing
// subset is the ascending list of its m rows, cut into segments of LS_RM_SEG positions; an exclusive scan of the
// segments' counts gives every segment's base.
//
// A shard of a sharded handle takes the bits [lo, lo + n) of the group's bitmap: ls_remove_slice realigns them to a
// byte (bit (lo & 7) + r of the slice is local row r), complemented for the survivor list. After the removal the
// shards' row blocks are contiguous again: ls_remove_new_lo.
#pragma once
#include <cstdint>
#include <vector>

#include "ls_rows_plan.h"

#define LS_RM_SEG (LS_LIST_THREADS * 32)  // list positions of one segment of a subset's list (32 steps)
#define LS_RM_STAGE_BYTES (256ll << 20)   // the automatic staging buffer (upload_rows' and ls_reconstruct's slab)

// ---- a handle's slice of the bitmap -----------------------------------------------------------------------------------
// bytes of the slice that holds the bits [bit0, bit0 + n), realigned to a byte
static inline int64_t ls_remove_slice_bytes(int64_t bit0, int64_t n) { return ((bit0 & 7) + n + 7) / 8; }
// The slice itself: byte i is byte (bit0 >> 3) + i of the bitmap (0 past its end), so bit (bit0 & 7) + r is local row
// r; with `complement` every byte is inverted (set = the row STAYS: rows past a short bitmap stay).
static inline void ls_remove_slice(const uint8_t* bitmap, int64_t nbytes, int64_t bit0, int64_t n, bool complement,
                                   std::vector<uint8_t>& out) {
    const int64_t need = ls_remove_slice_bytes(bit0, n), byte0 = bit0 >> 3;
    out.assign((size_t)need, 0);
    for (int64_t i = 0; i < need && byte0 + i < nbytes; ++i) out[(size_t)i] = bitmap[byte0 + i];
    if (complement)
        for (auto& b : out) b = (uint8_t)~b;
}
// The first local row < n the bits [bit0, bit0 + n) select, n when there is none (r0)
static inline int64_t ls_remove_first(const uint8_t* bitmap, int64_t nbytes, int64_t bit0, int64_t n) {
    int64_t r = 0;
    while (r < n) {
        const int64_t b = bit0 + r;
        if ((b >> 3) >= nbytes) return n;
        if ((b & 7) == 0 && r + 8 <= n && bitmap[b >> 3] == 0) {  // a whole clear byte
            r += 8;
            continue;
        }
        if ((bitmap[b >> 3] >> (b & 7)) & 1) return r;
        ++r;
    }
    return n;
}
// rows the bits [bit0, bit0 + n) select
static inline int64_t ls_remove_count(const uint8_t* bitmap, int64_t nbytes, int64_t bit0, int64_t n) {
    int64_t m = 0;
    for (int64_t r = 0; r < n && ((bit0 + r) >> 3) < nbytes; ++r) m += ls_rows_bit(bitmap, nbytes, bit0 + r) ? 1 : 0;
    return m;
}

// ---- the slabs --------------------------------------------------------------------------------------------------------
// rows that change place: the destination rows [r0, n_new)
static inline int64_t ls_remove_moved(int64_t r0, int64_t n_new) { return n_new > r0 ? n_new - r0 : 0; }
// rows per slab: `want` > 0 as the caller set it, else as many stored rows as fit LS_RM_STAGE_BYTES; at least one, at
// most the rows that move (0 when none does: no staging buffer)
static inline int64_t ls_remove_slab_rows(int64_t want, int64_t row_bytes, int64_t moved) {
    if (moved <= 0) return 0;
    int64_t R = want > 0 ? want : LS_RM_STAGE_BYTES / (row_bytes > 0 ? row_bytes : 1);
    if (R < 1) R = 1;
    return R < moved ? R : moved;
}
static inline int64_t ls_remove_slabs(int64_t r0, int64_t n_new, int64_t R) {
    const int64_t moved = ls_remove_moved(r0, n_new);
    return moved > 0 && R > 0 ? (moved + R - 1) / R : 0;
}
// slab j: its first destination row and its rows
static inline int64_t ls_remove_slab_begin(int64_t r0, int64_t R, int64_t j) { return r0 + j * R; }
static inline int64_t ls_remove_slab_count(int64_t r0, int64_t n_new, int64_t R, int64_t j) {
    const int64_t a = ls_remove_slab_begin(r0, R, j);
    return n_new - a < R ? n_new - a : R;
}

// segments of a list of m positions
static inline long long ls_remove_segs(long long m) { return m < 1 ? 1 : (m + LS_RM_SEG - 1) / LS_RM_SEG; }

// ---- a sharded handle -------------------------------------------------------------------------------------------------
// rows[g]: the rows shard g holds after the removal -> lo[g], the first row of its block (relative to the group's
// base); returns the group's rows
static inline int64_t ls_remove_new_lo(const int64_t* rows, int G, int64_t* lo) {
    int64_t at = 0;
    for (int g = 0; g < G; ++g) {
        lo[g] = at;
        at += rows[g];
    }
    return at;
}
