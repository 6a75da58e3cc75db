// ls_ivf_build_plan.h — how ls_ivf_build.hip's two kernels deal their work: the tiles of the assignment kernel, its
// walk over the centroids, and the blocks the means kernel cuts the assignment into. Plain inline functions (no HIP):
// the kernels and their launcher take every index from here, and tests/ivf_build_plan_check.cpp compiles this header
// alone to enumerate them on the host.
//
// Assignment (ls_ivf_assign_kernel<L, V, U>): a tile is U * (64 / L) rows, U = scan_unroll(V) - the scan kernel's tile.
// The launch has ls_scan_blocks_lv workgroups (at least 4 tiles per wave, at most 2 workgroups per CU) of 4 waves; wave
// gw of W takes tiles gw, gw + W, ... (the scan's round-robin deal). Slot (u, grp) of tile t is row t * TR + u * R + grp;
// a slot past the last row loads row n - 1 again and writes nothing. For every tile the wave walks ALL centroids, in
// batches of ls_ivfb_cent_batch(V) consecutive ones (a batch is loaded while the previous one is scored); a batch entry
// past the last centroid loads centroid nlist - 1 again and is not scored.
#pragma once
#include "ls_scan_plan.h"

#define LS_IVFB_MAX_NLIST 8191    // nlist < 8192: every route of ls_search over the centroids scores in scan order
#define LS_IVFB_MEANS_BLOCK 256   // rows of the assignment one step of the means kernel compacts (= its threads)
#define LS_IVFB_MEANS_AHEAD 8     // member rows whose loads the means kernel issues ahead of their adds

struct ls_ivfb_deal {
    long long n;   // rows
    long long NT;  // tiles
    long long W;   // waves of the launch
    int R;         // rows per wave load step (64 / L)
    int TR;        // rows per tile
    int blocks;    // workgroups
};

static inline int ls_ivfb_blocks(int64_t n, int L, int V, int32_t n_cu) { return ls_scan_blocks_lv(n, L, V, n_cu); }

static inline ls_ivfb_deal ls_ivfb_deal_make(long long n, int L, int V, int blocks) {
    ls_ivfb_deal d;
    d.n = n;
    d.R = LS_WAVE / L;
    d.TR = ls_scan_tile_rows(L, scan_unroll(V));
    d.NT = (n + d.TR - 1) / d.TR;
    d.blocks = blocks;
    d.W = (long long)blocks * LS_SCAN_WAVES;
    return d;
}
// the step-th tile of wave gw (the wave is done at the first one >= NT)
static constexpr long long ls_ivfb_tile(long long W, long long gw, long long step) { return gw + step * W; }
// row of slot (u, grp) of tile t; ls_ivfb_row_valid: it exists; ls_ivfb_row_load: the row the slot loads (n >= 1)
static constexpr long long ls_ivfb_row(long long t, int TR, int R, int u, int grp) { return t * TR + (long long)u * R + grp; }
static constexpr bool ls_ivfb_row_valid(long long row, long long n) { return row < n; }
static constexpr long long ls_ivfb_row_load(long long row, long long n) { return row < n ? row : n - 1; }

// centroids per batch: two batches are live (the one being scored, the one in flight), 8 * CB * V registers
static constexpr int ls_ivfb_cent_batch(int V) { return V >= 3 ? 2 : 4; }
static constexpr int ls_ivfb_cent_batches(int nlist, int CB) { return (nlist + CB - 1) / CB; }
static constexpr int ls_ivfb_cent(int batch, int CB, int j) { return batch * CB + j; }
static constexpr bool ls_ivfb_cent_valid(int c, int nlist) { return c < nlist; }
static constexpr int ls_ivfb_cent_load(int c, int nlist) { return c < nlist ? c : nlist - 1; }

// means kernel: steps over assign[0, n) and the rows one step covers
static constexpr long long ls_ivfb_means_steps(long long n) { return (n + LS_IVFB_MEANS_BLOCK - 1) / LS_IVFB_MEANS_BLOCK; }
static constexpr long long ls_ivfb_means_row(long long step, int tid) { return step * LS_IVFB_MEANS_BLOCK + tid; }
