// ls_scan_plan.h — how a scan launch is planned on the host: tile rows, the SMALL decision, workgroups per launch and
// k'. Plain C++ (no HIP): every launcher and orchestration file takes the rules from here, and tests/scan_plan_check.cpp
// compiles this header alone to hold tests/test_geometry_cpu.py's restatement of them to the code.
#pragma once
#include <algorithm>
#include <cstdint>

#define LS_WAVE 64
#define LS_SCAN_THREADS 256          // 4 waves per scan workgroup
#define LS_SCAN_WAVES (LS_SCAN_THREADS / LS_WAVE)
#define LS_KP_MAX 16                 // per-workgroup emitted candidates (k') + 1 bound
#define LS_MQ_KP_MAX 24              // ... of an ls_mq workgroup (it ranks waves x keys-per-lane of them; c_stride has the room)
#define LS_FINAL_CAP 8192            // keys the finalize workgroup sorts in LDS (64 KiB)
#define LS_GRAN_MAX 4096             // granules per query: blocks * (kprime + 1) above this -> own launch
#ifndef LS_SCAN_SMALL
#define LS_SCAN_SMALL 1              // small shards: waves rank their <= 64 keys once instead of inserting row by row
#endif
#ifndef LS_SCAN_SMALL_ROWS
#define LS_SCAN_SMALL_ROWS 64        // ... when no wave sees more rows than this (<= 64: one key per lane)
#endif
#ifndef LS_SCAN_SMALL_MAX_BLOCKS
#define LS_SCAN_SMALL_MAX_BLOCKS 256 // ... and the launch has at most one scan workgroup per CU
#endif

// row groups in flight per wave (U): a tile is U * (64 / L) rows
#ifndef LS_UNROLL_V3
#define LS_UNROLL_V3 4
#endif
static constexpr int scan_unroll(int V) { return (V >= 3) ? LS_UNROLL_V3 : 8; }  // >= 8 loads in flight
// ... of the SMALL variant. (the SMALL row-list kernel of sq8 rows with 4-chunk lanes spills 16 bytes per lane at
// U = 4: two row groups in flight there. U shapes the tiles only, never a score)
static constexpr int ls_scan_small_unroll(int V, bool sq8_rowlist) { return (sq8_rowlist && V == 4) ? 2 : scan_unroll(V); }
static constexpr int ls_scan_tile_rows(int L, int U) { return U * (LS_WAVE / L); }

// SMALL: single-query launches in which no wave sees more than 64 rows rank once instead of inserting.
// tile_rows: of the SMALL variant the launch would run.
// (with two or more workgroups per CU the other one hides the latency: measured neutral at
// N = 50 k, 3 % slower at 100 k, 6-11 % faster at 25 k and 10 k)
static inline bool ls_scan_is_small(long long rows, int blocks, int tile_rows, int nq) {
    const long long waves = (long long)blocks * LS_SCAN_WAVES;
    const long long tiles_per_wave = ((rows + tile_rows - 1) / tile_rows + waves - 1) / waves;
    return LS_SCAN_SMALL && nq == 1 && tiles_per_wave * tile_rows <= LS_SCAN_SMALL_ROWS &&
           blocks <= LS_SCAN_SMALL_MAX_BLOCKS;
}

// scan workgroups of a launch over n rows of (L, V) lanes on n_cu CUs (ls_scan_blocks)
static inline int ls_scan_blocks_lv(int64_t n, int L, int V, int32_t n_cu) {
    constexpr int bpc = 2;  // scan workgroups per CU
    const int64_t TR = ls_scan_tile_rows(L, scan_unroll(V));
    const int64_t NT = (n + TR - 1) / TR;
    // minimum tiles per wave. Small shards: fewer blocks -> fewer candidate keys for the
    // piggy-backed finalize, which bounds the launch there (N=25k: 18.6 -> 11.7 us/step)
    constexpr int tpw = 4;
    int64_t b = (NT + LS_SCAN_WAVES * tpw - 1) / (LS_SCAN_WAVES * tpw);
    const int64_t cap = (int64_t)n_cu * bpc;
    if (b > cap) {
        // Big shards: tiles are dealt round-robin to 4*b waves, so the launch ends with a partial
        // round in which only frac(NT / 4b) of the waves still have a tile - too few to keep HBM
        // busy. Measured on config 2 (25 000 tiles): 512 workgroups (12.2 rounds) 47.55 us,
        // 448 (13.95 rounds) 47.03 us; config 2' 123.2 vs 120.4 us (tools/scan_blocks_sweep.py).
        // Pick the count in [1.5, 2] workgroups per CU (multiples of the 8 XCDs) whose last round
        // is the fullest.
        int64_t best = cap;
        double best_fill = -1.0;
        for (int64_t c = cap; c >= cap * 3 / 4; c -= 8) {
            const double rounds = (double)NT / (double)(c * LS_SCAN_WAVES);
            double fill = rounds - (double)(int64_t)rounds;
            if (fill == 0.0) fill = 1.0;
            if (fill > best_fill + 0.02) {  // near-ties go to the larger count
                best_fill = fill;
                best = c;
            }
        }
        b = best;
    }
    if (b < 1) b = 1;
    return (int)b;
}

// k' (keys each scan workgroup emits) from lambda = expected top-k rows per workgroup: lambda + 5 sqrt(lambda) + 3 ...
static inline int ls_kprime_raw(int64_t keff, int blocks) {
    const double lam = (double)keff / (double)blocks;
    return (int)(lam + 5.0 * __builtin_sqrt(lam) + 3.0);
}
// ... at least 2, below the kernel's kp_max, and so that the finalize workgroup holds every emitted key
static inline int ls_kprime(int blocks, int keff, int kp_max) {
    int kp = ls_kprime_raw(keff, blocks);
    kp = std::max(kp, 2);
    kp = std::min(kp, kp_max - 1);
    while (kp > 1 && (int64_t)blocks * kp > LS_FINAL_CAP) --kp;
    return kp;
}
