// ls_mq_kernel.h — the small-batch kernel template of an fp32 index (see ls_mq.hip for the work decomposition and the
// bit-identity with the scan kernel). A header so that the row-list instantiations (ls_mq_subset.hip) compile in their
// own translation unit; ls_mq.hip instantiates the plain kernels from the same text.
#pragma once
#include "ls_mq_dev.h"

#include <type_traits>

// (LS_MQ_WAVES / LS_MQ_WAVES2, the waves per workgroup with one / two B blocks, and the LDS sizes: ls_mq_plan.h)
#ifndef LS_MQ_P1
#define LS_MQ_P1 0           // variant builds: ring depth in units, one B block (0: 2 V)
#endif
#ifndef LS_MQ_P2
#define LS_MQ_P2 0           // ... two B blocks (0: 2 V)
#endif

// 4 x 4 transpose across the four 16-lane groups: in: lane group g, register m = T[m][g];
// out: register m of lane group g = T[g][m]
__device__ __forceinline__ void mq_transpose(const mq_f32x4& x, float (&r)[4]) {
    u32 r0 = __builtin_bit_cast(u32, (float)x[0]), r1 = __builtin_bit_cast(u32, (float)x[1]);
    u32 r2 = __builtin_bit_cast(u32, (float)x[2]), r3 = __builtin_bit_cast(u32, (float)x[3]);
    const auto a = __builtin_amdgcn_permlane32_swap(r0, r2, false, false);  // rows 2,3 of r0 <-> rows 0,1 of r2
    const auto b = __builtin_amdgcn_permlane32_swap(r1, r3, false, false);
    const auto c = __builtin_amdgcn_permlane16_swap((u32)a[0], (u32)b[0], false, false);  // odd rows <-> even rows
    const auto e = __builtin_amdgcn_permlane16_swap((u32)a[1], (u32)b[1], false, false);
    r[0] = __builtin_bit_cast(float, (u32)c[0]);
    r[1] = __builtin_bit_cast(float, (u32)c[1]);
    r[2] = __builtin_bit_cast(float, (u32)e[0]);
    r[3] = __builtin_bit_cast(float, (u32)e[1]);
}

// mq_pitch (ls_mq_plan.h), floats between two queries in LDS: the stored row + 2. The LDS serves a wave's 64 lanes as two halves of 32 over
// 32 banks: the first half of a B fragment read is (query li = 0..15, k = 0..1) at li * pitch + k + 4c, so a pitch
// of 2 (mod 32) puts it on banks 2 li + k - all 32 - and the second half (k = 2, 3) likewise; a staging write
// (one query, 64 consecutive elements) is conflict-free under any pitch. PMC, 16 queries, d = 384:
// SQ_LDS_BANK_CONFLICT / SQ_INSTS_LDS = 0.019 (round 5's [chunk][k][query] layout: 0.24, all of it staging
// writes; a pitch of 4 (mod 64) - right for 64 banks - measured 3.8: half of all LDS cycles).

// NB = MFMA B blocks (16 query columns each) per A operand: 1 serves 2..16 queries, 2 serves 17..32.
// WPB = waves per workgroup (4, 8 with two blocks).
// RowList: empty, or `const u32*` - the subset pass (ls_mq_subset.hip, NB == 1): `n` then counts positions in an
// ascending list of selected rows and everything but the row loads (tiles, S, keys, bounds, selection) works in
// positions: lane (li, kq) loads chunk cb + kq of row list[t * 16 + li]. A wave holds the list entries of its next tile
// and fetches those of the tile after it while the current tile streams: the ring's refills reach into the next tile,
// and no row load waits for a list load of its own tile. Positions >= n (the ragged last tile, a prefetch past the
// wave's last tile) read list[n - 1]: nothing is read past the list, and no row that is not selected. The
// instantiations without a list are the plain pass, unchanged.
// RowList = mq_union_src (ls_mq_dev.h) - the IVF union pass (ls_ivf_batch.hip, NB == 1): the row-list form over the rows
// of the lists a group of queries probes, with three differences. `n` is read from device memory (src.m; the argument is
// the host's upper bound and unused): tiles at or past it are skipped wave-uniformly, workgroups without a tile emit
// empty candidates and a zero bound. A position also yields its ORIGINAL row and the mask of the group's queries that
// probe its list: a row enters only the lists of those queries, and the keys carry the original row (mq_take_scores_union).
// No score vectors are written. Row loads clamp to position n - 1 (to position 0 of an empty union: one row of the
// corpus is then read and masked); the id / mask arrays are padded to whole tiles, nothing is read past them.
template <int L, int V, int M, int NB, int WPB, typename... RowList>
__global__ __launch_bounds__(64 * WPB, WPB == 4 ? 2 : 1) void ls_mq_kernel(
    const mq_f32x4* __restrict__ corpus, long long n, const float* __restrict__ qraw, int d, int nq,
    int normalize, float* __restrict__ S, long long s_stride, u64* __restrict__ cand, long long c_stride,
    u64* __restrict__ bound, long long b_stride, int kprime, int nfin, ls_fin_batch fin,
    void* __restrict__ gran, long long g_stride, u32 tag, float* __restrict__ qkeep, RowList... rowlist) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_dyn[];
    // the first `nfin` workgroups run selection jobs (of the previous launch, or - same-launch hand-off -
    // of this launch's own queries), exactly as in ls_scan_kernel
    if ((int)blockIdx.x < nfin) {
        for (int j = blockIdx.x; j < fin.njobs; j += nfin) {  // (nfin workgroups share the fin.njobs jobs)
            if (j != (int)blockIdx.x) __syncthreads();
            finalize_body<64 * WPB>(ls_fin_job(fin, j), smem_dyn, threadIdx.x);
        }
        return;
    }
#ifdef LS_SCAN_TIMING  // developer instrumentation: phase stamps (100 MHz ticks) of one workgroup
    unsigned long long stamp[8] = {};
    int tiles_done = 0;
#define LS_MQSTAMP(i) stamp[i] = wall_clock64()
#else
#define LS_MQSTAMP(i) do {} while (0)
#endif
    LS_MQSTAMP(0);
    constexpr int CH = L * V;              // 16-byte chunks per stored row
    constexpr int NU = CH / 4;             // load units per tile (4 chunks = 64 bytes per row each)
    constexpr int GC = NB == 1 ? 16 : 8;   // chains per accumulator group (32 for 4 KB rows - 512 contiguous bytes per row and
                                           // round instead of 256, 226 registers - is exact and slower: 137.3 vs 134.4 us)
    constexpr int NG = L / GC;             // accumulator groups
    constexpr int UPG = V * GC / 4;        // units per group
    constexpr int PREQ = NB == 1 ? LS_MQ_P1 : LS_MQ_P2;
    constexpr int P = (PREQ > 0 && NU % PREQ == 0) ? PREQ : 2 * V;  // units in flight per lane (1 KB per wave each)
    constexpr int DP = mq_pitch(CH);       // floats between two queries in LDS
    constexpr int NQT = NB * LS_MQ_NQ;     // query columns of the launch
    static_assert(L % GC == 0 && NU % P == 0 && NG * UPG == NU && (NG & (NG - 1)) == 0, "geometry");
    const int bid = (int)blockIdx.x - nfin;
    const int nblk = (int)gridDim.x - nfin;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 15, kq = lane >> 4;

    float* Bs = reinterpret_cast<float*>(smem_dyn);   // [NQT queries][DP]
    // [NQT queries][WPB waves][M] key lists, then the bounds. Two blocks: over the queries, once every wave is through
    // its tiles (131 KB of queries at d = 1024 leave no room beside them); one block: behind them (no barrier needed)
    u64* Ks = reinterpret_cast<u64*>(smem_dyn + (NB == 1 ? ((size_t)NQT * DP * 4 + 15) / 16 * 16 : 0));

    // Tiles of 16 rows are dealt round-robin to the waves of the launch (adjacent tiles go to different
    // workgroups): a run of adjacent, similar rows spreads over many workgroups.
    // Measured alternatives (tools/multiq_time.py, N = 200 k, 2 / 16 queries per pass, d = 384 | d = 1024):
    //   this form with 448 workgroups of 4 waves (1.75 per CU; 256 are ~10 % faster) 62.0 / 66.1 | 150.9 / 165.6 us
    //   256 workgroups of 8 waves, the tiles of a workgroup dealt to its waves
    //     by an LDS counter (every CU the same load, tools/mq_lifetimes.py)     63.1 / 69.1 | 149.4 / 172.3 us
    //   the same with (tile, 16-chain group) tasks of 12-16 KB, the group sums
    //     met in LDS by the last arriver (uniform work items for every d)       67.5 / 82.2 | 154.3 / 192.0 us
    //   (round 6) 8-wave workgroups with this static deal, one B block          62.2 | 149.7 us at 16 queries (55 | 139)
    // The eight-wave forms balance the CUs but pay a workgroup-wide barrier at the end (the slowest of 8
    // waves), a per-task LDS round trip, and the riding selection workgroups then displace whole scan
    // workgroups (one workgroup per CU leaves no second slot).
    if constexpr ((std::is_same<RowList, mq_union_src>::value || ...))  // (the union size: only the device knows it)
        n = (long long)*[](const mq_union_src& x) { return x.m; }(rowlist...);
    const long long W = (long long)nblk * WPB;
    const long long NT = (n + 15) / 16;
    // wave-major numbering: the launch's last, partial round of tiles (12 500 tiles over 1024 waves: 0.2 of
    // a round) goes to ONE wave in each of many workgroups instead of all four waves of a few - the tail is a
    // lone wave's tile (~2 us) in 212 CUs, not four waves' worth (~4 us) in 53
    long long t = (long long)wave * nblk + bid;

    // unit u of a tile -> first chunk: group-major, then the lane's V rounds, then 4-chunk steps
    auto unit_chunk = [](int u) constexpr -> int {
        const int grp = u / UPG, v = (u % UPG) / (GC / 4), j = u % (GC / 4);
        return L * v + GC * grp + 4 * j;
    };
    auto tile_ptr = [&](long long tile) -> const mq_f32x4* {
        // (LS_CORPUS_PAD_ROWS zero rows follow row n-1: the ragged last tile needs no clamping)
        const long long tc = tile < NT ? tile : NT - 1;  // a prefetch past the wave's last tile re-reads it
        return corpus + (tc * 16 + li) * CH + kq;
    };
    // the row-list form: this lane's list entry of a tile, and the lane's chunk pointer into that row
    constexpr bool IDX = sizeof...(RowList) == 1;
    constexpr bool UNI = (std::is_same<RowList, mq_union_src>::value || ...);  // the IVF union: a row list with ids and masks
    static_assert(sizeof...(RowList) <= 1 && (!IDX || NB == 1), "the row-list pass has one B block");
    [[maybe_unused]] auto list_at = [&](long long tile) -> u32 {
        if constexpr (UNI) {
            const mq_union_src& src = [](const mq_union_src& x) -> const mq_union_src& { return x; }(rowlist...);
            const long long p = tile * 16 + li;
            return src.row[p < n ? p : (n > 0 ? n - 1 : 0)];
        } else if constexpr (IDX) {
            const u32* __restrict__ list = [](const u32* l) { return l; }(rowlist...);
            const long long p = tile * 16 + li;
            return list[p < n ? p : n - 1];
        } else {
            return 0u;
        }
    };
    [[maybe_unused]] auto row_ptr = [&](u32 row) -> const mq_f32x4* { return corpus + (long long)row * CH + kq; };
    [[maybe_unused]] u32 le_cur = 0u, le_next = 0u;  // list entries of the wave's current and next tile
    if constexpr (IDX) {
        le_cur = list_at(t);
        le_next = list_at(t + W);
    }

    // ---- queries -> LDS, faiss.normalize_L2 fused (reference engine.py:242) exactly as in ls_scan_kernel:
    // canonical wave sum of squares (ls_wave_sumsq's order: lane l sums x[l], x[l+64], .. by fused
    // multiply-adds, then the xor tree 32..1), one correctly rounded 1/sqrt, one multiply per element. Wave w
    // stages queries w, w + WPB, ..: only the launch's REAL queries are loaded (unused columns are written as
    // zeros: what the LDS held before may be NaNs or denormals; a live query's row padding is zero too). All
    // loads of a wave are issued before the first is used (one memory round trip instead of one per query),
    // and in FRONT of the corpus loads - vector memory returns in order, and the queries (L2 hits for all but
    // the first workgroup) would otherwise arrive behind a cold HBM round trip.
    constexpr int EPL = CH * 4 / 64;       // elements per lane and query
    constexpr int QPW = NQT / WPB;         // queries per wave at most
    float xq[QPW][EPL];
#pragma unroll
    for (int j = 0; j < QPW; ++j) {
        const int qi = WPB * j + wave;
        if (qi < nq) {  // (wave-uniform)
            const float* src = qraw + (long long)qi * d;
#pragma unroll
            for (int i = 0; i < EPL; ++i) {
                const int e = lane + 64 * i;
                xq[j][i] = src[e < d ? e : d - 1];  // (unconditional loads; masked below)
            }
        } else {
#pragma unroll
            for (int i = 0; i < EPL; ++i) xq[j][i] = 0.0f;
        }
    }
    // (a launch without score vectors keeps its raw queries for the repair: workgroup b copies query b)
    if (qkeep)
        for (int qq = bid; qq < nq; qq += nblk)
            for (int e = threadIdx.x; e < d; e += 64 * WPB) qkeep[(long long)qq * d + e] = qraw[(long long)qq * d + e];
    __builtin_amdgcn_sched_barrier(0);
    mq_f32x4 ring[P];
    {
        const mq_f32x4* p0;
        if constexpr (IDX) p0 = row_ptr(le_cur);
        else p0 = tile_ptr(t);
#pragma unroll
        for (int u = 0; u < P; ++u) ring[u] = __builtin_nontemporal_load(p0 + unit_chunk(u));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < QPW; ++j) {
        const int qi = WPB * j + wave;
        if (qi >= nq) {  // (wave-uniform) an unused column
#pragma unroll
            for (int i = 0; i < EPL; ++i) Bs[qi * DP + lane + 64 * i] = 0.0f;
            continue;
        }
#pragma unroll
        for (int i = 0; i < EPL; ++i)
            if (lane + 64 * i >= d) xq[j][i] = 0.0f;
        float inv = 1.0f;
        if (normalize) {
            float ss = 0.0f;
#pragma unroll
            for (int i = 0; i < EPL; ++i) ss = fmaf(xq[j][i], xq[j][i], ss);  // (zeros past d add nothing)
            ss = ls_wave_xor_sum(ss);
            if (ss > 0.0f) inv = 1.0f / sqrtf(ss);
        }
#pragma unroll
        for (int i = 0; i < EPL; ++i) Bs[qi * DP + lane + 64 * i] = xq[j][i] * inv;
    }
    __syncthreads();

    LS_MQSTAMP(1);
    // this lane's best rows (queries li, 16 + li; rows 4kq.. of the wave's tiles), best first - as (score, row) pairs
    // while the tiles stream (round 6): a lane meets its rows in increasing order, so "key greater" is "score
    // greater" (an equal score loses to the earlier row) and NaN / <= -FLT_MAX scores never pass `s > -FLT_MAX`:
    // one 32-bit compare and four selects per list step, no key built per row. The 64-bit keys are made once, below.
    float bs[NB][M];
    u32 br[NB][M];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < M; ++i) {
            bs[b][i] = -FLT_MAX;
            br[b][i] = 0u;
        }

    while (t < NT) {
        const mq_f32x4* pcur;
        const mq_f32x4* pnext;
        [[maybe_unused]] u32 le_after = 0u;
        [[maybe_unused]] mq_u32x4 uid;   // the union pass: original rows and query masks of the lane's four positions
        [[maybe_unused]] mq_u16x4 umask;
        if constexpr (UNI) {
            const mq_union_src& src = [](const mq_union_src& x) -> const mq_union_src& { return x; }(rowlist...);
            uid = *reinterpret_cast<const mq_u32x4*>(src.id + t * 16 + 4 * kq);
            umask = *reinterpret_cast<const mq_u16x4*>(src.mask + t * 16 + 4 * kq);
        }
        if constexpr (IDX) {
            // (the entries of tile t + W came a tile ago: the refills below reach into that tile. Those of t + 2 W are
            // requested now, in front of this tile's refills, and first used a tile from here)
            pcur = row_ptr(le_cur);
            pnext = row_ptr(le_next);
            le_after = list_at(t + 2 * W);
        } else {
            pcur = tile_ptr(t);
            pnext = tile_ptr(t + W);
        }
        constexpr int LV = NG > 1 ? 31 - __builtin_clz(NG) : 1;  // levels of the tree above the groups
        [[maybe_unused]] mq_f32x4 pend[NB][LV];   // partial sums of the groups seen so far, one per tree level (a binary counter)
        mq_f32x4 acc[NB][GC];
        mq_f32x4 sc[NB];
        // (the B fragments do not change from tile to tile: left alone, the compiler hoists all CH reads
        // out of this loop - 96 to 256 registers, spilled. An opaque copy of the lane offset per tile keeps
        // them where they are: one ds_read_b32 in front of its MFMA. The opaque value is the OFFSET, not the
        // pointer: an opaque pointer loses its LDS address space, the reads become flat_load_dword, and a
        // pending flat load forces every wait to vmcnt(0).)
        // (one base per B block: block 1 lies 16 x DP x 4 bytes up - past the 64 KB a ds_read offset field reaches
        // for 4 KB rows, and a base + constant the compiler forms per read costs a v_add each)
        const float* bf[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            int boff = (b * LS_MQ_NQ + li) * DP + kq;
            asm volatile("" : "+v"(boff));
            bf[b] = Bs + boff;
        }
        // (an explicit count: a bare `#pragma unroll` is a request the unroller declines past 16 K instructions - the
        // 64 units x 8 MFMAs of 4 KB rows with two B blocks - and a rolled loop indexes ring / acc dynamically)
        // (two waves share a SIMD's matrix pipe in the two-block form: the one streaming its tile's MFMAs goes first, the
        // other's list inserts fill the issue slots behind them - 32 queries, d = 384: 66.3 -> 64.5 us; one block: no change)
        if (NB == 2) __builtin_amdgcn_s_setprio(1);
#pragma unroll NU
        for (int u = 0; u < NU; ++u) {
            const mq_f32x4 x = ring[u % P];
            // refill the slot: a later unit of this tile, or the head of the wave's next tile
            if (u + P < NU)
                ring[u % P] = __builtin_nontemporal_load(pcur + unit_chunk(u + P));
            else
                ring[u % P] = __builtin_nontemporal_load(pnext + unit_chunk(u + P - NU));
            // The tile body is one basic block; left alone, the scheduler sinks every refill down to its
            // first use to shorten live ranges (it chases a higher occupancy), the waits become vmcnt(0)
            // and each unit pays a full memory round trip (measured: 93 us per 16-query pass at N = 200 k
            // instead of ~65). Nothing moves across this point: the refill stays P units ahead of its use.
            __builtin_amdgcn_sched_barrier(0);
            float a[4];
            mq_transpose(x, a);
            const int cb = unit_chunk(u);
            const int v = (u % UPG) / (GC / 4), j = u % (GC / 4), grp = u / UPG;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const float bv = bf[b][4 * (cb + m)];
                    mq_f32x4 c;
                    if (v == 0) {
                        c[0] = 0.0f; c[1] = 0.0f; c[2] = 0.0f; c[3] = 0.0f;
                    } else {
                        c = acc[b][4 * j + m];
                    }
#ifdef LS_MQ_ABL_NOMFMA  // (ablation: everything but the matrix instruction - wrong results)
                    c[0] = fmaf(a[m], bv, c[0]);
                    acc[b][4 * j + m] = c;
#else
                    acc[b][4 * j + m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], bv, c, 0, 0, 0);
#endif
                }
            }
            // (the unit's B fragment reads go first: their LDS round trip then runs under the lane swaps. The
            // scheduler did that on its own for the [chunk][k][query] layout of round 5 and stopped doing it for
            // this one - every read sat right in front of its MFMA: 3.53 instead of 3.36 us per tile)
            __builtin_amdgcn_sched_group_barrier(0x100, 4 * NB, 0);  // LDS reads
            __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);       // 2 moves + 4 lane swaps
            __builtin_amdgcn_sched_group_barrier(0x008, 4 * NB, 0);  // the MFMAs
            if (u % UPG == UPG - 1) {  // the group's chains are complete: xor tree 1, 2, 4, 8 ...
#pragma unroll
                for (int b = 0; b < NB; ++b) {
#pragma unroll
                    for (int o = 1; o < GC; o <<= 1)
#pragma unroll
                        for (int i = 0; i < GC; i += 2 * o) acc[b][i] = acc[b][i] + acc[b][i + o];
                    // ... and the levels above the groups (16, 32): group g's sum meets the partial sums of the same
                    // size as they complete - the same balanced tree as adding all NG group sums at the end, with
                    // log2(NG) live registers instead of NG
                    mq_f32x4 vsum = acc[b][0];
                    // (pinned here: the second block's sums are first USED behind the first block's score-vector
                    // branch at the end of the tile, and LLVM's sink pass moves a whole add tree down to its use -
                    // every chain sum of the tile then waits in registers, 149-214 of them spilled)
                    asm volatile("" : "+v"(vsum));
                    bool parked = false;
#pragma unroll
                    for (int lv = 0; lv < LV; ++lv) {
                        if (parked || NG == 1) continue;
                        if ((grp >> lv) & 1) {
                            vsum = pend[b][lv] + vsum;
                        } else {
                            pend[b][lv] = vsum;
                            parked = true;
                        }
                    }
                    if (grp == NG - 1) sc[b] = vsum;  // rows t*16 + 4kq + 0..3 of query 16 b + li
                }
            }
        }
        if (NB == 2) __builtin_amdgcn_s_setprio(0);
#ifdef LS_SCAN_TIMING
        if (tiles_done == 0) LS_MQSTAMP(2);
#endif

        const long long row0 = t * 16 + 4 * kq;
#pragma unroll
        for (int b = 0; b < NB; ++b) {  // the score vectors, the lane's key lists (ls_mq_dev.h)
            if constexpr (UNI) mq_take_scores_union<M>(sc[b], li, uid, umask, row0, n, bs[b], br[b]);
            else mq_take_scores<M>(sc[b], LS_MQ_NQ * b + li, nq, S, s_stride, row0, t, n, bs[b], br[b]);
        }
        t += W;
        if constexpr (IDX) {
            le_cur = le_next;
            le_next = le_after;
        }
#ifdef LS_SCAN_TIMING
        if (tiles_done++ == 0) LS_MQSTAMP(3);
#endif
    }
    LS_MQSTAMP(4);

    // ---- 16 lanes hold keys of one query: 4 lane groups x WPB waves: merged in registers, then in LDS, and the
    // workgroup emits its best k' keys + bound (ls_mq_dev.h)
    if (NB == 2) __syncthreads();        // (the key lists overwrite the queries: every wave is through its tiles)
    mq_merge_lists<M, NB, WPB>(bs, br, Ks, nq, lane, wave);
    __syncthreads();
    LS_MQSTAMP(5);
    mq_rank_emit<M, NB, WPB>(Ks, nq, kprime, cand, c_stride, bound, b_stride, gran, g_stride, tag, bid, nblk);
#ifdef LS_SCAN_TIMING
    LS_MQSTAMP(6);
    if (bid == nblk / 2 && threadIdx.x == 0) {
        for (int i = 0; i < 6; ++i) cand[c_stride - 8 + i] = stamp[i + 1] - stamp[i];
        cand[c_stride - 2] = (u64)tiles_done;
    }
    if (threadIdx.x == 0 && nq <= 7 && S) {  // every workgroup's start / end tick: score vector 7 is unused
        unsigned long long* life = reinterpret_cast<unsigned long long*>(S + 7 * s_stride);
        life[2 * bid] = stamp[0];
        life[2 * bid + 1] = stamp[6];
    }
#endif
}
