// ls_mq_dev.h — what the small-batch kernels (ls_mq.hip: fp32 index, ls_mq16.hip: fp16 index, ls_mq8.hip: sq8 index) share: all leave
// a 16-row x 16-query score block in the C/D layout of the 16x16 MFMAs (lane (kq = lane / 16, li = lane % 16)
// holds rows 4kq..4kq+3 of query li), so everything behind the inner products is one piece of code: the per-lane
// key lists, the in-register merge of a wave's four lane groups, the workgroup's rank and emit.
#pragma once
#include "ls_select_dev.h"

typedef float mq_f32x4 __attribute__((ext_vector_type(4)));

// (LS_MQ_NQ, the query columns of one MFMA block, and mq_key_pitch, the u64 between two queries' key lists: ls_mq_plan.h)

// One score block of query column `qc` (rows row0..row0+3 of tile t) meets the lane's list and, where the launch
// keeps score vectors, S.
// The list: this lane's best rows, best first - as (score, row) pairs while the tiles stream (round 6): a lane
// meets its rows in increasing order, so "key greater" is "score greater" (an equal score loses to the earlier
// row) and NaN / <= -FLT_MAX scores never pass `s > -FLT_MAX`: one 32-bit compare and four selects per list step,
// no key built per row. The 64-bit keys are made once, in mq_merge_lists.
template <int M>
__device__ __forceinline__ void mq_take_scores(const mq_f32x4& sc, int qc, int nq, float* __restrict__ S,
                                               long long s_stride, long long row0, long long t, long long n,
                                               float (&bs)[M], u32 (&br)[M]) {
    const bool live_q = qc < nq;
    // the score vector (what the selection's rescue sweeps). S == nullptr: the caller repairs a query whose
    // workgroup keys cannot be proven complete by serving it again on the single-query path (ls_api.hip).
    // What these stores cost is paid in the memory system, per write request, once the corpus no longer
    // fits the Infinity Cache: fp32, N = 200 k, d = 1024: 136 us without them for any query count, 140 / 144 /
    // 155 / 167 us with 2 / 4 / 8 / 16 queries (200 k half-line writes at 16: TCC_EA0_WRREQ_64B,
    // tools/mq_pmc.sh); d = 384 (307 MB): 54 -> 57.5 us. Tried, same times: a fifth wave that only stores
    // (fed through LDS: the scanning waves' in-order vmcnt never sees a store), quad-coalesced stores,
    // adjacent tiles paired into whole 128-byte lines per query (docs/EXPERIMENTS.md, round 5).
    if (live_q && S) {
        float* sp = S + (long long)qc * s_stride + row0;
        if (row0 + 3 < n) {
            *reinterpret_cast<mq_f32x4*>(sp) = sc;  // s_stride is a multiple of 64 floats
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (row0 + r < n) sp[r] = sc[r];
        }
    }
    // (unused query columns keep lists of whatever their zero columns score: dropped when the keys are made)
    const bool ragged = t * 16 + 16 > n;  // (wave-uniform: only the launch's last tile holds rows >= n)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float xs = (ragged && row0 + r >= n) ? -FLT_MAX : sc[r];
        u32 xr = (u32)(row0 + r);
#pragma unroll
        for (int i = 0; i < M; ++i) {  // branch-free insert: the better row stays, the other moves on
            const bool gt = xs > bs[i];
            const float hs = gt ? xs : bs[i];
            const u32 hr = gt ? xr : br[i];
            xs = gt ? bs[i] : xs;
            xr = gt ? br[i] : xr;
            bs[i] = hs;
            br[i] = hr;
        }
    }
}

// The IVF-union source of ls_mq_kernel (ls_ivf_batch.hip): the rows of the lists a GROUP of queries probes, list after
// list, as three flat arrays per position - storage row, original row, and the 16-bit mask of the group's queries that
// probe the position's list - and the union size, which only the device knows. The arrays are filled up to the next
// multiple of 16 positions (mask 0), so a tile's four ids / masks per lane are one 16-byte / 8-byte load.
typedef u32 mq_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short mq_u16x4 __attribute__((ext_vector_type(4)));
struct mq_union_src {
    const u32* row;              // [m] storage row of every union position
    const u32* id;               // [m padded to 16] original row
    const unsigned short* mask;  // [m padded to 16] bit q: query q of the group probes this position's list
    const u32* m;                // the union size
};

// mq_take_scores for the IVF union: no score vector; a row enters query column qc's list only if bit qc of its mask is
// set (else it is -FLT_MAX, which never passes); the list's row half is the ORIGINAL row `id`. Union positions are
// list-major, so a lane does not meet its rows in increasing original-row order: the insert compares (score, then
// original row ascending) - the order of the 64-bit keys made in mq_merge_lists - instead of letting an equal score
// lose to the earlier position. (-0.0 == +0.0 here as in ls_ord; a NaN compares false everywhere and falls off the end.)
template <int M>
__device__ __forceinline__ void mq_take_scores_union(const mq_f32x4& sc, int qc, const mq_u32x4& id, const mq_u16x4& mask,
                                                     long long pos0, long long n, float (&bs)[M], u32 (&br)[M]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const bool probed = ((u32)mask[r] >> qc) & 1u;
        float xs = (probed && pos0 + r < n) ? sc[r] : -FLT_MAX;
        u32 xr = id[r];
#pragma unroll
        for (int i = 0; i < M; ++i) {  // branch-free insert: the better (score, row) stays, the other moves on
            // (bitwise on purpose: `||` / `&&` compile to two exec-mask branches per list step)
            const bool gt = (xs > bs[i]) | ((xs == bs[i]) & (xr < br[i]));
            const float hs = gt ? xs : bs[i];
            const u32 hr = gt ? xr : br[i];
            xs = gt ? bs[i] : xs;
            xr = gt ? br[i] : xr;
            bs[i] = hs;
            br[i] = hr;
        }
    }
}

// ---- 16 lanes hold keys of one query: 4 lane groups x WPB waves ------------------------------------
// In the wave first (registers, every query of the wave at once): the lane groups kq and kq ^ 1,
// then ^ 2 merge their sorted lists - C[i] = max(A[i], B[M-1-i]) is the top M of the union (a bitonic
// sequence, re-sorted by a small network), min(A[i], B[M-1-i]) are the keys that leave - and carry a
// bound: the best key dropped anywhere below (a lane's own drops lie under its last key).
// (lane ^ 16 / lane ^ 32 by v_permlane16_swap / v_permlane32_swap: no LDS crossbar round trips)
// Then across the waves through LDS: per query WPB lists of M keys + WPB bounds (Ks: [NB x 16 queries][mq_key_pitch(WPB M)]
// keys, then [NB x 16][WPB + 1] bounds). The caller puts a barrier in front where Ks overlays something the waves
// still read, and one behind before mq_rank_emit.
template <int M, int NB, int WPB>
__device__ __forceinline__ void mq_merge_lists(const float (&bs)[NB][M], const u32 (&br)[NB][M], u64* Ks, int nq,
                                               int lane, int wave) {
    const int li = lane & 15, kq = lane >> 4;
    auto xor_lanes32 = [&](u32 v, int mask) -> u32 {
        if (mask == 32) {
            const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
            return lane < 32 ? (u32)r[1] : (u32)r[0];
        }
        const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
        return (lane & 16) ? (u32)r[0] : (u32)r[1];
    };
    auto xor_lanes64 = [&](u64 v, int mask) -> u64 {
        return ((u64)xor_lanes32((u32)(v >> 32), mask) << 32) | xor_lanes32((u32)v, mask);
    };
    constexpr int NQT = NB * LS_MQ_NQ;
    constexpr int TK = WPB * M;          // keys per query (k' + 1 <= TK)
    // (a query's keys / bounds start TKP / WPB + 1 u64 apart - 2 (mod 32) dwords: the 16 lanes that write one key slot of
    // 16 queries at once fall on 32 different banks; with the plain pitch of 32 u64 at M = 8 they all shared one pair)
    constexpr int TKP = mq_key_pitch(TK);
    u64* Kb = Ks + NQT * TKP;            // [NQT queries][WPB waves] bounds
    u64 lst[NB][M];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const bool live_q = LS_MQ_NQ * b + li < nq;
#pragma unroll
        for (int i = 0; i < M; ++i) lst[b][i] = live_q ? ls_make_key(bs[b][i], br[b][i]) : 0ull;  // (-FLT_MAX -> 0: no row)
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        u64 bnd = lst[b][M - 1];
#pragma unroll
        for (int mask = 16; mask <= 32; mask <<= 1) {
            u64 other[M];
#pragma unroll
            for (int i = 0; i < M; ++i) other[i] = xor_lanes64(lst[b][i], mask);
            const u64 obnd = xor_lanes64(bnd, mask);
            bnd = bnd > obnd ? bnd : obnd;
#pragma unroll
            for (int i = 0; i < M; ++i) {
                const u64 a = lst[b][i], o = other[M - 1 - i];
                const u64 lo = a < o ? a : o;
                lst[b][i] = a < o ? o : a;
                bnd = bnd > lo ? bnd : lo;
            }
#pragma unroll
            for (int pass = 0; pass < M; ++pass)  // odd-even transposition sort, descending (M <= 8)
#pragma unroll
                for (int i = pass & 1; i + 1 < M; i += 2) {
                    const u64 a = lst[b][i], o = lst[b][i + 1];
                    lst[b][i] = a > o ? a : o;
                    lst[b][i + 1] = a > o ? o : a;
                }
        }
        // Across the waves through LDS: per query WPB lists of M keys + WPB bounds
        if (kq == 0) {
            const int qc = LS_MQ_NQ * b + li;
#pragma unroll
            for (int i = 0; i < M; ++i) Ks[qc * TKP + wave * M + i] = lst[b][i];
            Kb[qc * (WPB + 1) + wave] = bnd;
        }
    }
}

// thread (query = tid / TPQ, slot = tid % TPQ) ranks keys slot, slot + TPQ, .. of its query among the
// WPB M by counting; the best k' go out, the bound is the best key that does not, or the best of the
// waves' bounds: cand / bound, or tagged granules for the same-launch selection (ls_scan.hip).
template <int M, int NB, int WPB>
__device__ __forceinline__ void mq_rank_emit(const u64* Ks, int nq, int kprime, u64* __restrict__ cand,
                                             long long c_stride, u64* __restrict__ bound, long long b_stride,
                                             void* __restrict__ gran, long long g_stride, u32 tag, int bid, int nblk) {
    constexpr int NQT = NB * LS_MQ_NQ;
    constexpr int TK = WPB * M;
    constexpr int TKP = mq_key_pitch(TK);
    const u64* Kb = Ks + NQT * TKP;
    constexpr int TPQ = 64 * WPB / NQT;           // threads per query
    constexpr int SPT = (TK + TPQ - 1) / TPQ;     // keys per thread
    const int qi = threadIdx.x / TPQ, slot = threadIdx.x % TPQ;
    const u64* kk = Ks + qi * TKP;
    u64 mine[SPT];
    int rank[SPT];
#pragma unroll
    for (int c = 0; c < SPT; ++c) {
        mine[c] = slot + TPQ * c < TK ? kk[slot + TPQ * c] : 0ull;
        rank[c] = 0;
    }
#pragma unroll
    for (int i = 0; i < TK; ++i) {
        const u64 o = kk[i];
#pragma unroll
        for (int c = 0; c < SPT; ++c)
            rank[c] += (o > mine[c]) || (o == mine[c] && i < slot + TPQ * c);  // ties exist only among the zeros
    }
    u64 lb = Kb[qi * (WPB + 1)];
#pragma unroll
    for (int w = 1; w < WPB; ++w) lb = Kb[qi * (WPB + 1) + w] > lb ? Kb[qi * (WPB + 1) + w] : lb;
#pragma unroll
    for (int c = 0; c < SPT; ++c) {
        if (qi >= nq || slot + TPQ * c >= TK) continue;
        if (gran) {  // same-launch selection: tagged 16-byte granules, rank-major (ls_scan.hip)
            if (rank[c] <= kprime) {
                const u64 out = rank[c] == kprime ? (mine[c] > lb ? mine[c] : lb) : mine[c];
                __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
                    (char*)gran + (long long)qi * g_stride * 16, 0, nblk * (kprime + 1) * 16, LS_BUF_RSRC_FLAGS);
                __builtin_amdgcn_raw_buffer_store_b128(u32x4{(u32)out, (u32)(out >> 32), tag, 0u}, rsrc,
                                                       (rank[c] * nblk + bid) * 16, 0, LS_AUX_SC1);
            }
        } else {
            if (rank[c] < kprime) cand[qi * c_stride + (long long)bid * kprime + rank[c]] = mine[c];
            if (rank[c] == kprime) bound[qi * b_stride + bid] = mine[c] > lb ? mine[c] : lb;
        }
    }
}
