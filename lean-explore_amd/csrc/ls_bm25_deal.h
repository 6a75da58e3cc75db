// ls_bm25_deal.h — which row (document, or position of a document list) a thread of the BM25 score kernel
// owns at a step. Plain inline functions, usable from the kernel and from a host program (the host test
// enumerates every (workgroup, thread, step) and checks that each row of [0, n) is visited exactly once).
//
// Rows are dealt in granules of 4 (rows 4j .. 4j+3: a lane quad reads 16 contiguous bytes) so that ANY run
// of low rows spreads evenly over all B workgroups. With B a multiple of 8, WHICH workgroup gets granule j
// is XCD-aware: runs of 8 consecutive granules (32 rows = one 128-byte line of u32) go to ONE XCD (run r ->
// workgroups with blockIdx % 8 == r % 8) and are dealt to that XCD's workgroups (blockIdx = xcd + 8 m)
// round-robin in run order. Otherwise granule j goes to workgroup j mod B.
#ifndef LS_BM25_DEAL_H
#define LS_BM25_DEAL_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LS_DEAL_HD __host__ __device__ __forceinline__
#else
#define LS_DEAL_HD inline
#endif

struct ls_bm25_deal {
    long long n;      // rows
    long long Bx;     // workgroups that share this one's granule sequence
    long long xcd;    // blockIdx % 8
    long long m;      // this workgroup's number among those Bx
    long long steps;  // steps of 64 granules (256 rows) per workgroup
    bool xcd_aware;
};

// n rows over B workgroups of 256 threads, seen from workgroup `block`
LS_DEAL_HD ls_bm25_deal ls_bm25_deal_make(long long n, long long B, long long block) {
    ls_bm25_deal d;
    const long long NG = (n + 3) / 4;  // granules
    d.n = n;
    d.xcd_aware = (B & 7) == 0;        // (the host launches a multiple of 8 workgroups above 8)
    d.Bx = d.xcd_aware ? B >> 3 : B;
    d.xcd = block & 7;
    d.m = d.xcd_aware ? block >> 3 : block;
    // granules of one sequence: an XCD owns every 8th run of 8 granules
    const long long NGx = d.xcd_aware ? ((NG + 63) / 64) * 8 : NG;
    d.steps = (NGx + 64 * d.Bx - 1) / (64 * d.Bx);  // 64 granules per workgroup and step
    return d;
}

// the row thread `thread` (0..255) owns at step `step`; it exists iff ls_bm25_deal_valid
LS_DEAL_HD long long ls_bm25_deal_row(const ls_bm25_deal& d, long long step, int thread) {
    const long long l = d.m + d.Bx * (step * 64 + (thread >> 2));  // number in the sequence
    const long long j = d.xcd_aware ? ((l >> 3) * 8 + d.xcd) * 8 + (l & 7) : l;
    return 4 * j + (thread & 3);
}

LS_DEAL_HD bool ls_bm25_deal_valid(const ls_bm25_deal& d, long long step, long long row) {
    return step < d.steps && row < d.n;
}

#endif  // LS_BM25_DEAL_H
