/* l2_ref.c - "distance of a query to a stored row" of the L2 metric (include/leansearch_l2.h), restated
 * in plain C. Built by tests/test_l2_cpu.py with gcc -O2 -ffp-contract=off. rows: the padded row matrix as stored,
 * n x (chunks * per) floats - the f32 values, or the fp16 values widened - with chunks = L * V chunks of `per` elements
 * (4 for f32, 8 for f16); q: the query as the kernel sees it (scaled; for f16 rounded to fp16 and widened), zero padded
 * to chunks * per floats. */
#include <math.h>
#include <stdint.h>

void l2_ref_dists(const float* rows, int64_t n, int chunks, int L, int V, int per, const float* q, float* dists) {
    for (int64_t r = 0; r < n; ++r) {
        const float* row = rows + r * (int64_t)chunks * per;
        float part[64], next[64];
        for (int sub = 0; sub < L; ++sub) { /* lane `sub`: chunks sub, sub + L, .. - ONE chain in memory order */
            float acc = 0.0f;
            for (int v = 0; v < V; ++v) {
                const int c = sub + L * v;
                for (int j = 0; j < per; ++j) {
                    const float t = row[c * per + j] - q[c * per + j]; /* one rounded subtraction */
                    acc = fmaf(t, t, acc);
                }
            }
            part[sub] = acc;
        }
        for (int b = 1; b < L; b <<= 1) { /* the balanced xor tree: lane ^ 1, ^ 2, ^ 4, .. */
            for (int i = 0; i < L; ++i) next[i] = part[i] + part[i ^ b];
            for (int i = 0; i < L; ++i) part[i] = next[i];
        }
        dists[r] = part[0];
    }
}
