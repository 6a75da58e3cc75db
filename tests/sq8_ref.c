/* sq8_ref.c - "score of a row" of the sq8 storage dtype (include/leansearch_sq8.h), restated in plain C.
 * Built by tests/test_sq8_cpu.py with gcc -O2 -ffp-contract=off. A stored row is `chunks` = L * V chunks of 16 int8
 * codes, zero padded; qp is the prepared query q' = (q * inv) * step, zero padded to chunks * 16 floats. */
#include <math.h>
#include <stdint.h>

void sq8_ref_scores(const int8_t* codes, int64_t n, int chunks, int L, int V, const float* qp, float* scores) {
    for (int64_t r = 0; r < n; ++r) {
        const int8_t* row = codes + r * (int64_t)chunks * 16;
        float part[64], next[64];
        for (int sub = 0; sub < L; ++sub) { /* lane `sub`: chunks sub, sub + L, .. - ONE fmaf chain in memory order */
            float acc = 0.0f;
            for (int v = 0; v < V; ++v) {
                const int c = sub + L * v;
                for (int j = 0; j < 16; ++j) acc = fmaf((float)row[c * 16 + j], qp[c * 16 + j], acc);
            }
            part[sub] = acc;
        }
        for (int b = 1; b < L; b <<= 1) { /* the balanced xor tree: lane ^ 1, ^ 2, ^ 4, .. */
            for (int i = 0; i < L; ++i) next[i] = part[i] + part[i ^ b];
            for (int i = 0; i < L; ++i) part[i] = next[i];
        }
        scores[r] = part[0];
    }
}
