/* bf16_ref.c - "score of a row" of the bf16 storage dtype (include/leansearch_bf16.h), restated in plain
 * C. Built by tests/test_bf16_cpu.py with gcc -O2 -ffp-contract=off. A stored row is `chunks` = L * V chunks of 8 bfloat16
 * bit patterns, zero padded; q_padded is the prepared f32 query (q * inv), zero padded to chunks * 8 floats. */
#include <math.h>
#include <stdint.h>
#include <string.h>

static float bf16_to_f32(uint16_t b) { /* bits << 16, exact */
    const uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

void bf16_ref_scores(const uint16_t* rows, int64_t n, int chunks, int L, int V, const float* q_padded, float* scores) {
    for (int64_t r = 0; r < n; ++r) {
        const uint16_t* row = rows + r * (int64_t)chunks * 8;
        float part[64], next[64];
        for (int sub = 0; sub < L; ++sub) { /* lane `sub`: chunks sub, sub + L, .. - ONE fmaf chain in memory order */
            float acc = 0.0f;
            for (int v = 0; v < V; ++v) {
                const int c = sub + L * v;
                for (int j = 0; j < 8; ++j) acc = fmaf(bf16_to_f32(row[c * 8 + j]), q_padded[c * 8 + j], acc);
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
