/* The numeric contract of tutel_amd_expert_gemm_f32 (include/tutel_amd.h) written out, for the tests to replay on the CPU:
 *
 *     D[e, r, n] = act( chain(e, r, n) + bias[e, n] )
 *     chain(e, r, n) = fmaf(a[K-1], w[K-1], ... fmaf(a[1], w[1], fmaf(a[0], w[0], 0.f)))
 *
 * one accumulator per output, k ascending from 0, starting from 0.f; then ONE fp32 add of the bias (none without a bias) and the
 * activation in fp32 (act: 0 none, 1 relu -- the two whose bits no math library decides).
 * Build: gcc -O2 -ffp-contract=off -shared -fPIC expert_gemm_f32_ref.c -o expert_gemm_f32_ref.so -lm
 *
 *   a    [E, R, K]                          contiguous fp32
 *   w    [E, N, K] (w_kmajor != 0) or [E, K, N]
 *   bias [E, N] or NULL
 *   out  [E, R, N] */
#include <math.h>
#include <stddef.h>

void expert_gemm_f32_chain(const float *a, const float *w, const float *bias, int E, int R, int N, int K, int w_kmajor, int act,
                           float *out) {
  for (int e = 0; e < E; ++e)
    for (int r = 0; r < R; ++r) {
      const float *ar = a + ((size_t)e * R + r) * K;
      for (int n = 0; n < N; ++n) {
        const float *we = w + (size_t)e * N * K;
        float acc = 0.f;
        for (int k = 0; k < K; ++k) acc = fmaf(ar[k], w_kmajor ? we[(size_t)n * K + k] : we[(size_t)k * N + n], acc);
        if (bias != NULL) acc = acc + bias[(size_t)e * N + n];
        if (act == 1) acc = fmaxf(acc, 0.f);
        out[((size_t)e * R + r) * N + n] = acc;
      }
    }
}
