/* The reference of tests/test_gate_fp32_gpu.py: the ordering contract of tutel_amd_gate_proj_f32w (include/tutel_amd.h) written
 * out -- one sequential fmaf chain per (token, expert) over a range of m, ascending, from 0.  Built by the test with
 * `gcc -O2 -ffp-contract=off -shared -fPIC`; fmaf is libm's correctly rounded one whatever the host's instruction set. */
#include <math.h>

/* x [T, M] (tokens already widened to float, which is exact), w [E, M], out [T, E] */
void gate_fp32_chain(const float *x, const float *w, int T, int M, int E, int m0, int m1, float *out) {
  for (int t = 0; t < T; ++t)
    for (int e = 0; e < E; ++e) {
      const float *xr = x + (long)t * M, *wr = w + (long)e * M;
      float acc = 0.f;
      for (int m = m0; m < m1; ++m) acc = fmaf(xr[m], wr[m], acc);
      out[(long)t * E + e] = acc;
    }
}
