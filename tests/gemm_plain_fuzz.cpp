/* The division-free index helpers of the PLAIN ring GEMM kernel (tutel_amd/csrc/gemm_plain.h) over arrays, for tests/test_gemm_plain_cpu.py:
 * `g++ -O2 -shared -fPIC -I tutel_amd/csrc`.  The header is plain C++; the reciprocals come from gemm_plain_rcp as the host's launcher
 * takes them.  The test computes the division forms itself (numpy, 64-bit) and compares. */
#include "gemm_plain.h"

extern "C" {
void plain_rot(long n, const int *pair, const int *e, const int *nk, const int *npair, int *out) {
  for (long i = 0; i < n; ++i)
    out[i] = gemm_plain_rot(pair[i], e[i], nk[i], npair[i], gemm_plain_rcp((uint32_t)npair[i]), gemm_plain_rcp((uint32_t)nk[i]));
}
void plain_rot_fits(long n, const int *npair, const int *E_loc, const int *nk, int *out) {
  for (long i = 0; i < n; ++i) out[i] = gemm_plain_rot_fits(npair[i], E_loc[i], nk[i]);
}
void plain_slot_token(long n, const int *q, const int *rows_mod, int *out) {
  for (long i = 0; i < n; ++i) out[i] = gemm_plain_slot_token(q[i], rows_mod[i], gemm_plain_rcp((uint32_t)rows_mod[i]));
}
void plain_row_off(long n, const int *m, const int *ld, int *out) {
  for (long i = 0; i < n; ++i) out[i] = gemm_plain_row_off(m[i], ld[i]);
}
void plain_div(long n, const uint32_t *x, const uint32_t *d, uint32_t *out) {
  for (long i = 0; i < n; ++i) out[i] = gemm_plain_div(x[i], d[i], gemm_plain_rcp(d[i]));
}
int plain_args_bytes(void) { return (int)sizeof(GemmPlainArgs); }
}
