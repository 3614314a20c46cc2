// gemm_plain.h -- the PLAIN form of the 128 x 256 ring tile (gemm_big_tile<.., PLAIN = true>, gemm_dev.h): its argument block and the
// three pieces of index arithmetic that replace the general kernel's divisions by run-time divisors.  Plain C++ (no HIP header), so a
// CPU test can compile it on its own and fuzz the helpers against the division forms (tests/test_gemm_plain_cpu.py).
//
// Why a second form: the general tile serves every layout the library has (rows split over source ranks, peer stores, a gating
// operand, per-expert row counts, three store policies), and pays for it at both ends of every workgroup -- a chain of dependent
// kernel-argument fetches and a dozen expansions of integer division before the first weight byte is requested, the bias round trip
// and a dozen more expansions after the last MFMA.  The headline launches use none of that.  The PLAIN tile is the same K loop on the
// same ring with the same rotation, swizzles, MFMA order and epilogue arithmetic (the same bits); only the address arithmetic around
// it is that of the one layout it admits (gemm_plain_admits, gemm_plan.hip).
#pragma once
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

// floor(x / d) for any 32-bit x and d >= 1 from rcp = gemm_plain_rcp(d): the high word of x * rcp is the quotient or one below it
// (2^32 = rcp * d + s with 1 <= s <= d, so x * rcp / 2^32 = x / d - x * s / (d * 2^32), an error below 1), one compare settles it
__host__ __device__ inline uint32_t gemm_plain_rcp(uint32_t d) { return 0xffffffffu / d; }
__host__ __device__ inline uint32_t gemm_plain_div(uint32_t x, uint32_t d, uint32_t rcp) {
  const uint32_t q = (uint32_t)(((uint64_t)x * rcp) >> 32);
  return q + (x - q * d >= d ? 1u : 0u);
}

// (1) element offset of row m in an operand whose rows all belong to one source rank (rows_per_w >= R): what
//     (m / rows_per_w) * stride_w + (m % rows_per_w) * ld comes to
__host__ __device__ inline int gemm_plain_row_off(int m, int ld) { return m * ld; }
// (2) first K-tile of the (pair, e) workgroup: ((pair + 3 e) * nk / npair) % nk, in 32 bits -- the host admits the launch only when
//     (npair + 3 E_loc) * nk < 2^31
__host__ __device__ inline int gemm_plain_rot(int pair, int e, int nk, int npair, uint32_t rcp_npair, uint32_t rcp_nk) {
  const uint32_t t = gemm_plain_div((uint32_t)(pair + 3 * e) * (uint32_t)nk, (uint32_t)npair, rcp_npair);
  return (int)(t - gemm_plain_div(t, (uint32_t)nk, rcp_nk) * (uint32_t)nk);
}
// (3) token row of slot-map entry q >= 0: q % rows_mod
__host__ __device__ inline int gemm_plain_slot_token(int q, int rows_mod, uint32_t rcp_rows_mod) {
  return (int)((uint32_t)q - gemm_plain_div((uint32_t)q, (uint32_t)rows_mod, rcp_rows_mod) * (uint32_t)rows_mod);
}
// the 32-bit bound of (2)
__host__ __device__ inline bool gemm_plain_rot_fits(int npair, int E_loc, int nk) {
  return ((long long)npair + 3LL * E_loc) * nk < (1LL << 31);
}

// Everything the PLAIN tile reads, 160 bytes: the kernel fetches it as ONE batch of five 8-dword scalar loads at entry (one wait) instead
// of field by field where each is first used.  First 64 bytes: what the weight issue (and the choice of prologue) needs.
struct GemmPlainArgs {
  const void *W; long long w_stride_e; int ldw, K;
  int N, ntn; uint32_t rcp_ntn, rcp_nk;                  // npair = ntn; the reciprocals of gemm_plain_div
  int R, E_loc;
  const int32_t *a_rows;                                 // optional row gather for A (fused fast_encode), as in GemmArgs
  const uint8_t *fl_idx8;                                // fused location (FL instantiation)
  // ---- 64
  const void *A; long long a_stride_e; int lda, a_span_bytes;
  const void *a_zero; int a_rows_mod; uint32_t rcp_rows_mod;
  int32_t *fl_loc; int fl_n, ldd;
  const void *bias; long long bias_stride_e;
  void *D; long long d_stride_e;
  int grid, sgather;                                     // grid: workgroups of the launch (the hidden argument would be one more fetch);
                                                         // sgather: slot-map entries through the scalar cache, as in GemmArgs
};
static_assert(sizeof(GemmPlainArgs) == 160, "GemmPlainArgs: five 32-byte scalar loads");
