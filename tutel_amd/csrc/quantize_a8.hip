// quantize_a8.hip -- the per-row FP8 (OCP e4m3fn) quantiser of the W8A8 grouped GEMMs (expert_gemm_w8a8.hip): 16-bit activation rows
// in, e4m3 codes and one fp32 scale per row out.  The contract -- per row, bit for bit experts/w8.py::quantize_e4m3(X.unsqueeze(0),
// True) on a CPU -- is in include/tutel_amd.h; the rounding is quantize_e4m3.h's, shared with the weight quantiser.
//
// One WAVE per row, four rows per workgroup, no LDS and no barrier:
//   load    the row is read ONCE, 16 bytes (8 elements) per lane per round, a wave covers 1 KB contiguous per round.  All rounds are
//           issued before the first is used and the row stays in registers (its raw 16-bit words: 4 VGPRs per round) between the
//           amax pass and the convert.  The kernel is compiled for 1, 4 and 16 rounds -- K <= 512, 2048, 8192 -- so a short row does
//           not carry the long row's registers; QA_MAX_K = 8192 is the bound (64 VGPRs of row), a longer K is refused with a reason.
//   amax    on the BIT PATTERN of |x| as an unsigned integer (quantize_w8.hip: orders the finite values as their magnitudes, puts
//           inf and every NaN on top), reduced over the wave with six xor shuffles: every lane ends with the row's maximum.
//   scale   amax / 448 by a correctly rounded division, an all-zero row 1.  A row that holds a non-finite value: scale = NaN and the
//           NaN code 0x7F in every position -- no status word, no host read: the launch is graph-capturable and the GEMM behind it
//           turns the row into NaN outputs.
//   codes   lane l of round j holds elements 512 j + 8 l .. + 7: eight codes, ONE 8-byte store, 512 bytes contiguous per wave.
// K is a multiple of 64: the last round is whole lanes (lane l is live when 512 j + 8 l < K).
// Byte model: 2 K bytes read and K + 4 bytes written per row.
//
// BOUNDED (tutel_amd_quantize_rows_a8_bounded): the same kernel body with the row count on the DEVICE.  The grid is sized by the host
// bound `rows`; a wave whose row is >= *rows_dev returns before its first load -- the rows of a packed [rows_bound, K] array past
// offsets[E] were never written and are not read as data.  One scalar load and one wave-uniform branch, no host read: capturable.
#include "quantize_e4m3.h"

#define QA_THREADS 256
#define QA_ROWS (QA_THREADS / WAVE)   // rows per workgroup
#define QA_MAX_K 8192

struct QaArgs {
  const unsigned char *X; int ldx;   // elements
  unsigned char *Xq; int ldq;        // bytes
  float *scale;
  int rows, K;
  const int32_t *rows_dev;           // BOUNDED: the live row count, read by every wave
};

template <typename T, int NR, bool BOUNDED>
__global__ __launch_bounds__(QA_THREADS) void quantize_rows_a8_kernel(const QaArgs p) {
  const int lane = (int)threadIdx.x & 63;
  const int row = (int)blockIdx.x * QA_ROWS + ((int)threadIdx.x >> 6);
  if (row >= p.rows) return;   // (wave-uniform; the kernel has no barrier)
  if constexpr (BOUNDED) {
    if (row >= *p.rows_dev) return;   // (wave-uniform as well)
  }
  const T *x = reinterpret_cast<const T *>(p.X) + (int64_t)row * p.ldx + lane * 8;

  vec16 v[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    v[j] = vec16{{0u, 0u, 0u, 0u}};
    if (j * 512 + lane * 8 < p.K) v[j] = *reinterpret_cast<const vec16 *>(x + j * 512);
  }
  uint32_t m = 0u;
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    float f[8];
    Vec<T>::unpack(v[j], f);
#pragma unroll
    for (int i = 0; i < 8; ++i) m = qw_umax(m, __float_as_uint(f[i]) & 0x7fffffffu);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = qw_umax(m, (uint32_t)__shfl_xor((int)m, o, 64));

  const bool finite = m < 0x7f800000u;
  const float s = !finite ? __uint_as_float(0x7fc00000u) : m == 0u ? 1.0f : __fdiv_rn(__uint_as_float(m), 448.0f);
  if (lane == 0) p.scale[row] = s;

  unsigned char *q = p.Xq + (int64_t)row * p.ldq + lane * 8;
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    if (j * 512 + lane * 8 < p.K) {
      float f[8];
      Vec<T>::unpack(v[j], f);
      uint2 o = make_uint2(0x7f7f7f7fu, 0x7f7f7f7fu);
      if (finite) {
        o.x = qw_code(f[0], s) | (qw_code(f[1], s) << 8) | (qw_code(f[2], s) << 16) | (qw_code(f[3], s) << 24);
        o.y = qw_code(f[4], s) | (qw_code(f[5], s) << 8) | (qw_code(f[6], s) << 16) | (qw_code(f[7], s) << 24);
      }
      *reinterpret_cast<uint2 *>(q + j * 512) = o;
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------

static const char *qa_shape_refusal(int dtype, int K) {
  if (dtype != TUTEL_BF16 && dtype != TUTEL_F16) return "the rows must be bf16 or fp16";
  if (K < 64 || K % 64 != 0) return "K must be a multiple of 64";
  if (K > QA_MAX_K) return "K must not exceed 8192 (a row is kept in registers)";
  return nullptr;
}

extern "C" int tutel_amd_quantize_rows_a8_supported(int dtype, int K) { return qa_shape_refusal(dtype, K) == nullptr ? 1 : 0; }

template <typename T, bool BOUNDED> static void qa_launch(const QaArgs &a, unsigned grid, hipStream_t st) {
  if (a.K <= 512) hipLaunchKernelGGL((quantize_rows_a8_kernel<T, 1, BOUNDED>), dim3(grid), dim3(QA_THREADS), 0, st, a);
  else if (a.K <= 2048) hipLaunchKernelGGL((quantize_rows_a8_kernel<T, 4, BOUNDED>), dim3(grid), dim3(QA_THREADS), 0, st, a);
  else hipLaunchKernelGGL((quantize_rows_a8_kernel<T, 16, BOUNDED>), dim3(grid), dim3(QA_THREADS), 0, st, a);
}

// Both entry points.  Every check stands in front of the first HIP call
template <bool BOUNDED>
static int qa_run(const char *name, const void *X, int dtype, int ldx, int rows, int K, void *Xq, int ldq, float *scale,
                  const int32_t *rows_dev, tutel_stream_t stream) {
  TUTEL_REQUIRE(rows >= 0 && K >= 1, "%s: bad sizes rows=%d K=%d", name, rows, K);
  const char *why = qa_shape_refusal(dtype, K);
  if (why != nullptr) return tutel_notsup(name, why);
  if (ldx < K || ldq < K) return tutel_notsup(name, "ldx and ldq must be at least K");
  if (ldx % 8 != 0 || ldq % 8 != 0) return tutel_notsup(name, "rows of X must stay 16-byte aligned (ldx % 8), rows of Xq 8-byte aligned (ldq % 8)");
  if (rows == 0) return 0;
  TUTEL_REQUIRE(X != nullptr && Xq != nullptr && scale != nullptr, "%s: null pointer", name);
  if (((uintptr_t)X % 16) != 0 || ((uintptr_t)Xq % 8) != 0) return tutel_notsup(name, "X must be 16-byte aligned, Xq 8-byte aligned");
  TUTEL_REQUIRE(((uintptr_t)scale % 4) == 0, "%s: scale must be 4-byte aligned", name);
  if (BOUNDED) TUTEL_REQUIRE(rows_dev != nullptr && ((uintptr_t)rows_dev % 4) == 0, "%s: rows_dev must be a 4-byte aligned pointer", name);

  QaArgs a;
  a.X = (const unsigned char *)X; a.ldx = ldx;
  a.Xq = (unsigned char *)Xq; a.ldq = ldq;
  a.scale = scale;
  a.rows = rows; a.K = K; a.rows_dev = rows_dev;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)((rows + QA_ROWS - 1) / QA_ROWS);
  if (dtype == TUTEL_BF16) qa_launch<bf16_t, BOUNDED>(a, grid, st);
  else qa_launch<f16_t, BOUNDED>(a, grid, st);
  TUTEL_CHECK_LAUNCH(name);
  return 0;
}

extern "C" int tutel_amd_quantize_rows_a8(const void *X, int dtype, int ldx, int rows, int K, void *Xq, int ldq, float *scale,
                                          tutel_stream_t stream) {
  return qa_run<false>("tutel_amd_quantize_rows_a8", X, dtype, ldx, rows, K, Xq, ldq, scale, nullptr, stream);
}

extern "C" int tutel_amd_quantize_rows_a8_bounded(const void *X, int dtype, int ldx, int rows, int K, void *Xq, int ldq, float *scale,
                                                  const int32_t *rows_dev, tutel_stream_t stream) {
  return qa_run<true>("tutel_amd_quantize_rows_a8_bounded", X, dtype, ldx, rows, K, Xq, ldq, scale, rows_dev, stream);
}
