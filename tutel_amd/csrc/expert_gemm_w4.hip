// expert_gemm_w4.hip -- W4A16: the grouped GEMM of bf16 / fp16 experts whose weights are stored as OCP MXFP4: e2m1 codes, two per byte,
// with one e8m0 scale byte per 32 values along K.
//
//   D[e, r, n] = round_T( act( acc(e, r, n) + bias[e, n] ) )          acc = sum_k A[e, r, k] * w(e, n, k) in fp32
//   w(e, n, k) = val(code[e, n, k]) * 2^(s[e, n, k / 32] - 127)       val in +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}
//
// The widen is v_cvt_scalef32_pk_{bf16,f16}_fp4: two codes of one byte of a dword and an fp32 scale -> two 16-bit values.  The scale
// operand is the fp32 with bits s << 23, a power of two, and for the admitted scale bytes (include/tutel_amd.h) every product is a
// normal number of the dtype: the widened operand is EXACT, so there is no scale multiply in the epilogue and no second rounding.  The
// product runs on v_mfma_f32_32x32x16_{bf16,f16} with ONE fp32 accumulator per output (no split-K, no atomics); then one fp32 add of
// the bias, the activation (gemm_dev.h::activate) and one rounding.  The contract is written into include/tutel_amd.h.
//
// The kernels are gemm_wstream.h's weight-streaming tile, the one expert_gemm_w8.hip runs (the design, the packed work-item order and
// the host path are written there); this file is the MXFP4 format (W4Fmt), the kernels under their names and the C entry points.  It
// stays a translation unit of its own because its object is built without packed fp32 arithmetic (Makefile).  The format:
//   * ONE 16-byte load per lane per K-tile of 64 (1 KB contiguous per wave): dword q of it holds the lane's eight codes of operand q,
//     k = 64 t + 16 q + 8 (lane >> 5) + j -- the image of include/tutel_amd.h (tutel_amd/experts/w4.py::pack);
//   * one scale dword per lane per K-tile (128 B contiguous per 32 lanes): the scale bytes of the four 32-blocks of k-range
//     [128 (t >> 1), + 128); K-tile t uses bytes 2 (t & 1) (operands 0, 1) and 2 (t & 1) + 1 (operands 2, 3);
//   * operand q = four converts of dword q, byte_sel 0 .. 3;
//   * the epilogue has no scale;
//   * the K loop is specialised per count of live 32-row groups, and the packed layout has a second, WIDE form (MG = 8).
//
// SwiGLU experts (tutel_amd_expert_gemm_w4_glu): D = round_T( float(round_T(act(gacc))) * uacc ); gate and up interleaved by 16 channels
// in one image (experts/w8.py::interleave_gate_up over codes and scale bytes), the gating product register against register.
#include "w4_image.h"  // W4Args, W4Ring, W4Weights: shared with expert_gemm_w4a8.hip

template <typename T> struct W4Cvt;
template <> struct W4Cvt<bf16_t> {  // the two codes of byte SEL of `u`, times `scale` -> two bf16 in one word (low nibble first)
  template <int SEL> __device__ static __forceinline__ uint32_t run(uint32_t u, float scale) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(u, scale, SEL));
  }
};
template <> struct W4Cvt<f16_t> {
  template <int SEL> __device__ static __forceinline__ uint32_t run(uint32_t u, float scale) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(u, scale, SEL));
  }
};

// 8 codes (one dword) under one block scale -> the 8-element MFMA operand
template <typename T> __device__ __forceinline__ u32x4 w4_widen(uint32_t u, float scale) {
  u32x4 r;
  r[0] = W4Cvt<T>::template run<0>(u, scale);
  r[1] = W4Cvt<T>::template run<1>(u, scale);
  r[2] = W4Cvt<T>::template run<2>(u, scale);
  r[3] = W4Cvt<T>::template run<3>(u, scale);
  return r;
}

// byte i of the scale dword -> the fp32 with bits s << 23: 2^(s - 127) for 1 <= s <= 254
__device__ __forceinline__ float w4_scale(uint32_t sd, int i) {
  return __builtin_bit_cast(float, ((sd >> (8 * i)) & 0xffu) << 23);
}

// TUTEL_AMD_W4_PACKED_TILE below
#define W4_PACKED_DEFAULT_HALVES 1

struct W4Fmt {
  using Args = W4Args;

  // w4_image.h's ring, widened to the dtype
  template <typename T> struct Ring : W4Ring {
    // dword q holds k = 64 t + 16 q + 8 kg .. + 7; t & 1 == d & 1 (the ring depth is even): the tile's two 32-blocks are bytes
    // 2 (d & 1) and 2 (d & 1) + 1 of its scale dword
    __device__ __forceinline__ void widen(int d, u32x4 (&wa)[4]) const {
      const float s0 = w4_scale(s[d], 2 * (d & 1)), s1 = w4_scale(s[d], 2 * (d & 1) + 1);
#pragma unroll
      for (int q = 0; q < 4; ++q) wa[q] = w4_widen<T>(w[d][q], q < 2 ? s0 : s1);
    }
  };

  // the block scales went into the widen: nothing per channel
  struct Scale {
    __device__ __forceinline__ void fetch(const W4Args &, int, int, int) {}
    __device__ __forceinline__ float apply(float acc, int, int) const { return acc; }
  };

  using Weights = W4Weights;
  static constexpr WsText TEXT = {
      {"rows of A must stay 16-byte aligned (lda, a_stride_e % 8), rows of D and bias 8-byte aligned (% 4), w_stride_e % 16, s_stride_e % 4",
       "rows of A must stay 16-byte aligned (lda % 8), rows of D and bias 8-byte aligned (% 4), w_stride_e % 16, s_stride_e % 4"},
      {"E_loc * R, the tile count and one channel group's run of 16 K bytes must stay below 2^31",
       "the work item count tiles_bound * 2 * ceil(channels / 128) and one channel group's run of 16 K bytes must stay below 2^31"},
      "%s: A and Wq must be 16-byte aligned, D and bias 8-byte aligned, Ws 4-byte aligned"};
  // The form of the packed kernels, read at EVERY call: TUTEL_AMD_W4_PACKED_TILE=halves | wide; anything else is the default, which
  // tools/packed_w4_bench.py's A/B decided: HALVES -- the wide form measured slower at 64 x 128 rows (108.7 against 79.5 us)
  // AND at 64 x 160 rows (147.2 against 121.5 us); it stays selectable
  static bool packed_halves() {
    const char *s = getenv("TUTEL_AMD_W4_PACKED_TILE");
    if (s != nullptr && strcmp(s, "halves") == 0) return true;
    if (s != nullptr && strcmp(s, "wide") == 0) return false;
    return W4_PACKED_DEFAULT_HALVES != 0;
  }
  template <typename T, int ACT, bool GLU>
  static void launch(const W4Args &a, const WsTables *pk, bool halves, unsigned grid, hipStream_t st);
};

template <typename T, int ACT>
__global__ __launch_bounds__(WS_THREADS, 2) void expert_gemm_w4_kernel(const W4Args p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * WS_STAGE];
  ws_padded<W4Fmt, T, ACT, false, true>(p, smem);
}

// SwiGLU gate and up products in one launch: 128 image channels = 64 output channels x 128 rows per workgroup
template <typename T, int ACT>
__global__ __launch_bounds__(WS_THREADS, 2) void expert_gemm_w4_glu_kernel(const W4Args p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * WS_STAGE];
  ws_padded<W4Fmt, T, ACT, true, true>(p, smem);
}

// ---- the packed dropless layout, both forms of gemm_wstream.h's ws_packed, always cut from the live pairs --------------------------
// WIDE: this kernel is bound by its converts, not by the bytes, and a second half of 32 live rows would redo every one of
// them for a quarter of the matrix instructions.  Registers: eight accumulators are 128 of a lane's registers, and with the ring, the
// token tiles two ahead and the fragments the tile does not fit 256 without scratch, so the wide kernels take ONE workgroup per CU (512
// registers per lane, zero scratch: profiles/expert_gemm_w4_packed_kernel_resources.txt); the panel is 2 x 32 KB of LDS.
// HALVES (TUTEL_AMD_W4_PACKED_TILE=halves): the measurement's other arm and a second, independent computation of the same bits -- and,
// measured faster at both shapes, the default: one workgroup of four waves per CU does not hide the wide tile's converts and LDS traffic.
struct W4Tables { const int32_t *off, *tiles, *ntiles; int tiles_bound; };

template <typename T, int ACT, bool GLU>
__global__ __launch_bounds__(WS_THREADS, 1) void expert_gemm_w4_packed_kernel(const W4Args p, const W4Tables t) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * WS_STAGE];   // two stages of 256 rows
  ws_packed<W4Fmt, T, ACT, GLU, 8, true>(p, t.off, t.tiles, t.ntiles, t.tiles_bound, 1, smem);
}

template <typename T, int ACT, bool GLU>
__global__ __launch_bounds__(WS_THREADS, 2) void expert_gemm_w4_packed_halves_kernel(const W4Args p, const W4Tables t) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * WS_STAGE];
  ws_packed<W4Fmt, T, ACT, GLU, 4, true>(p, t.off, t.tiles, t.ntiles, t.tiles_bound, 1, smem);
}

template <typename T, int ACT, bool GLU>
void W4Fmt::launch(const W4Args &a, const WsTables *pk, bool halves, unsigned grid, hipStream_t st) {
  if (pk != nullptr) {
    const W4Tables t = {pk->offsets, pk->tiles, pk->ntiles, pk->tiles_bound};
    if (halves) hipLaunchKernelGGL((expert_gemm_w4_packed_halves_kernel<T, ACT, GLU>), dim3(grid), dim3(WS_THREADS), 0, st, a, t);
    else hipLaunchKernelGGL((expert_gemm_w4_packed_kernel<T, ACT, GLU>), dim3(grid), dim3(WS_THREADS), 0, st, a, t);
  } else if constexpr (GLU) {
    hipLaunchKernelGGL((expert_gemm_w4_glu_kernel<T, ACT>), dim3(grid), dim3(WS_THREADS), 0, st, a);
  } else {
    hipLaunchKernelGGL((expert_gemm_w4_kernel<T, ACT>), dim3(grid), dim3(WS_THREADS), 0, st, a);
  }
}

extern "C" int tutel_amd_expert_gemm_w4_supported(int dtype, int N, int K) { return ws_supported(dtype, N, K); }
extern "C" int tutel_amd_expert_gemm_w4_glu_supported(int dtype, int H, int K) { return ws_glu_supported(dtype, H, K); }

extern "C" int tutel_amd_expert_gemm_w4(const void *A, int64_t a_stride_e, int64_t a_stride_w, int a_rows_per_w, int lda, const void *Wq,
                                        int64_t w_stride_e, const void *Ws, int64_t s_stride_e, const void *bias, int64_t bias_stride_e,
                                        void *D, int64_t d_stride_e, int64_t d_stride_w, int d_rows_per_w, int ldd, int E_loc, int R, int N,
                                        int K, int dtype, int act, const int32_t *row_counts, const int32_t *slot_map, int T,
                                        const void *zero_row, tutel_stream_t stream) {
  const WsBucket bk = {a_stride_e, a_stride_w, a_rows_per_w, d_stride_e, d_stride_w, d_rows_per_w, row_counts};
  return ws_run<W4Fmt, false>({"tutel_amd_expert_gemm_w4", W4_SMALL}, {Wq, w_stride_e, Ws, s_stride_e}, &bk, nullptr, A, lda, slot_map, T,
                              zero_row, bias, bias_stride_e, D, ldd, E_loc, R, N, K, dtype, act, stream);
}

// SwiGLU gate and up products of MXFP4 weights in one launch (the contract: include/tutel_amd.h).  No bias: these experts have none
extern "C" int tutel_amd_expert_gemm_w4_glu(const void *A, int64_t a_stride_e, int64_t a_stride_w, int a_rows_per_w, int lda,
                                            const void *Wq_gu, int64_t w_stride_e, const void *Ws_gu, int64_t s_stride_e, void *D,
                                            int64_t d_stride_e, int64_t d_stride_w, int d_rows_per_w, int ldd, int E_loc, int R, int H, int K,
                                            int dtype, int act, const int32_t *row_counts, const int32_t *slot_map, int T,
                                            const void *zero_row, tutel_stream_t stream) {
  const WsBucket bk = {a_stride_e, a_stride_w, a_rows_per_w, d_stride_e, d_stride_w, d_rows_per_w, row_counts};
  return ws_run<W4Fmt, true>({"tutel_amd_expert_gemm_w4_glu", W4_SMALL_GU}, {Wq_gu, w_stride_e, Ws_gu, s_stride_e}, &bk, nullptr, A, lda,
                             slot_map, T, zero_row, nullptr, 0, D, ldd, E_loc, R, H, K, dtype, act, stream);
}

// The two GEMMs above over the packed dropless layout (the contract: include/tutel_amd.h): the row ranges come from the device tables
extern "C" int tutel_amd_expert_gemm_w4_packed(const void *A, int lda, const int32_t *a_rows, int T, const void *zero_row, const void *Wq,
                                               int64_t w_stride_e, const void *Ws, int64_t s_stride_e, const void *bias,
                                               int64_t bias_stride_e, void *D, int ldd, int E, int rows_bound, int N, int K, int dtype,
                                               int act, const int32_t *offsets, const int32_t *tiles, const int32_t *ntiles,
                                               int tiles_bound, tutel_stream_t stream) {
  const WsTables pk = {offsets, tiles, ntiles, tiles_bound};
  return ws_run<W4Fmt, false>({"tutel_amd_expert_gemm_w4_packed", W4_SMALL}, {Wq, w_stride_e, Ws, s_stride_e}, nullptr, &pk, A, lda, a_rows,
                              T, zero_row, bias, bias_stride_e, D, ldd, E, rows_bound, N, K, dtype, act, stream);
}

extern "C" int tutel_amd_expert_gemm_w4_glu_packed(const void *A, int lda, const int32_t *a_rows, int T, const void *zero_row,
                                                   const void *Wq_gu, int64_t w_stride_e, const void *Ws_gu, int64_t s_stride_e, void *D,
                                                   int ldd, int E, int rows_bound, int H, int K, int dtype, int act,
                                                   const int32_t *offsets, const int32_t *tiles, const int32_t *ntiles, int tiles_bound,
                                                   tutel_stream_t stream) {
  const WsTables pk = {offsets, tiles, ntiles, tiles_bound};
  return ws_run<W4Fmt, true>({"tutel_amd_expert_gemm_w4_glu_packed", W4_SMALL_GU}, {Wq_gu, w_stride_e, Ws_gu, s_stride_e}, nullptr, &pk, A,
                             lda, a_rows, T, zero_row, nullptr, 0, D, ldd, E, rows_bound, H, K, dtype, act, stream);
}
