// expert_gemm_w8.hip -- W8A16: the grouped GEMM of bf16 / fp16 experts whose weights are stored as OCP e4m3fn bytes with one fp32
// scale per (expert, output channel).
//
//   D[e, r, n] = round_T( act( acc(e, r, n) * scale[e, n] + bias[e, n] ) )          acc = sum_k A[e, r, k] * dq(Wq[e, n, k]) in fp32
//
// dq widens an e4m3 code to A's dtype EXACTLY (every finite code is a bf16 and an fp16 value; 0x7F / 0xFF are NaN and propagate):
// v_cvt_scalef32_pk_{bf16,f16}_fp8 with scale 1.0, two elements per instruction.  The product then runs on the 16-bit matrix
// instruction v_mfma_f32_32x32x16_{bf16,f16} with ONE fp32 accumulator per output (no split-K, no atomics); the scale is ONE fp32
// multiply per output in the epilogue, then one fp32 add of the bias, the activation (gemm_dev.h::activate) and one rounding
// (the library builds with -ffp-contract=off; the multiply and the add are written as __fmul_rn / __fadd_rn).  The contract is
// written into include/tutel_amd.h.
//
// The kernels are gemm_wstream.h's weight-streaming tile (the design, the packed work-item order and the host path are written
// there); this file is the e4m3 format (W8Fmt), the kernels under their names and the C entry points.  The format:
//   * the image (include/tutel_amd.h, tutel_amd/experts/w8.py::pack) is blocked by (32 channels, 32 k, lane) so that ONE
//     global_load_dwordx4 per lane fetches 1 KB contiguous per wave -- the MFMA fragments of two K-steps of 16 for the lane's channel
//     -- and a wave walks its 32 channels' whole K extent as one contiguous run of K * 32 bytes; a K-tile of 64 is two such loads
//     (2 KB per wave);
//   * the K loop is ONE loop that tests each 32-row group against the live count at run time.
//
// SwiGLU experts (tutel_amd_expert_gemm_w8_glu): D = round_T( round_T(act(gacc * scale_gate)) * (uacc * scale_up) ), the gate and up
// products of one launch over the interleaved image (experts/w8.py::interleave_gate_up).
#include "gemm_wstream.h"

struct W8Args {
  const unsigned char *A; long long a_stride_e; int lda;     // elements
  const unsigned char *Wq; long long w_stride_e;             // bytes
  const float *scale;
  const uint16_t *bias; long long bias_stride_e;             // elements
  uint16_t *D; long long d_stride_e; int ldd;                // elements
  int R, N, K, ntm, ntn;
  const int32_t *slot_map; int T; const unsigned char *zero_row;
};

template <typename T> struct W8Cvt;
template <> struct W8Cvt<bf16_t> {  // bytes 0, 1 (hi: 2, 3) of `u` -> two bf16 in one word
  template <bool HI> __device__ static __forceinline__ uint32_t run(uint32_t u) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(u, 1.0f, HI));
  }
};
template <> struct W8Cvt<f16_t> {
  template <bool HI> __device__ static __forceinline__ uint32_t run(uint32_t u) {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(u, 1.0f, HI));
  }
};

// 8 codes (two words) -> the 8-element MFMA operand
template <typename T> __device__ __forceinline__ u32x4 w8_widen(uint32_t lo, uint32_t hi) {
  u32x4 r;
  r[0] = W8Cvt<T>::template run<false>(lo);
  r[1] = W8Cvt<T>::template run<true>(lo);
  r[2] = W8Cvt<T>::template run<false>(hi);
  r[3] = W8Cvt<T>::template run<true>(hi);
  return r;
}

// 16 weight bytes per lane through the channel group's descriptor, streamed (each byte is read once by one workgroup per row tile)
__device__ __forceinline__ u32x4 w8_wload(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
  return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 2));
}

struct W8Fmt {
  using Args = W8Args;

  // Two 16-byte loads per lane per K-tile, through ONE descriptor over the group's run of K * 32 bytes; the K-tile's offset goes in
  // the SCALAR offset
  template <typename T> struct Ring {
    __amdgpu_buffer_rsrc_t rs;
    int wl;
    u32x4 w[WS_DEPTH][2];
    __device__ __forceinline__ void open(const W8Args &p, int e, int nt, int lane) {
      const int KT32 = p.K >> 5;
      rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char *>(p.Wq + (long long)e * p.w_stride_e + (long long)nt * KT32 * 1024), 0,
                                             KT32 * 1024, 0x00020000);
      wl = lane * 16;
    }
    __device__ __forceinline__ void load(int d, int t) {
#pragma unroll
      for (int h = 0; h < 2; ++h) w[d][h] = w8_wload(rs, wl, t * 2048 + h * 1024);
    }
    // word pair s of load h holds k = 64 t + 32 h + 16 s + 8 kg .. + 7
    __device__ __forceinline__ void widen(int d, u32x4 (&wa)[4]) const {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int s = 0; s < 2; ++s) wa[2 * h + s] = w8_widen<T>(w[d][h][2 * s], w[d][h][2 * s + 1]);
    }
  };

  // one fp32 scale per channel: a 4-vector per register group, one __fmul_rn per output
  struct Scale {
    float4 s[4];
    __device__ __forceinline__ void fetch(const W8Args &p, int e, int n, int rg) {
      s[rg] = *reinterpret_cast<const float4 *>(p.scale + (long long)e * p.N + n);
    }
    __device__ __forceinline__ float apply(float acc, int rg, int r) const {
      const float s4[4] = {s[rg].x, s[rg].y, s[rg].z, s[rg].w};
      return __fmul_rn(acc, s4[r]);
    }
  };

  struct Weights {
    const void *Wq; int64_t w_stride_e; const float *scale;
    bool strides_ok() const { return w_stride_e % 16 == 0; }
    bool image_ok(long long NI, int K) const { return w_stride_e >= NI * K; }
    static bool run_ok(int) { return true; }
    bool present() const { return Wq && scale; }
    bool aligned() const { return ((uintptr_t)Wq % 16) == 0 && ((uintptr_t)scale % 16) == 0; }
    void fill(W8Args &a) const { a.Wq = (const unsigned char *)Wq; a.w_stride_e = w_stride_e; a.scale = scale; }
  };
  static constexpr WsText TEXT = {
      {"rows of A must stay 16-byte aligned (lda, a_stride_e % 8), rows of D and bias 8-byte aligned (% 4), w_stride_e % 16",
       "rows of A must stay 16-byte aligned (lda % 8), rows of D and bias 8-byte aligned (% 4), w_stride_e % 16"},
      {"E_loc * R and the tile count must stay below 2^31",
       "the work item count tiles_bound * 2 * ceil(channels / 128) must stay below 2^31"},
      "%s: A, Wq and scale must be 16-byte aligned, D and bias 8-byte aligned"};
  static bool packed_halves() { return true; }   // the only packed form
  template <typename T, int ACT, bool GLU>
  static void launch(const W8Args &a, const WsTables *pk, bool halves, unsigned grid, hipStream_t st);
};

template <typename T, int ACT>
__global__ __launch_bounds__(WS_THREADS, 2) void expert_gemm_w8_kernel(const W8Args p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * WS_STAGE];
  ws_padded<W8Fmt, T, ACT, false, false>(p, smem);
}

// SwiGLU gate and up products in one launch: 128 image channels = 64 output channels x 128 rows per workgroup
template <typename T, int ACT>
__global__ __launch_bounds__(WS_THREADS, 2) void expert_gemm_w8_glu_kernel(const W8Args p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * WS_STAGE];
  ws_padded<W8Fmt, T, ACT, true, false>(p, smem);
}

// the packed dropless layout, halves form (gemm_wstream.h: ws_packed); live_map: TUTEL_AMD_W8_PACKED_MAP below
struct W8Tables { const int32_t *off, *tiles, *ntiles; int tiles_bound, live_map; };

template <typename T, int ACT, bool GLU>
__global__ __launch_bounds__(WS_THREADS, 2) void expert_gemm_w8_packed_kernel(const W8Args p, const W8Tables t) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * WS_STAGE];
  ws_packed<W8Fmt, T, ACT, GLU, 4, false>(p, t.off, t.tiles, t.ntiles, t.tiles_bound, t.live_map, smem);
}

// TUTEL_AMD_W8_PACKED_MAP=bound: cut the XCD chunks of the packed kernels from the grid, not from the live tile count (A/B runs only)
static int w8_packed_live_map() {
  static const int v = [] {
    const char *s = getenv("TUTEL_AMD_W8_PACKED_MAP");
    return s != nullptr && strcmp(s, "bound") == 0 ? 0 : 1;
  }();
  return v;
}

template <typename T, int ACT, bool GLU>
void W8Fmt::launch(const W8Args &a, const WsTables *pk, bool, unsigned grid, hipStream_t st) {
  if (pk != nullptr) {
    const W8Tables t = {pk->offsets, pk->tiles, pk->ntiles, pk->tiles_bound, w8_packed_live_map()};
    hipLaunchKernelGGL((expert_gemm_w8_packed_kernel<T, ACT, GLU>), dim3(grid), dim3(WS_THREADS), 0, st, a, t);
  } else if constexpr (GLU) {
    hipLaunchKernelGGL((expert_gemm_w8_glu_kernel<T, ACT>), dim3(grid), dim3(WS_THREADS), 0, st, a);
  } else {
    hipLaunchKernelGGL((expert_gemm_w8_kernel<T, ACT>), dim3(grid), dim3(WS_THREADS), 0, st, a);
  }
}

extern "C" int tutel_amd_expert_gemm_w8_supported(int dtype, int N, int K) { return ws_supported(dtype, N, K); }
extern "C" int tutel_amd_expert_gemm_w8_glu_supported(int dtype, int H, int K) { return ws_glu_supported(dtype, H, K); }

#define W8_SMALL "w_stride_e is smaller than one expert's image (N * K bytes)"
#define W8_SMALL_GU "w_stride_e is smaller than one expert's image (2 * H * K bytes)"

extern "C" int tutel_amd_expert_gemm_w8(const void *A, int64_t a_stride_e, int64_t a_stride_w, int a_rows_per_w, int lda, const void *Wq,
                                        int64_t w_stride_e, const float *scale, const void *bias, int64_t bias_stride_e, void *D,
                                        int64_t d_stride_e, int64_t d_stride_w, int d_rows_per_w, int ldd, int E_loc, int R, int N, int K,
                                        int dtype, int act, const int32_t *row_counts, const int32_t *slot_map, int T,
                                        const void *zero_row, tutel_stream_t stream) {
  const WsBucket bk = {a_stride_e, a_stride_w, a_rows_per_w, d_stride_e, d_stride_w, d_rows_per_w, row_counts};
  return ws_run<W8Fmt, false>({"tutel_amd_expert_gemm_w8", W8_SMALL}, {Wq, w_stride_e, scale}, &bk, nullptr, A, lda, slot_map, T, zero_row,
                              bias, bias_stride_e, D, ldd, E_loc, R, N, K, dtype, act, stream);
}

// SwiGLU gate and up products of FP8 weights in one launch (the contract: include/tutel_amd.h).  No bias: these experts have none
extern "C" int tutel_amd_expert_gemm_w8_glu(const void *A, int64_t a_stride_e, int64_t a_stride_w, int a_rows_per_w, int lda,
                                            const void *Wq_gu, int64_t w_stride_e, const float *scale_gu, void *D, int64_t d_stride_e,
                                            int64_t d_stride_w, int d_rows_per_w, int ldd, int E_loc, int R, int H, int K, int dtype, int act,
                                            const int32_t *row_counts, const int32_t *slot_map, int T, const void *zero_row,
                                            tutel_stream_t stream) {
  const WsBucket bk = {a_stride_e, a_stride_w, a_rows_per_w, d_stride_e, d_stride_w, d_rows_per_w, row_counts};
  return ws_run<W8Fmt, true>({"tutel_amd_expert_gemm_w8_glu", W8_SMALL_GU}, {Wq_gu, w_stride_e, scale_gu}, &bk, nullptr, A, lda, slot_map, T,
                             zero_row, nullptr, 0, D, ldd, E_loc, R, H, K, dtype, act, stream);
}

// The two GEMMs above over the packed dropless layout (the contract: include/tutel_amd.h): the row ranges come from the device tables
extern "C" int tutel_amd_expert_gemm_w8_packed(const void *A, int lda, const int32_t *a_rows, int T, const void *zero_row, const void *Wq,
                                               int64_t w_stride_e, const float *scale, const void *bias, int64_t bias_stride_e, void *D,
                                               int ldd, int E, int rows_bound, int N, int K, int dtype, int act, const int32_t *offsets,
                                               const int32_t *tiles, const int32_t *ntiles, int tiles_bound, tutel_stream_t stream) {
  const WsTables pk = {offsets, tiles, ntiles, tiles_bound};
  return ws_run<W8Fmt, false>({"tutel_amd_expert_gemm_w8_packed", W8_SMALL}, {Wq, w_stride_e, scale}, nullptr, &pk, A, lda, a_rows, T,
                              zero_row, bias, bias_stride_e, D, ldd, E, rows_bound, N, K, dtype, act, stream);
}

extern "C" int tutel_amd_expert_gemm_w8_glu_packed(const void *A, int lda, const int32_t *a_rows, int T, const void *zero_row,
                                                   const void *Wq_gu, int64_t w_stride_e, const float *scale_gu, void *D, int ldd, int E,
                                                   int rows_bound, int H, int K, int dtype, int act, const int32_t *offsets,
                                                   const int32_t *tiles, const int32_t *ntiles, int tiles_bound, tutel_stream_t stream) {
  const WsTables pk = {offsets, tiles, ntiles, tiles_bound};
  return ws_run<W8Fmt, true>({"tutel_amd_expert_gemm_w8_glu_packed", W8_SMALL_GU}, {Wq_gu, w_stride_e, scale_gu}, nullptr, &pk, A, lda,
                             a_rows, T, zero_row, nullptr, 0, D, ldd, E, rows_bound, H, K, dtype, act, stream);
}
