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
// The kernel is expert_gemm_w8.hip's weight-streaming kernel with another weight format -- a sibling with its own tile function, so
// that the W8 kernels' code objects stay what they were.  What is the same: one 4-wave workgroup per (expert, 128 rows, 128 image
// channels), wave w owning 32 channels and all 128 rows; weights global -> VGPR -> convert -> MFMA A operand, never through LDS, a
// register ring of W4_DEPTH K-tiles in flight, every load unconditional through a buffer descriptor of exactly the run's size (the
// refills past the last K-tile fetch nothing and return zeros that are never used); token rows through the swizzled 128-byte-row LDS
// panel, two tiles ahead in registers, one barrier per K-tile; rows plain or gathered through the slot map (negative slot: the zero
// row); ragged tiles clamp their loads and mask their stores; the XCD-local work-item order.  What differs:
//   * ONE 16-byte load per lane per K-tile of 64 (1 KB contiguous per wave): dword q of it holds the lane's eight codes of operand q,
//     k = 64 t + 16 q + 8 (lane >> 5) + j -- the image of include/tutel_amd.h (tutel_amd/experts/w4.py::pack);
//   * one scale dword per lane per K-tile (128 B contiguous per 32 lanes): the scale bytes of the four 32-blocks of k-range
//     [128 (t >> 1), + 128); K-tile t uses bytes 2 (t & 1) (operands 0, 1) and 2 (t & 1) + 1 (operands 2, 3);
//   * operand q = four converts of dword q, byte_sel 0 .. 3;
//   * the epilogue has no scale.
//
// SwiGLU experts (tutel_amd_expert_gemm_w4_glu): D = round_T( float(round_T(act(gacc))) * uacc ); gate and up interleaved by 16 channels
// in one image (experts/w8.py::interleave_gate_up over codes and scale bytes), the gating product register against register.
#include "gemm_dev.h"  // Mma<T>, activate<ACT>

#define W4_BM 128
#define W4_BN 128
#define W4_BK 64
#define W4_THREADS 256
#define W4_DEPTH 4       // K-tiles of weights in flight per wave (even: the token registers alternate with it)
#define W4_STAGE (W4_BM * W4_BK * 2)

struct W4Args {
  const unsigned char *A; long long a_stride_e; int lda;     // elements
  const unsigned char *Wq; long long w_stride_e;             // bytes
  const unsigned char *Ws; long long s_stride_e;             // bytes
  const uint16_t *bias; long long bias_stride_e;             // elements
  uint16_t *D; long long d_stride_e; int ldd;                // elements
  int R, N, K, ntm, ntn;
  const int32_t *slot_map; int T; const unsigned char *zero_row;
};

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

// streamed loads through the channel group's descriptors (each byte is read once by one workgroup per row tile)
__device__ __forceinline__ u32x4 w4_wload(__amdgpu_buffer_rsrc_t rs, int voff) {
  return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 2));
}
__device__ __forceinline__ uint32_t w4_sload(__amdgpu_buffer_rsrc_t rs, int voff) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_raw_buffer_load_b32(rs, voff, 0, 0));
}

// One (expert, 128 rows, 128 image channels) work item; both kernels below are this function.  GLU: the image holds a SwiGLU expert's
// gate and up channels interleaved by 16, p.N = 2 H image channels, and only the epilogue differs.
template <typename T, int ACT, bool GLU>
__device__ __forceinline__ void w4_tile(const W4Args &p, unsigned char *smem, const int e, const int tn, const int m0, const int rend,
                                        const long long slot0) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, kg = lane >> 5;
  const int n0 = tn * W4_BN;
  const int nk = p.K / W4_BK;
  const int NT = p.N >> 5;
  const int T128 = (p.K + 127) >> 7;              // scale dwords per channel
  const int nmi = min(4, (rend - m0 + 31) >> 5);  // live 32-row groups of this tile

  // ---- token rows: thread `tid` moves chunk (tid & 7) of rows 32 i + (tid >> 3), i < 4, of every K-tile -------------------------------
  const unsigned char *rowp[4];
  int ldst[4];
  {
    int slot[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) slot[i] = 0;
    if (p.slot_map != nullptr) {  // the slots first, so that their loads are in flight together
#pragma unroll
      for (int i = 0; i < 4; ++i) slot[i] = p.slot_map[slot0 + min(m0 + 32 * i + (tid >> 3), rend - 1)];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 32 * i + (tid >> 3), c = tid & 7;
      const int gr = min(m0 + r, rend - 1);
      const unsigned char *row;
      if (p.slot_map != nullptr) row = slot[i] < 0 ? p.zero_row : p.A + (long long)(slot[i] % p.T) * p.lda * 2;
      else row = p.A + ((long long)e * p.a_stride_e + (long long)gr * p.lda) * 2;
      rowp[i] = row + c * 16;
      ldst[i] = r * 128 + ((c ^ ((r >> 1) & 7)) << 4);
    }
  }

  // ---- weights: the wave's 32-channel group, clamped to the last one (a clamped wave computes and stores nothing new) ---------------------
  const int nt = min((n0 >> 5) + wn, NT - 1);
  const bool wave_live = (n0 >> 5) + wn < NT;
  // The group's codes are one run of 16 K bytes (nk blocks of 1 KB) and its scales one run of 128 T128 bytes, each read through a
  // buffer descriptor of exactly that size: every load of the K loop is UNCONDITIONAL, and the refills past the last K-tile are out
  // of the descriptors' ranges -- they fetch nothing and return zeros that are never used.  The K-tile's offset is part of the VECTOR
  // offset: the hardware's range check covers the vector and the immediate offset, not the scalar one.
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char *>(p.Wq + (long long)e * p.w_stride_e + (long long)nt * nk * 1024), 0, nk * 1024, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_s = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char *>(p.Ws + (long long)e * p.s_stride_e + (long long)nt * T128 * 128), 0, T128 * 128, 0x00020000);
  const int wl = lane * 16, sl = l31 * 4;
  u32x4 wreg[W4_DEPTH];
  uint32_t sreg[W4_DEPTH];
#pragma unroll
  for (int d = 0; d < W4_DEPTH; ++d) {
    wreg[d] = w4_wload(rs_w, wl + d * 1024);
    sreg[d] = w4_sload(rs_s, sl + (d >> 1) * 128);
  }

  f32x16 acc[4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mi][r] = 0.f;

  // Token rows run TWO tiles ahead in registers (treg[j]: a tile of parity j), as in the W8 kernel: the memory counter retires loads
  // in order, so a token tile asked for one step ago would wait for every weight refill issued before it.  Tile 0 goes to LDS here,
  // tile 1 waits in treg[1]
  u32x4 treg[2][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) treg[0][i] = *reinterpret_cast<const u32x4 *>(rowp[i]);
#pragma unroll
  for (int i = 0; i < 4; ++i) treg[1][i] = *reinterpret_cast<const u32x4 *>(rowp[i] + (long long)min(1, nk - 1) * (W4_BK * 2));
#pragma unroll
  for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4 *>(smem + ldst[i]) = treg[0][i];
  __syncthreads();

  const int sw = (l31 >> 1) & 7;
  const int frag = l31 * 128;  // + mi * 32 rows

  // The K loop, once per count of live 32-row groups: straight-line matrix instructions, no branch around any of them (the dead
  // groups' accumulators stay zero and their stores are masked)
  auto kloop = [&](auto nmi_c) __attribute__((always_inline)) {
    constexpr int NMI = decltype(nmi_c)::value;
    for (int kt0 = 0; kt0 < nk; kt0 += W4_DEPTH) {
#pragma unroll
      for (int d = 0; d < W4_DEPTH; ++d) {
        const int kt = kt0 + d;
        if (kt >= nk) break;  // block-uniform
        // token tile kt + 2 (behind the last tile: that tile again -- it is stored into the free stage and never read)
        const long long tnext = (long long)min(kt + 2, nk - 1) * (W4_BK * 2);
#pragma unroll
        for (int i = 0; i < 4; ++i) treg[d & 1][i] = *reinterpret_cast<const u32x4 *>(rowp[i] + tnext);
        // the K-tile's four operands of 8 k: dword q holds k = 64 kt + 16 q + 8 kg .. + 7; kt & 1 == d & 1 (kt0 is a multiple of the
        // even ring depth): the tile's two 32-blocks are bytes 2 (d & 1) and 2 (d & 1) + 1 of its scale dword
        const float s0 = w4_scale(sreg[d], 2 * (d & 1)), s1 = w4_scale(sreg[d], 2 * (d & 1) + 1);
        u32x4 wa[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) wa[q] = w4_widen<T>(wreg[d][q], q < 2 ? s0 : s1);
        wreg[d] = w4_wload(rs_w, wl + (kt + W4_DEPTH) * 1024);
        sreg[d] = w4_sload(rs_s, sl + ((kt + W4_DEPTH) >> 1) * 128);
        // operand q multiplies token chunk 2 q + kg of every row; the fragments of operand q + 1 are asked for before the matrix
        // instructions of operand q (two sets of four in registers, not all sixteen)
        const unsigned char *st = smem + (kt & 1) * W4_STAGE + frag;
        u32x4 tb[2][4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) tb[0][mi] = *reinterpret_cast<const u32x4 *>(st + mi * (32 * 128) + ((kg ^ sw) << 4));
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (q < 3) {
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
              tb[(q + 1) & 1][mi] = *reinterpret_cast<const u32x4 *>(st + mi * (32 * 128) + (((2 * (q + 1) + kg) ^ sw) << 4));
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int mi = 0; mi < 4; ++mi)
            if (mi < NMI) acc[mi] = Mma<T>::run(wa[q], tb[q & 1][mi], acc[mi]);
          __builtin_amdgcn_sched_barrier(0);
        }
        {  // the other stage is free since the last barrier (behind the last tile nobody reads what is stored)
          unsigned char *nx = smem + ((kt + 1) & 1) * W4_STAGE;
#pragma unroll
          for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4 *>(nx + ldst[i]) = treg[(d + 1) & 1][i];
        }
        __syncthreads();
      }
    }
  };
  switch (nmi) {
    case 1: kloop(std::integral_constant<int, 1>{}); break;
    case 2: kloop(std::integral_constant<int, 2>{}); break;
    case 3: kloop(std::integral_constant<int, 3>{}); break;
    default: kloop(std::integral_constant<int, 4>{}); break;
  }

  // ---- epilogue: lane = row m0 + 32 mi + l31; register 4 rg + r of accumulator mi = channel 32 nt + 8 rg + 4 kg + r ---------------------
  if (!wave_live) return;
  if constexpr (GLU) {
    // Registers rg = 0, 1 are gate channels 16 nt + 8 rg + 4 kg + r of the expert, registers rg + 2 the up channels of the same
    // indices (the image's interleave).  g = act(gacc) rounded to T, D = round_T(float(g) * uacc); no bias
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int m = m0 + mi * 32 + l31;
      if (m >= rend) continue;
      uint16_t *drow = p.D + (long long)e * p.d_stride_e + (long long)m * p.ldd + nt * 16 + kg * 4;
#pragma unroll
      for (int rg = 0; rg < 2; ++rg) {
        uint16_t o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float a = activate<ACT>(acc[mi][rg * 4 + r]);
          asm("" : "+v"(a));  // the fp32 activation exists before it is rounded
          const T g = Elem<T>::from_f32(a);
          float v = __fmul_rn(Elem<T>::to_f32(g), acc[mi][(rg + 2) * 4 + r]);
          asm("" : "+v"(v));  // and so does the product
          const T tv = Elem<T>::from_f32(v);
          __builtin_memcpy(&o[r], &tv, 2);
        }
        uint2 ov;
        ov.x = (uint32_t)o[0] | ((uint32_t)o[1] << 16);
        ov.y = (uint32_t)o[2] | ((uint32_t)o[3] << 16);
        *reinterpret_cast<uint2 *>(drow + rg * 8) = ov;
      }
    }
    return;
  }
  // the bias of the lane's channels 32 nt + 8 rg + 4 kg .. + 3, all fetched before the first is used
  uint2 bi[4];
#pragma unroll
  for (int rg = 0; rg < 4; ++rg) {
    const int n = nt * 32 + rg * 8 + kg * 4;
    bi[rg] = p.bias != nullptr ? *reinterpret_cast<const uint2 *>(p.bias + (long long)e * p.bias_stride_e + n) : make_uint2(0u, 0u);
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int m = m0 + mi * 32 + l31;
    if (m >= rend) continue;
    uint16_t *drow = p.D + (long long)e * p.d_stride_e + (long long)m * p.ldd + nt * 32 + kg * 4;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const uint16_t b4[4] = {(uint16_t)(bi[rg].x & 0xffff), (uint16_t)(bi[rg].x >> 16), (uint16_t)(bi[rg].y & 0xffff), (uint16_t)(bi[rg].y >> 16)};
      uint16_t o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[mi][rg * 4 + r];
        if (p.bias != nullptr) {
          T tb;
          __builtin_memcpy(&tb, &b4[r], 2);
          v = __fadd_rn(v, Elem<T>::to_f32(tb));
        }
        v = activate<ACT>(v);
        asm("" : "+v"(v));  // the fp32 value exists before it is rounded (no fused multiply-and-round for fp16)
        const T tv = Elem<T>::from_f32(v);
        __builtin_memcpy(&o[r], &tv, 2);
      }
      uint2 ov;
      ov.x = (uint32_t)o[0] | ((uint32_t)o[1] << 16);
      ov.y = (uint32_t)o[2] | ((uint32_t)o[3] << 16);
      *reinterpret_cast<uint2 *>(drow + rg * 8) = ov;
    }
  }
}

// (expert, row tile tm of the bucket [E_loc, R, *], channel tile): the channel tiles of one (expert, row tile) are consecutive work
// items on ONE XCD, so that its L2 fetches the tile's token rows once
template <typename T, int ACT, bool GLU>
__device__ __forceinline__ void w4_padded(const W4Args &p, unsigned char *smem) {
  const int b = xcd_work_item((int)gridDim.x);
  const int tn = b % p.ntn, tm = (b / p.ntn) % p.ntm, e = b / (p.ntn * p.ntm);
  w4_tile<T, ACT, GLU>(p, smem, e, tn, tm * W4_BM, p.R, (long long)e * p.R);
}

template <typename T, int ACT>
__global__ __launch_bounds__(W4_THREADS, 2) void expert_gemm_w4_kernel(const W4Args p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * W4_STAGE];
  w4_padded<T, ACT, false>(p, smem);
}

// SwiGLU gate and up products in one launch: 128 image channels = 64 output channels x 128 rows per workgroup
template <typename T, int ACT>
__global__ __launch_bounds__(W4_THREADS, 2) void expert_gemm_w4_glu_kernel(const W4Args p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * W4_STAGE];
  w4_padded<T, ACT, true>(p, smem);
}

static bool w4_dtype_ok(int dtype) { return dtype == TUTEL_BF16 || dtype == TUTEL_F16; }
static bool w4_shape_ok(int N, int K) { return N >= 32 && N % 32 == 0 && K >= W4_BK && K % W4_BK == 0; }

extern "C" int tutel_amd_expert_gemm_w4_supported(int dtype, int N, int K) { return w4_dtype_ok(dtype) && w4_shape_ok(N, K) ? 1 : 0; }
// the gate / up image has 2 H channels: H a multiple of 16
extern "C" int tutel_amd_expert_gemm_w4_glu_supported(int dtype, int H, int K) {
  return w4_dtype_ok(dtype) && H >= 16 && H % 16 == 0 && w4_shape_ok(2 * H, K) ? 1 : 0;
}

// what differs between the two entry points on the host: the names in the messages, and the image's channels per output channel
struct W4Entry { const char *name, *bad_n, *small_image; int per_out; };
static const W4Entry W4_PLAIN = {"tutel_amd_expert_gemm_w4", "N must be a multiple of 32",
                                 "w_stride_e / s_stride_e is smaller than one expert's image (N * K / 2 code bytes, N * ceil(K / 128) * 4 scale bytes)", 1};
static const W4Entry W4_GLU = {"tutel_amd_expert_gemm_w4_glu", "H must be a multiple of 16",
                               "w_stride_e / s_stride_e is smaller than one expert's image (H * K code bytes, 2 * H * ceil(K / 128) * 4 scale bytes)", 2};

// (the activations last to first: the compiler instantiates the list's kernels from its end, and they keep their order in the code object)
template <typename T, bool GLU> static int w4_launch(const W4Entry &en, const W4Args &a, int act, unsigned grid, hipStream_t st) {
  return dispatch_act<TUTEL_ACT_SILU, TUTEL_ACT_GELU, TUTEL_ACT_RELU, TUTEL_ACT_NONE>(
      act,
      [&](auto ac) {
        if constexpr (GLU) hipLaunchKernelGGL((expert_gemm_w4_glu_kernel<T, decltype(ac)::value>), dim3(grid), dim3(W4_THREADS), 0, st, a);
        else hipLaunchKernelGGL((expert_gemm_w4_kernel<T, decltype(ac)::value>), dim3(grid), dim3(W4_THREADS), 0, st, a);
        TUTEL_CHECK_LAUNCH(en.name);
        return 0;
      },
      [&] { return tutel_notsup(en.name, "the activation must be none, relu, gelu or silu"); });
}

// Both entry points: N output channels per row of D, en.per_out * N image channels.  Every check stands in front of the first HIP call
template <bool GLU>
static int w4_run(const W4Entry &en, const void *A, int64_t a_stride_e, int64_t a_stride_w, int a_rows_per_w, int lda, const void *Wq,
                  int64_t w_stride_e, const void *Ws, int64_t s_stride_e, const void *bias, int64_t bias_stride_e, void *D,
                  int64_t d_stride_e, int64_t d_stride_w, int d_rows_per_w, int ldd, int E_loc, int R, int N, int K, int dtype, int act,
                  const int32_t *row_counts, const int32_t *slot_map, int T, const void *zero_row, tutel_stream_t stream) {
  TUTEL_REQUIRE(E_loc >= 0 && R >= 0 && N >= 1 && K >= 1, "%s: bad sizes E_loc=%d R=%d %s=%d K=%d", en.name, E_loc, R, GLU ? "H" : "N", N, K);
  if (!w4_dtype_ok(dtype)) return tutel_notsup(en.name, "the activations must be bf16 or fp16");
  if (K % W4_BK != 0) return tutel_notsup(en.name, "K must be a multiple of 64");
  if (N % (32 / en.per_out) != 0) return tutel_notsup(en.name, en.bad_n);
  if (act != TUTEL_ACT_NONE && act != TUTEL_ACT_RELU && act != TUTEL_ACT_GELU && act != TUTEL_ACT_SILU)
    return tutel_notsup(en.name, "the activation must be none, relu, gelu or silu");
  if (row_counts != nullptr) return tutel_notsup(en.name, "row_counts (megablocks) are not covered");
  if ((slot_map == nullptr && (a_rows_per_w < R || a_stride_w != 0)) || d_rows_per_w < R || d_stride_w != 0)
    return tutel_notsup(en.name, "the [W, E_loc, C, *] exchange layouts are not covered (rows_per_w >= R and stride_w == 0)");
  if (lda % 8 != 0 || ldd % 4 != 0 || a_stride_e % 8 != 0 || d_stride_e % 4 != 0 || bias_stride_e % 4 != 0 || w_stride_e % 16 != 0 ||
      s_stride_e % 4 != 0)
    return tutel_notsup(en.name, "rows of A must stay 16-byte aligned (lda, a_stride_e % 8), rows of D and bias 8-byte aligned (% 4), "
                                 "w_stride_e % 16, s_stride_e % 4");
  const long long NI = (long long)en.per_out * N;   // image channels
  const long long T128 = ((long long)K + 127) / 128;
  if (w_stride_e < NI * K / 2 || s_stride_e < NI * T128 * 4) return tutel_notsup(en.name, en.small_image);
  const long long ntm = (R + W4_BM - 1) / W4_BM, ntn = (NI + W4_BN - 1) / W4_BN;
  if ((long long)E_loc * R > 0x7fffffffLL || (long long)E_loc * ntm * ntn > 0x7fffffffLL || NI > 0x7fffffffLL ||
      (long long)K * 16 > 0x7fffffffLL)
    return tutel_notsup(en.name, "E_loc * R, the tile count and one channel group's run of 16 K bytes must stay below 2^31");
  if (E_loc == 0 || R == 0) return 0;
  TUTEL_REQUIRE(A && Wq && Ws && D, "%s: null pointer", en.name);
  TUTEL_REQUIRE(((uintptr_t)A % 16) == 0 && ((uintptr_t)Wq % 16) == 0 && ((uintptr_t)Ws % 4) == 0 && ((uintptr_t)D % 8) == 0 &&
                    ((uintptr_t)bias % 8) == 0,
                "%s: A and Wq must be 16-byte aligned, D and bias 8-byte aligned, Ws 4-byte aligned", en.name);
  if (slot_map != nullptr)
    TUTEL_REQUIRE(T >= 1 && zero_row != nullptr && ((uintptr_t)zero_row % 16) == 0,
                  "%s: a slot map needs T >= 1 and a 16-byte aligned zero row", en.name);

  W4Args a;
  a.A = (const unsigned char *)A; a.a_stride_e = a_stride_e; a.lda = lda;
  a.Wq = (const unsigned char *)Wq; a.w_stride_e = w_stride_e;
  a.Ws = (const unsigned char *)Ws; a.s_stride_e = s_stride_e;
  a.bias = (const uint16_t *)bias; a.bias_stride_e = bias_stride_e;
  a.D = (uint16_t *)D; a.d_stride_e = d_stride_e; a.ldd = ldd;
  a.R = R; a.N = (int)NI; a.K = K; a.ntm = (int)ntm; a.ntn = (int)ntn;
  a.slot_map = slot_map; a.T = T; a.zero_row = (const unsigned char *)zero_row;
  hipStream_t st = (hipStream_t)stream;
  StageScope stage(GLU || act != TUTEL_ACT_NONE ? TUTEL_STAGE_FC1 : TUTEL_STAGE_FC2, st);
  const unsigned grid = (unsigned)((long long)E_loc * ntm * ntn);
  return dtype == TUTEL_BF16 ? w4_launch<bf16_t, GLU>(en, a, act, grid, st) : w4_launch<f16_t, GLU>(en, a, act, grid, st);
}

extern "C" int tutel_amd_expert_gemm_w4(const void *A, int64_t a_stride_e, int64_t a_stride_w, int a_rows_per_w, int lda, const void *Wq,
                                        int64_t w_stride_e, const void *Ws, int64_t s_stride_e, const void *bias, int64_t bias_stride_e,
                                        void *D, int64_t d_stride_e, int64_t d_stride_w, int d_rows_per_w, int ldd, int E_loc, int R, int N,
                                        int K, int dtype, int act, const int32_t *row_counts, const int32_t *slot_map, int T,
                                        const void *zero_row, tutel_stream_t stream) {
  return w4_run<false>(W4_PLAIN, A, a_stride_e, a_stride_w, a_rows_per_w, lda, Wq, w_stride_e, Ws, s_stride_e, bias, bias_stride_e, D,
                       d_stride_e, d_stride_w, d_rows_per_w, ldd, E_loc, R, N, K, dtype, act, row_counts, slot_map, T, zero_row, stream);
}

// SwiGLU gate and up products of MXFP4 weights in one launch (the contract: include/tutel_amd.h).  No bias: these experts have none
extern "C" int tutel_amd_expert_gemm_w4_glu(const void *A, int64_t a_stride_e, int64_t a_stride_w, int a_rows_per_w, int lda,
                                            const void *Wq_gu, int64_t w_stride_e, const void *Ws_gu, int64_t s_stride_e, void *D,
                                            int64_t d_stride_e, int64_t d_stride_w, int d_rows_per_w, int ldd, int E_loc, int R, int H, int K,
                                            int dtype, int act, const int32_t *row_counts, const int32_t *slot_map, int T,
                                            const void *zero_row, tutel_stream_t stream) {
  return w4_run<true>(W4_GLU, A, a_stride_e, a_stride_w, a_rows_per_w, lda, Wq_gu, w_stride_e, Ws_gu, s_stride_e, nullptr, 0, D, d_stride_e,
                      d_stride_w, d_rows_per_w, ldd, E_loc, R, H, K, dtype, act, row_counts, slot_map, T, zero_row, stream);
}
