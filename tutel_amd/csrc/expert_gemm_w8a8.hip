// expert_gemm_w8a8.hip -- W8A8: the grouped GEMM of bf16 / fp16 experts whose weights AND activations are OCP e4m3fn bytes -- one fp32
// scale per (expert, output channel) on the weights (the W8A16 image and scales, unchanged), one fp32 scale per row on the activations
// (quantize_a8.hip).
//
//   D[e, r, n] = round_T( act( (acc(e, r, n) * a_scale[row]) * scale[e, n] + bias[e, n] ) )     acc = sum_k Aq[row, k] * Wq[e, n, k] in fp32
//
// Both operands go into v_mfma_f32_32x32x16_fp8_fp8 as they are stored: no convert anywhere.  ONE fp32 accumulator per output, a chain
// of that instruction over K ascending in steps of 16 (no split-K, no atomics); the order of the 16 products inside one instruction is
// the hardware's.  The epilogue is two fp32 multiplies (__fmul_rn: the row's scale, then the channel's), one add of the bias, the
// activation and one rounding.  The contract is written into include/tutel_amd.h.
//
// The tile -- one (expert, 128 rows, 128 image channels) work item, 4 waves, wave w owns channels 32 w .. 32 w + 31 and all rows -- has
// the shape of gemm_wstream.h's (its work-item order, its register ring of weight K-tiles through buffer descriptors, its clamp-and-mask
// treatment of ragged rows and channels and its host path, ws_run, are reused); what differs is what the fp8 operands change:
//   * weights: the W8A16 image, one 16-byte load per lane = the A operands of two K-steps.  Word pair s of load h of K-tile t IS the
//     8-byte operand for k = 64 t + 32 h + 16 s + 8 kg .. + 7 (kg = lane >> 5): global -> VGPR -> MFMA, no convert, no LDS;
//   * token rows: fp8 in LDS, K-tiles of 64 -- the ring's granularity and the contract's K % 64, so there is no tail -- in two stages
//     of 128 rows x 64 bytes (8 KB each: half the 16-bit panel).  A row is eight 8-byte SLOTS; slot s = 2 q + kg is what lane (row,
//     kg) reads as the B operand of K-step q.  kg is fixed over a half-wave, so without a swizzle the 32 lanes of a ds_read_b64 would
//     hit the same two slot columns.  Slot s of row r is stored at slot s ^ f(r), f(r) = ((r >> 1) & 7) ^ ((r >> 4) & 1):
//       - 32 banks of 4 bytes (16 lanes per cycle): the 8-byte unit index modulo 16 is 8 (r & 1) + (s ^ f(r)); over 16 consecutive rows
//         bits 1 .. 3 of r run through all values while bit 4 is fixed, so f is a bijection and the 16 units are distinct;
//       - 64 banks (32 lanes per cycle): the unit index modulo 32 is 8 (r & 3) + (s ^ f(r)); for fixed r & 3 the bits (4, 2, 3) of r give
//         8 distinct f: the 32 units are distinct.  Conflict-free under either model.
//     f flips bit 0 of the slot, so the two halves of a 16-byte chunk swap places when f(r) is odd: the storing thread swaps them in
//     registers (four v_cndmask) and still stores ONE ds_write_b128 -- 8 consecutive lanes store two whole rows, every bank once;
//   * thread `tid` moves chunk tid & 3 of rows 64 i + (tid >> 2), i < 2, of every K-tile: two 16-byte global loads, issued two tiles
//     ahead (the in-order memory counter argument of gemm_wstream.h), stored behind the previous tile's matrix instructions, one
//     barrier per K-tile;
//   * the epilogue fetches the lane's four row scales (one per 32-row group; a gathered row reads a_scale[slot % T], a negative slot
//     1.0) with the channel scales and the bias, all in front of the first use.
//
// SwiGLU experts (tutel_amd_expert_gemm_w8a8_glu): D = round_T( round_T(act(gacc sa sg)) * (uacc sa su) ) over the interleaved gate / up
// image, register against register as in the W8A16 kernel.
#include "gemm_wstream.h"

#define A8_STAGE (WS_BM * WS_BK)   // one stage of the fp8 token panel: 128 rows x 64 bytes

struct A8Args {
  const unsigned char *A; long long a_stride_e; int lda;     // bytes
  const float *a_scale;
  const unsigned char *Wq; long long w_stride_e;             // bytes
  const float *scale;
  const uint16_t *bias; long long bias_stride_e;             // elements
  uint16_t *D; long long d_stride_e; int ldd;                // elements
  int R, N, K, ntm, ntn;
  const int32_t *slot_map; int T; const unsigned char *zero_row;
};

typedef __attribute__((ext_vector_type(2))) uint32_t a8_op;   // one 8-byte MFMA operand: eight consecutive-k codes

__device__ __forceinline__ f32x16 a8_mma(a8_op a, a8_op b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(__builtin_bit_cast(long, a), __builtin_bit_cast(long, b), c, 0, 0, 0);
}

// the panel's swizzle (file header)
__device__ __forceinline__ int a8_f(int r) { return ((r >> 1) & 7) ^ ((r >> 4) & 1); }

// One (expert, 128 rows, 128 image channels) work item: expert e, rows [m0, min(m0 + 128, rend)), channel tile tn; slot0: the slot of
// the bucket's row 0.  GLU: p.N = 2 H image channels, and only the epilogue differs
template <typename T, int ACT, bool GLU>
__device__ __forceinline__ void a8_tile(const A8Args &p, unsigned char *smem, const int e, const int tn, const int m0, const int rend,
                                        const long long slot0) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, kg = lane >> 5;
  const int n0 = tn * WS_BN;
  const int nk = p.K / WS_BK;
  const int NT = p.N >> 5;
  const int nmi = min(4, (rend - m0 + 31) >> 5);  // live 32-row groups of this tile

  // ---- token rows: thread `tid` moves chunk (tid & 3) of rows 64 i + (tid >> 2), i < 2, of every K-tile; rows past the window's end
  // read the last row again (their outputs are masked) ------------------------------------------------------------------------------------
  const unsigned char *rowp[2];
  const int tr = tid >> 2, tc = tid & 3;
  const int tf = a8_f(tr);                                           // (rows tr and 64 + tr share it)
  const int ldst = tr * WS_BK + ((2 * tc) ^ (tf & 6)) * 8;           // + i * 64 rows
  const bool tswap = (tf & 1) != 0;
  {
    int slot[2] = {0, 0};
    if (p.slot_map != nullptr) {  // the slots first, so that their loads are in flight together
#pragma unroll
      for (int i = 0; i < 2; ++i) slot[i] = p.slot_map[slot0 + min(m0 + 64 * i + tr, rend - 1)];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int gr = min(m0 + 64 * i + tr, rend - 1);
      const unsigned char *row;
      if (p.slot_map != nullptr) row = slot[i] < 0 ? p.zero_row : p.A + (long long)(slot[i] % p.T) * p.lda;
      else row = p.A + (long long)e * p.a_stride_e + (long long)gr * p.lda;
      rowp[i] = row + tc * 16;
    }
  }
  auto tstore = [&](unsigned char *stage, const u32x4 (&t)[2]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      u32x4 v = t[i];
      if (tswap) v = u32x4{t[i][2], t[i][3], t[i][0], t[i][1]};
      *reinterpret_cast<u32x4 *>(stage + i * (64 * WS_BK) + ldst) = v;
    }
  };

  // ---- weights: the wave's 32-channel group, clamped to the last one (a clamped wave computes and stores nothing new).  The group's
  // run of K * 32 bytes is read through a buffer descriptor of exactly its size: every load of the K loop is unconditional, the
  // refills past the last K-tile are out of range and return zeros that are never used ------------------------------------------------------
  const int nt = min((n0 >> 5) + wn, NT - 1);
  const bool wave_live = (n0 >> 5) + wn < NT;
  const int KT32 = p.K >> 5;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char *>(p.Wq + (long long)e * p.w_stride_e + (long long)nt * KT32 * 1024), 0, KT32 * 1024, 0x00020000);
  const int wl = lane * 16;
  u32x4 w[WS_DEPTH][2];
  auto wload = [&](int d, int t) __attribute__((always_inline)) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
      w[d][h] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, wl, t * 2048 + h * 1024, 2));
  };
#pragma unroll
  for (int d = 0; d < WS_DEPTH; ++d) wload(d, d);

  f32x16 acc[4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mi][r] = 0.f;

  // token tile 0 goes to LDS here, tile 1 waits in treg[1] (treg[j]: a tile of parity j)
  u32x4 treg[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i) treg[0][i] = *reinterpret_cast<const u32x4 *>(rowp[i]);
#pragma unroll
  for (int i = 0; i < 2; ++i) treg[1][i] = *reinterpret_cast<const u32x4 *>(rowp[i] + (long long)min(1, nk - 1) * WS_BK);
  tstore(smem, treg[0]);
  __syncthreads();

  const int lf = a8_f(l31);                      // (rows 32 mi + l31 share it)
  const unsigned char *frag = smem + l31 * WS_BK;   // + mi * 32 rows

  for (int kt0 = 0; kt0 < nk; kt0 += WS_DEPTH) {
#pragma unroll
    for (int d = 0; d < WS_DEPTH; ++d) {
      const int kt = kt0 + d;   // kt & 1 == d & 1: kt0 is a multiple of the even ring depth
      if (kt >= nk) break;  // block-uniform
      // token tile kt + 2 (behind the last tile: that tile again -- it is stored into the free stage and never read)
      const long long tnext = (long long)min(kt + 2, nk - 1) * WS_BK;
#pragma unroll
      for (int i = 0; i < 2; ++i) treg[d & 1][i] = *reinterpret_cast<const u32x4 *>(rowp[i] + tnext);
      // the K-tile's four operands: operand q = 2 h + s holds k = 64 kt + 16 q + 8 kg .. + 7; then the slot's refill
      a8_op wa[4];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int s = 0; s < 2; ++s) wa[2 * h + s] = a8_op{w[d][h][2 * s], w[d][h][2 * s + 1]};
      wload(d, kt + WS_DEPTH);
      // operand q multiplies slot 2 q + kg of every row; the fragments of operand q + 1 are asked for before the matrix instructions
      // of operand q
      const unsigned char *st = frag + (kt & 1) * A8_STAGE;
      a8_op tb[2][4];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) tb[0][mi] = *reinterpret_cast<const a8_op *>(st + mi * (32 * WS_BK) + ((kg ^ lf) << 3));
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q < 3) {
#pragma unroll
          for (int mi = 0; mi < 4; ++mi)
            tb[(q + 1) & 1][mi] = *reinterpret_cast<const a8_op *>(st + mi * (32 * WS_BK) + (((2 * (q + 1) + kg) ^ lf) << 3));
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
          if (mi < nmi) acc[mi] = a8_mma(wa[q], tb[q & 1][mi], acc[mi]);
        __builtin_amdgcn_sched_barrier(0);
      }
      // the other stage is free since the last barrier (behind the last tile nobody reads what is stored)
      tstore(smem + ((kt + 1) & 1) * A8_STAGE, treg[(d + 1) & 1]);
      __syncthreads();
    }
  }

  // ---- epilogue: lane = row m0 + 32 mi + l31; register 4 rg + r of accumulator mi = channel 32 nt + 8 rg + 4 kg + r ---------------------
  if (!wave_live) return;
  // the lane's row scales, channel scales and bias, all fetched before the first is used
  float sa[4];
  {
    int slot[4] = {0, 0, 0, 0};
    if (p.slot_map != nullptr) {
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) slot[mi] = p.slot_map[slot0 + min(m0 + mi * 32 + l31, rend - 1)];
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      if (p.slot_map != nullptr) sa[mi] = slot[mi] < 0 ? 1.0f : p.a_scale[slot[mi] % p.T];
      else sa[mi] = p.a_scale[(long long)e * p.R + min(m0 + mi * 32 + l31, rend - 1)];
    }
  }
  float4 sc[4];
  uint2 bi[4];
#pragma unroll
  for (int rg = 0; rg < 4; ++rg) {
    const int n = nt * 32 + rg * 8 + kg * 4;
    sc[rg] = *reinterpret_cast<const float4 *>(p.scale + (long long)e * p.N + n);
    if constexpr (!GLU)
      bi[rg] = p.bias != nullptr ? *reinterpret_cast<const uint2 *>(p.bias + (long long)e * p.bias_stride_e + n) : make_uint2(0u, 0u);
  }
  // acc * a_scale[row], then * scale[channel]: two separate fp32 multiplies
  auto scaled = [&](int mi, int rg, int r) __attribute__((always_inline)) {
    const float s4[4] = {sc[rg].x, sc[rg].y, sc[rg].z, sc[rg].w};
    return __fmul_rn(__fmul_rn(acc[mi][rg * 4 + r], sa[mi]), s4[r]);
  };
  if constexpr (GLU) {
    // registers rg = 0, 1 are gate channels 16 nt + 8 rg + 4 kg + r of the expert, registers rg + 2 the up channels of the same indices
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
          float a = activate<ACT>(scaled(mi, rg, r));
          asm("" : "+v"(a));  // the fp32 activation exists before it is rounded
          const T g = Elem<T>::from_f32(a);
          const float u = scaled(mi, rg + 2, r);
          float v = __fmul_rn(Elem<T>::to_f32(g), u);
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
        float v = scaled(mi, rg, r);
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

// (expert, row tile of the bucket [E_loc, R, *], channel tile) in ws_padded's order: the channel tiles of one (expert, row tile) are
// consecutive work items on ONE XCD, whose L2 then fetches the tile's token rows once
template <typename T, int ACT, bool GLU>
__global__ __launch_bounds__(WS_THREADS, 2) void expert_gemm_w8a8_kernel(const A8Args p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * A8_STAGE];
  const int b = xcd_work_item((int)gridDim.x);
  const int tn = b % p.ntn, tm = (b / p.ntn) % p.ntm, e = b / (p.ntn * p.ntm);
  a8_tile<T, ACT, GLU>(p, smem, e, tn, tm * WS_BM, p.R, (long long)e * p.R);
}

// ---- host: gemm_wstream.h's ws_run over this format's operands (its checks, its refusals, its grid) -----------------------------------
struct A8Fmt {
  using Args = A8Args;
  struct Weights {
    const void *Wq; int64_t w_stride_e; const float *scale;
    const float *a_scale; int lda; int64_t a_stride_e;   // the activations' own: byte strides of 16-byte aligned fp8 rows
    bool strides_ok() const { return w_stride_e % 16 == 0 && lda % 16 == 0 && a_stride_e % 16 == 0; }
    bool image_ok(long long NI, int K) const { return w_stride_e >= NI * K; }
    static bool run_ok(int) { return true; }
    bool present() const { return Wq && scale && a_scale; }
    bool aligned() const { return ((uintptr_t)Wq % 16) == 0 && ((uintptr_t)scale % 16) == 0 && ((uintptr_t)a_scale % 4) == 0; }
    void fill(A8Args &a) const { a.Wq = (const unsigned char *)Wq; a.w_stride_e = w_stride_e; a.scale = scale; a.a_scale = a_scale; }
  };
  static constexpr WsText TEXT = {
      {"rows of Aq must stay 16-byte aligned (lda, a_stride_e % 16), rows of D and bias 8-byte aligned (% 4), w_stride_e % 16", ""},
      {"E_loc * R and the tile count must stay below 2^31", ""},
      "%s: Aq, Wq and scale must be 16-byte aligned, D and bias 8-byte aligned, a_scale 4-byte aligned"};
  static bool packed_halves() { return false; }   // (no packed form)
  template <typename T, int ACT, bool GLU>
  static void launch(const A8Args &a, const WsTables *, bool, unsigned grid, hipStream_t st) {
    hipLaunchKernelGGL((expert_gemm_w8a8_kernel<T, ACT, GLU>), dim3(grid), dim3(WS_THREADS), 0, st, a);
  }
};

extern "C" int tutel_amd_expert_gemm_w8a8_supported(int dtype, int N, int K) { return ws_supported(dtype, N, K); }
extern "C" int tutel_amd_expert_gemm_w8a8_glu_supported(int dtype, int H, int K) { return ws_glu_supported(dtype, H, K); }

extern "C" int tutel_amd_expert_gemm_w8a8(const void *Aq, const float *a_scale, int64_t a_stride_e, int64_t a_stride_w, int a_rows_per_w,
                                          int lda, const void *Wq, int64_t w_stride_e, const float *scale, const void *bias,
                                          int64_t bias_stride_e, void *D, int64_t d_stride_e, int64_t d_stride_w, int d_rows_per_w, int ldd,
                                          int E_loc, int R, int N, int K, int dtype, int act, const int32_t *row_counts,
                                          const int32_t *slot_map, int T, const void *zero_row, tutel_stream_t stream) {
  const WsBucket bk = {a_stride_e, a_stride_w, a_rows_per_w, d_stride_e, d_stride_w, d_rows_per_w, row_counts};
  return ws_run<A8Fmt, false>({"tutel_amd_expert_gemm_w8a8", "w_stride_e is smaller than one expert's image (N * K bytes)"},
                              {Wq, w_stride_e, scale, a_scale, lda, a_stride_e}, &bk, nullptr, Aq, lda, slot_map, T, zero_row, bias,
                              bias_stride_e, D, ldd, E_loc, R, N, K, dtype, act, stream);
}

// SwiGLU gate and up products of FP8 weights over FP8 activations in one launch (the contract: include/tutel_amd.h).  No bias
extern "C" int tutel_amd_expert_gemm_w8a8_glu(const void *Aq, const float *a_scale, int64_t a_stride_e, int64_t a_stride_w,
                                              int a_rows_per_w, int lda, const void *Wq_gu, int64_t w_stride_e, const float *scale_gu,
                                              void *D, int64_t d_stride_e, int64_t d_stride_w, int d_rows_per_w, int ldd, int E_loc, int R,
                                              int H, int K, int dtype, int act, const int32_t *row_counts, const int32_t *slot_map, int T,
                                              const void *zero_row, tutel_stream_t stream) {
  const WsBucket bk = {a_stride_e, a_stride_w, a_rows_per_w, d_stride_e, d_stride_w, d_rows_per_w, row_counts};
  return ws_run<A8Fmt, true>({"tutel_amd_expert_gemm_w8a8_glu", "w_stride_e is smaller than one expert's image (2 * H * K bytes)"},
                             {Wq_gu, w_stride_e, scale_gu, a_scale, lda, a_stride_e}, &bk, nullptr, Aq, lda, slot_map, T, zero_row, nullptr,
                             0, D, ldd, E_loc, R, H, K, dtype, act, stream);
}
