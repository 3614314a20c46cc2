// expert_gemm_w4a8.hip -- W4A8: the grouped GEMM of bf16 / fp16 experts whose weights are OCP MXFP4 (the W4A16 image, unchanged: e2m1
// codes under one e8m0 scale byte per 32 values along K) and whose activations are OCP e4m3fn bytes with one fp32 scale per row
// (quantize_a8.hip), on the block-scaled matrix instruction v_mfma_scale_f32_32x32x64_f8f6f4 (A = fp4, B = fp8 e4m3).
//
//   D[e, r, n] = round_T( act( fmul(acc(e, r, n), a_scale[row]) + bias[e, n] ) )
//   acc = sum over K-tiles of 64, ascending, of the instruction's result over  e2m1(code[e, n, k]) * 2^(s[e, n, k / 32] - 127) * e4m3(Aq[row, k])
//
// Both operands enter the instruction as stored and the hardware applies the MX block scale: no convert, no scale multiply, ONE
// instruction per 32-row group per K-tile where W4A16 issues sixteen converts and sixteen 16-bit matrix instructions.  ONE fp32
// accumulator per output (no split-K, no atomics); the order of the 64 products inside one instruction is the hardware's.  The
// activations' block scale is the constant byte 127 (2^0).  The epilogue is one fp32 multiply (__fmul_rn: the row's scale), one add of
// the bias, the activation and one rounding; there is no channel scale.  The contract is written into include/tutel_amd.h.
//
// The tile -- one (expert, 128 rows, 128 image channels) work item, 4 waves, wave w owns channels 32 w .. 32 w + 31 and all rows -- is
// gemm_wstream.h's: its work-item order (xcd_work_item, the channel tiles of a row tile on one XCD), its clamp-and-mask treatment of
// ragged rows and channels and its host path (ws_run) are reused, and so is the W4A16 ring (w4_image.h: W4Ring -- four K-tiles of codes
// and scale dwords in flight per lane through descriptors of exactly the channel group's size, the K-tile's offset in the VECTOR offset so
// that the refills past the last K-tile are out of range and fetch nothing).  What the instruction changes:
//   * an MX block in one lane.  The image gives lane (ch, kg) dword q = codes k = 64 t + 16 q + 8 kg + j: a lane's 16 bytes straddle
//     both 32-blocks of the K-tile, but the instruction applies ONE scale byte to all 32 values of a lane: lanes 0 .. 31 must hold block
//     0 (k 0 .. 31 of the tile) and lanes 32 .. 63 block 1.  Two v_permlane32_swap per K-tile do it: swap(q0, q2) and swap(q1, q3)
//     exchange the upper half-wave of the first register with the lower half-wave of the second, after which the registers
//     (q0', q2', q1', q3') hold k = 32 kg + {0 .. 7, 8 .. 15, 16 .. 23, 24 .. 31}: ASCENDING k.  The image, a stored format, is
//     untouched;
//   * the fp8 operand's K order is NOT the fp4 operand's (established on the hardware by tests/test_expert_gemm_w4a8_gpu.py's first
//     test): a lane's 128-bit register quad is one unit of K -- 32 fp4 values, but 16 fp8 values -- and the units interleave over the
//     half-waves, so the fp8 lane (row, kg) holds k = 16 kg .. 16 kg + 15 in registers 0 .. 3 and k = 32 + 16 kg .. + 15 in registers
//     4 .. 7 against the fp4 lane's k = 32 kg .. 32 kg + 31.  The scale byte goes with the fp4 lane: one MX block;
//   * the scale byte.  The lane's scale dword covers 128 k; K-tile t needs byte 2 (t & 1) + kg.  One v_lshrrev per K-tile by the lane
//     constant 8 kg + 16 (t & 1) (two registers, t & 1 is the unrolled ring slot's parity) brings it to byte 0, which the instruction
//     reads with op_sel 0: the same one VALU instruction per K-tile that a shift by 8 kg in front of an op_sel of 0 / 2 costs, without
//     depending on the instruction's byte select (Composable Kernel's sources note that it read byte 0 whatever op_sel said).  The bytes
//     above byte 0 are not read.  The activations' scale, 127, sits in a register for the same reason: a constant operand would be
//     encoded as an fp32 inline constant;
//   * token rows: fp8 in LDS, K-tiles of 64 in two stages of 128 rows x 64 bytes (8 KB each), fetched two tiles ahead in registers (the
//     in-order memory counter argument of gemm_wstream.h), stored behind the previous tile's matrix instructions, one barrier per
//     K-tile.  A row is four 16-byte CHUNKS; lane (row, kg) reads chunks kg and kg + 2 with two ds_read_b128 per 32-row group per
//     K-tile (W8A8: four ds_read_b64).  kg is fixed over a half-wave, so unswizzled the 32 lanes of a read would hit one chunk column.
//     Chunk c of row r is stored at chunk c ^ f(r), f(r) = ((r >> 1) & 3) ^ ((r >> 3) & 1):
//       - 32 banks of 4 bytes (8 lanes of 16 bytes per cycle): the 16-byte unit index modulo 8 is 4 (r & 1) + (c ^ f(r)); over 8
//         consecutive rows bits 1 .. 2 of r run through all values while bit 3 is fixed: f is a bijection and the 8 units are distinct;
//       - 64 banks (16 lanes per cycle): the unit index modulo 16 is 4 (r & 3) + (c ^ f(r)); for fixed r & 3, bit 1 is fixed and bits
//         (2, 3) of r give f = (2 b2 + b1) ^ b3: four distinct values, the 16 units are distinct.  Conflict-free under either model.
//     The storing thread moves whole chunks (chunk tid & 3 of rows tid >> 2 and 64 + (tid >> 2)): one ds_write_b128 each, 8 consecutive
//     lanes store two whole rows, every bank once;
//   * the K loop is compiled once per count of live 32-row groups (straight-line matrix instructions, no branch around any of them, no
//     accumulator copies), as the W4A16 tile's, and chosen by a switch;
//   * the epilogue fetches the lane's four row scales (one per 32-row group; a gathered row reads a_scale[slot % T], a negative slot
//     1.0) with the bias, all in front of the first use.
// Built with the default flags: the only fp32 arithmetic is the epilogue's __fmul_rn / __fadd_rn, whose packed forms round each element
// alike (expert_gemm_w8a8.hip is built the same way).
//
// The packed dropless layout (tutel_amd_expert_gemm_w4a8_packed / _glu_packed): the same tile over row windows read from the device
// tables, as two 128-row halves or as one WIDE 256-row window per table tile (w4a8_tile's MG; the kernels stand behind the padded one).
//
// SwiGLU experts (tutel_amd_expert_gemm_w4a8_glu): D = round_T( float(round_T(act(gacc sa))) * (uacc sa) ) over the 16-channel-interleaved
// gate / up image, register against register as in the other GLU kernels.
#include "w4_image.h"

#define A8_STAGE (WS_BM * WS_BK)   // one stage of the 128-row fp8 token panel: 128 rows x 64 bytes (the wide window's: two of them)

struct W4A8Args : W4Args {   // A: e4m3 bytes, a_stride_e and lda in bytes
  const float *a_scale;
};

typedef __attribute__((ext_vector_type(8))) int i32x8;

// A: 32 e2m1 codes (registers 4 .. 7 are not read), B: 32 e4m3 bytes, one e8m0 scale byte each in byte 0 of sa / sb
__device__ __forceinline__ f32x16 w4a8_mma(i32x8 a, i32x8 b, f32x16 c, uint32_t sa, uint32_t sb) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 4 /* A: fp4 */, 0 /* B: e4m3 */, 0, (int)sa, 0, (int)sb);
#else
  return c;
#endif
}

// x's lanes 32 .. 63 <-> y's lanes 0 .. 31
__device__ __forceinline__ void w4a8_swap(uint32_t &x, uint32_t &y) {
#if defined(__HIP_DEVICE_COMPILE__)
  const auto r = __builtin_amdgcn_permlane32_swap(x, y, false, false);
  x = r[0];
  y = r[1];
#endif
}

// the panel's swizzle (file header)
__device__ __forceinline__ int w4a8_f(int r) { return ((r >> 1) & 3) ^ ((r >> 3) & 1); }

// One (expert, 32 MG rows, 128 image channels) work item: expert e, rows [m0, min(m0 + 32 MG, rend)), channel tile tn; slot0: the slot
// -- and the index of the row scale -- of the layout's row 0 (e * R in the bucket, 0 on the packed layout, whose rows are absolute).
// GLU: p.N = 2 H image channels, and only the epilogue differs.
//   MG = 4: the 128-row tile of the padded kernels and of the packed kernels' halves form.
//   MG = 8: the WIDE window of the packed layout, a whole 256-row table tile.  A ring slot is fetched and prepared (two swaps, one
//           shift) ONCE per K-tile and feeds up to eight matrix instructions.  The panel is two stages of 256 rows x 64 bytes (32 KB);
//           thread `tid` moves chunk tid & 3 of rows 64 i + (tid >> 2), i < 4 (rows 64 apart share f: the swizzle is unchanged).  Live-
//           group counts 1 .. 4 move two token passes as the 128-row tile does (rows 128 .. 255 of the panel are neither written nor
//           read).  Counts above four ask for the fragments two groups at a time -- 16 registers, not 64: with 128
//           accumulators the tile then fits 256 registers and two workgroups per CU -- in front of their two matrix instructions;
//           a batch's reads are issued behind the previous batch's instructions and land under them.
// Whatever MG and the count: one fp32 accumulator per output, K-tiles ascending, the same operand, the same epilogue -- the same bits.
template <typename T, int ACT, bool GLU, int MG>
__device__ __forceinline__ void w4a8_tile(const W4A8Args &p, unsigned char *smem, const int e, const int tn, const int m0, const int rend,
                                          const long long slot0) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, kg = lane >> 5;
  const int n0 = tn * WS_BN;
  const int nk = p.K / WS_BK;
  const int NT = p.N >> 5;
  constexpr int NP = MG / 2;                      // token passes of 64 rows
  constexpr int STAGE = MG * 32 * WS_BK;          // one stage of the token panel
  const int nmi = min(MG, (rend - m0 + 31) >> 5); // live 32-row groups of this tile
  const bool wide = MG > 4 && nmi > 4;            // (block-uniform) the token passes 2 .. NP - 1 are live

  // ---- token rows: thread `tid` moves chunk (tid & 3) of rows 64 i + (tid >> 2), i < NP, of every K-tile; rows past the window's end
  // read the last row again (their outputs are masked) ------------------------------------------------------------------------------------
  const unsigned char *rowp[NP];
  const int tr = tid >> 2, tc = tid & 3;
  const int ldst = tr * WS_BK + ((tc ^ w4a8_f(tr)) << 4);            // + i * 64 rows (rows tr and 64 + tr share f)
  {
    int slot[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) slot[i] = 0;
    if (p.slot_map != nullptr) {  // the slots first, so that their loads are in flight together
#pragma unroll
      for (int i = 0; i < NP; ++i) slot[i] = p.slot_map[slot0 + min(m0 + 64 * i + tr, rend - 1)];
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int gr = min(m0 + 64 * i + tr, rend - 1);
      const unsigned char *row;
      if (p.slot_map != nullptr) row = slot[i] < 0 ? p.zero_row : p.A + (long long)(slot[i] % p.T) * p.lda;
      else row = p.A + (long long)e * p.a_stride_e + (long long)gr * p.lda;
      rowp[i] = row + tc * 16;
    }
  }
  auto tstore = [&](unsigned char *stage, const u32x4 (&t)[NP], auto np) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < decltype(np)::value; ++i) *reinterpret_cast<u32x4 *>(stage + i * (64 * WS_BK) + ldst) = t[i];
  };

  // ---- weights: the wave's 32-channel group, clamped to the last one (a clamped wave computes and stores nothing new) ---------------------
  const int nt = min((n0 >> 5) + wn, NT - 1);
  const bool wave_live = (n0 >> 5) + wn < NT;
  W4Ring ring;
  ring.open(p, e, nt, lane);
#pragma unroll
  for (int d = 0; d < WS_DEPTH; ++d) ring.load(d, d);

  f32x16 acc[MG];
#pragma unroll
  for (int mi = 0; mi < MG; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mi][r] = 0.f;

  // token tile 0 goes to LDS here, tile 1 waits in treg[1] (treg[j]: a tile of parity j)
  u32x4 treg[2][NP];
#pragma unroll
  for (int i = 0; i < NP; ++i)
    if (i < 2 || wide) treg[0][i] = *reinterpret_cast<const u32x4 *>(rowp[i]);
#pragma unroll
  for (int i = 0; i < NP; ++i)
    if (i < 2 || wide) treg[1][i] = *reinterpret_cast<const u32x4 *>(rowp[i] + (long long)min(1, nk - 1) * WS_BK);
  if (wide) tstore(smem, treg[0], std::integral_constant<int, NP>{});
  else tstore(smem, treg[0], std::integral_constant<int, 2>{});
  __syncthreads();

  // the lane's fragment: chunks kg (k = 16 kg .. + 15) and kg + 2 (k = 32 + 16 kg .. + 15) of row 32 mi + l31 -- the fp8 operand's K
  // order, file header (rows 32 mi + l31 share f)
  const int lf = w4a8_f(l31);
  const unsigned char *frag0 = smem + l31 * WS_BK + ((kg ^ lf) << 4);   // + mi * 32 rows
  const unsigned char *frag1 = smem + l31 * WS_BK + (((kg + 2) ^ lf) << 4);
  // the shift that brings the K-tile's scale byte 2 (t & 1) + kg to byte 0, per parity of t; the activations' block scale 2^0
  const int ssh[2] = {8 * kg, 8 * kg + 16};
  uint32_t one = 127u;
  asm volatile("" : "+v"(one));   // in a register: a constant scale operand would be encoded as an fp32 inline constant

  auto kloop = [&](auto nmi_c) __attribute__((always_inline)) {
    constexpr int NMI = decltype(nmi_c)::value;
    constexpr auto np = std::integral_constant<int, (NMI <= 4 ? 2 : NP)>{};   // token passes per K-tile
    for (int kt0 = 0; kt0 < nk; kt0 += WS_DEPTH) {
#pragma unroll
      for (int d = 0; d < WS_DEPTH; ++d) {
        const int kt = kt0 + d;   // kt & 1 == d & 1: kt0 is a multiple of the even ring depth
        if (kt >= nk) break;  // block-uniform
        // token tile kt + 2 (behind the last tile: that tile again -- it is stored into the free stage and never read)
        const long long tnext = (long long)min(kt + 2, nk - 1) * WS_BK;
#pragma unroll
        for (int i = 0; i < np(); ++i) treg[d & 1][i] = *reinterpret_cast<const u32x4 *>(rowp[i] + tnext);
        // the K-tile's operand: block kg of the tile in ascending k, its scale byte in byte 0; then the slot's refill
        uint32_t q0 = ring.w[d][0], q1 = ring.w[d][1], q2 = ring.w[d][2], q3 = ring.w[d][3];
        w4a8_swap(q0, q2);
        w4a8_swap(q1, q3);
        const i32x8 wa = {(int)q0, (int)q2, (int)q1, (int)q3, 0, 0, 0, 0};
        const uint32_t sc = ring.s[d] >> ssh[d & 1];
        ring.load(d, kt + WS_DEPTH);
        // a batch of live groups' fragments is asked for in front of the batch's first matrix instruction: every group of the
        // 128-row loops, two groups at a time above four (the wide window's registers, w4a8_tile's header)
        const int so = (kt & 1) * STAGE;
        constexpr int NB = NMI <= 4 ? NMI : 2;
#pragma unroll
        for (int m0g = 0; m0g < NMI; m0g += NB) {
          u32x4 tb[NB][2];
#pragma unroll
          for (int mi = 0; mi < NB; ++mi) {
            if (m0g + mi < NMI) {
              tb[mi][0] = *reinterpret_cast<const u32x4 *>(frag0 + so + (m0g + mi) * (32 * WS_BK));
              tb[mi][1] = *reinterpret_cast<const u32x4 *>(frag1 + so + (m0g + mi) * (32 * WS_BK));
            }
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int mi = 0; mi < NB; ++mi) {
            if (m0g + mi < NMI) {
              const i32x8 b = {(int)tb[mi][0][0], (int)tb[mi][0][1], (int)tb[mi][0][2], (int)tb[mi][0][3],
                               (int)tb[mi][1][0], (int)tb[mi][1][1], (int)tb[mi][1][2], (int)tb[mi][1][3]};
              acc[m0g + mi] = w4a8_mma(wa, b, acc[m0g + mi], sc, one);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        // the other stage is free since the last barrier (behind the last tile nobody reads what is stored)
        tstore(smem + ((kt + 1) & 1) * STAGE, treg[(d + 1) & 1], np);
        __syncthreads();
      }
    }
  };
  switch (nmi) {   // (block-uniform)
    case 1: kloop(std::integral_constant<int, 1>{}); break;
    case 2: kloop(std::integral_constant<int, 2>{}); break;
    case 3: kloop(std::integral_constant<int, 3>{}); break;
    default:
      if constexpr (MG == 4) {
        kloop(std::integral_constant<int, 4>{});
      } else {
        switch (nmi) {
          case 4: kloop(std::integral_constant<int, 4>{}); break;
          case 5: kloop(std::integral_constant<int, 5>{}); break;
          case 6: kloop(std::integral_constant<int, 6>{}); break;
          case 7: kloop(std::integral_constant<int, 7>{}); break;
          default: kloop(std::integral_constant<int, 8>{}); break;
        }
      }
      break;
  }

  // ---- epilogue: lane = row m0 + 32 mi + l31; register 4 rg + r of accumulator mi = channel 32 nt + 8 rg + 4 kg + r ---------------------
  if (!wave_live) return;
  // the lane's row scales and bias, all fetched before the first is used
  float sa[MG];
  {
    int slot[MG];
#pragma unroll
    for (int mi = 0; mi < MG; ++mi) slot[mi] = 0;
    if (p.slot_map != nullptr) {
#pragma unroll
      for (int mi = 0; mi < MG; ++mi) slot[mi] = p.slot_map[slot0 + min(m0 + mi * 32 + l31, rend - 1)];
    }
#pragma unroll
    for (int mi = 0; mi < MG; ++mi) {
      if (p.slot_map != nullptr) sa[mi] = slot[mi] < 0 ? 1.0f : p.a_scale[slot[mi] % p.T];
      else sa[mi] = p.a_scale[slot0 + min(m0 + mi * 32 + l31, rend - 1)];
    }
  }
  uint2 bi[4];
  if constexpr (!GLU) {
#pragma unroll
    for (int rg = 0; rg < 4; ++rg)
      bi[rg] = p.bias != nullptr ? *reinterpret_cast<const uint2 *>(p.bias + (long long)e * p.bias_stride_e + nt * 32 + rg * 8 + kg * 4)
                                 : make_uint2(0u, 0u);
  }
  auto store4 = [&](uint16_t *dst, const T (&o)[4]) __attribute__((always_inline)) {
    uint16_t h[4];
    __builtin_memcpy(h, o, 8);
    uint2 ov;
    ov.x = (uint32_t)h[0] | ((uint32_t)h[1] << 16);
    ov.y = (uint32_t)h[2] | ((uint32_t)h[3] << 16);
    *reinterpret_cast<uint2 *>(dst) = ov;
  };
#pragma unroll
  for (int mi = 0; mi < MG; ++mi) {
    const int m = m0 + mi * 32 + l31;
    if (m >= rend) continue;
    uint16_t *drow = p.D + (long long)e * p.d_stride_e + (long long)m * p.ldd + nt * (GLU ? 16 : 32) + kg * 4;
    if constexpr (GLU) {
      // registers rg = 0, 1 are gate channels 16 nt + 8 rg + 4 kg + r of the expert, registers rg + 2 the up channels of the same indices
#pragma unroll
      for (int rg = 0; rg < 2; ++rg) {
        T o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float a = activate<ACT>(__fmul_rn(acc[mi][rg * 4 + r], sa[mi]));
          asm("" : "+v"(a));  // the fp32 activation exists before it is rounded
          const T g = Elem<T>::from_f32(a);
          float v = __fmul_rn(Elem<T>::to_f32(g), __fmul_rn(acc[mi][(rg + 2) * 4 + r], sa[mi]));
          asm("" : "+v"(v));  // and so does the product
          o[r] = Elem<T>::from_f32(v);
        }
        store4(drow + rg * 8, o);
      }
    } else {
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const uint16_t b4[4] = {(uint16_t)(bi[rg].x & 0xffff), (uint16_t)(bi[rg].x >> 16), (uint16_t)(bi[rg].y & 0xffff), (uint16_t)(bi[rg].y >> 16)};
        T o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = __fmul_rn(acc[mi][rg * 4 + r], sa[mi]);
          if (p.bias != nullptr) {
            T tb;
            __builtin_memcpy(&tb, &b4[r], 2);
            v = __fadd_rn(v, Elem<T>::to_f32(tb));
          }
          v = activate<ACT>(v);
          asm("" : "+v"(v));  // the fp32 value exists before it is rounded (no fused multiply-and-round for fp16)
          o[r] = Elem<T>::from_f32(v);
        }
        store4(drow + rg * 8, o);
      }
    }
  }
}

// (expert, row tile of the bucket [E_loc, R, *], channel tile) in ws_padded's order: the channel tiles of one (expert, row tile) are
// consecutive work items on ONE XCD, whose L2 then fetches the tile's token rows once
template <typename T, int ACT, bool GLU>
__global__ __launch_bounds__(WS_THREADS, 2) void expert_gemm_w4a8_kernel(const W4A8Args p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * A8_STAGE];
  const int b = xcd_work_item((int)gridDim.x);
  const int tn = b % p.ntn, tm = (b / p.ntn) % p.ntm, e = b / (p.ntn * p.ntm);
  w4a8_tile<T, ACT, GLU, 4>(p, smem, e, tn, tm * WS_BM, p.R, (long long)e * p.R);
}

// ---- the packed dropless layout: gemm_wstream.h's work-item order (ws_packed_window), always cut from the live pairs, in two forms -----
// WIDE: one work item per (table tile, channel tile) owns all live rows of the 256-row window, so an expert above 128 rows streams its
// weights once and prepares each K-tile's operand once.  No converts and 128 accumulators: the tile is meant to fit 256 registers, two
// workgroups per CU, 2 x 32 KB of LDS each (profiles/expert_gemm_w4a8_packed_kernel_resources.txt).
// HALVES: the 128-row tile over the two halves of a table tile, the halves that are not live at the end of every XCD's queue.
// Both write the padded kernels' bits (w4a8_tile); TUTEL_AMD_W4A8_PACKED_TILE below picks one at every call.
template <typename T, int ACT, bool GLU>
__global__ __launch_bounds__(WS_THREADS, 2) void expert_gemm_w4a8_packed_kernel(const W4A8Args p, const WsTables t) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * A8_STAGE];   // two stages of 256 rows
  WsWindow w;
  if (!ws_packed_window<1>(p.ntn, t.offsets, t.tiles, t.ntiles, t.tiles_bound, w)) return;
  w4a8_tile<T, ACT, GLU, 8>(p, smem, w.e, w.tn, w.m0, w.rend, 0);
}

template <typename T, int ACT, bool GLU>
__global__ __launch_bounds__(WS_THREADS, 2) void expert_gemm_w4a8_packed_halves_kernel(const W4A8Args p, const WsTables t) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * A8_STAGE];
  WsWindow w;
  if (!ws_packed_window<2>(p.ntn, t.offsets, t.tiles, t.ntiles, t.tiles_bound, w)) return;
  w4a8_tile<T, ACT, GLU, 4>(p, smem, w.e, w.tn, w.m0, w.rend, 0);
}

// TUTEL_AMD_W4A8_PACKED_TILE below
#define W4A8_PACKED_DEFAULT_HALVES 0

// ---- host: gemm_wstream.h's ws_run over the W4 image (w4_image.h's checks) and the quantised rows' own operands -------------------------
struct W4A8Fmt {
  using Args = W4A8Args;
  struct Weights : W4Weights {
    const float *a_scale; int lda; int64_t a_stride_e;   // the activations' own: byte strides of 16-byte aligned fp8 rows
    bool strides_ok() const { return W4Weights::strides_ok() && lda % 16 == 0 && a_stride_e % 16 == 0; }
    bool present() const { return W4Weights::present() && a_scale; }
    bool aligned() const { return W4Weights::aligned() && ((uintptr_t)a_scale % 4) == 0; }
    void fill(W4A8Args &a) const { W4Weights::fill(a); a.a_scale = a_scale; }
  };
  static constexpr WsText TEXT = {
      {"rows of Aq must stay 16-byte aligned (lda, a_stride_e % 16), rows of D and bias 8-byte aligned (% 4), w_stride_e % 16, s_stride_e % 4",
       "rows of Aq must stay 16-byte aligned (lda % 16), rows of D and bias 8-byte aligned (% 4), w_stride_e % 16, s_stride_e % 4"},
      {"E_loc * R, the tile count and one channel group's run of 16 K bytes must stay below 2^31",
       "the work item count tiles_bound * 2 * ceil(channels / 128) and one channel group's run of 16 K bytes must stay below 2^31"},
      "%s: Aq and Wq must be 16-byte aligned, D and bias 8-byte aligned, Ws and a_scale 4-byte aligned"};
  // The form of the packed kernels, read at EVERY call: TUTEL_AMD_W4A8_PACKED_TILE=halves | wide; anything else is the default, which
  // tools/packed_w4a8_bench.py's A/B decided: WIDE -- 72.5 against 96.0 us at 64 x 160 rows, 59.7 against 59.1 us at 64 x 128
  // rows (inside the halves arm's spread of 58.1 - 64.0 us); halves stays selectable
  static bool packed_halves() {
    const char *s = getenv("TUTEL_AMD_W4A8_PACKED_TILE");
    if (s != nullptr && strcmp(s, "halves") == 0) return true;
    if (s != nullptr && strcmp(s, "wide") == 0) return false;
    return W4A8_PACKED_DEFAULT_HALVES != 0;
  }
  template <typename T, int ACT, bool GLU>
  static void launch(const W4A8Args &a, const WsTables *pk, bool halves, unsigned grid, hipStream_t st) {
    if (pk == nullptr) hipLaunchKernelGGL((expert_gemm_w4a8_kernel<T, ACT, GLU>), dim3(grid), dim3(WS_THREADS), 0, st, a);
    else if (halves) hipLaunchKernelGGL((expert_gemm_w4a8_packed_halves_kernel<T, ACT, GLU>), dim3(grid), dim3(WS_THREADS), 0, st, a, *pk);
    else hipLaunchKernelGGL((expert_gemm_w4a8_packed_kernel<T, ACT, GLU>), dim3(grid), dim3(WS_THREADS), 0, st, a, *pk);
  }
};

// dtype is D's and the bias's here, the activations are e4m3: asked in front of ws_run, whose wording names the activations
#define W4A8_DTYPE "D and bias must be bf16 or fp16 (dtype is the output's; the activations are e4m3)"

extern "C" int tutel_amd_expert_gemm_w4a8_supported(int dtype, int N, int K) { return ws_supported(dtype, N, K); }
extern "C" int tutel_amd_expert_gemm_w4a8_glu_supported(int dtype, int H, int K) { return ws_glu_supported(dtype, H, K); }

extern "C" int tutel_amd_expert_gemm_w4a8(const void *Aq, const float *a_scale, int64_t a_stride_e, int64_t a_stride_w, int a_rows_per_w,
                                          int lda, const void *Wq, int64_t w_stride_e, const void *Ws, int64_t s_stride_e, const void *bias,
                                          int64_t bias_stride_e, void *D, int64_t d_stride_e, int64_t d_stride_w, int d_rows_per_w, int ldd,
                                          int E_loc, int R, int N, int K, int dtype, int act, const int32_t *row_counts,
                                          const int32_t *slot_map, int T, const void *zero_row, tutel_stream_t stream) {
  if (!ws_dtype_ok(dtype)) return tutel_notsup("tutel_amd_expert_gemm_w4a8", W4A8_DTYPE);
  const WsBucket bk = {a_stride_e, a_stride_w, a_rows_per_w, d_stride_e, d_stride_w, d_rows_per_w, row_counts};
  return ws_run<W4A8Fmt, false>({"tutel_amd_expert_gemm_w4a8", W4_SMALL}, {{Wq, w_stride_e, Ws, s_stride_e}, a_scale, lda, a_stride_e}, &bk,
                                nullptr, Aq, lda, slot_map, T, zero_row, bias, bias_stride_e, D, ldd, E_loc, R, N, K, dtype, act, stream);
}

// SwiGLU gate and up products of MXFP4 weights over FP8 activations in one launch (the contract: include/tutel_amd.h).  No bias
extern "C" int tutel_amd_expert_gemm_w4a8_glu(const void *Aq, const float *a_scale, int64_t a_stride_e, int64_t a_stride_w,
                                              int a_rows_per_w, int lda, const void *Wq_gu, int64_t w_stride_e, const void *Ws_gu,
                                              int64_t s_stride_e, void *D, int64_t d_stride_e, int64_t d_stride_w, int d_rows_per_w, int ldd,
                                              int E_loc, int R, int H, int K, int dtype, int act, const int32_t *row_counts,
                                              const int32_t *slot_map, int T, const void *zero_row, tutel_stream_t stream) {
  if (!ws_dtype_ok(dtype)) return tutel_notsup("tutel_amd_expert_gemm_w4a8_glu", W4A8_DTYPE);
  const WsBucket bk = {a_stride_e, a_stride_w, a_rows_per_w, d_stride_e, d_stride_w, d_rows_per_w, row_counts};
  return ws_run<W4A8Fmt, true>({"tutel_amd_expert_gemm_w4a8_glu", W4_SMALL_GU}, {{Wq_gu, w_stride_e, Ws_gu, s_stride_e}, a_scale, lda, a_stride_e},
                               &bk, nullptr, Aq, lda, slot_map, T, zero_row, nullptr, 0, D, ldd, E_loc, R, H, K, dtype, act, stream);
}

// The two GEMMs above over the packed dropless layout (the contract: include/tutel_amd.h): the row ranges come from the device tables,
// a_scale is indexed by the packed row, or by the token where a_rows gathers
extern "C" int tutel_amd_expert_gemm_w4a8_packed(const void *Aq, const float *a_scale, int lda, const int32_t *a_rows, int T,
                                                 const void *zero_row, const void *Wq, int64_t w_stride_e, const void *Ws, int64_t s_stride_e,
                                                 const void *bias, int64_t bias_stride_e, void *D, int ldd, int E, int rows_bound, int N, int K,
                                                 int dtype, int act, const int32_t *offsets, const int32_t *tiles, const int32_t *ntiles,
                                                 int tiles_bound, tutel_stream_t stream) {
  if (!ws_dtype_ok(dtype)) return tutel_notsup("tutel_amd_expert_gemm_w4a8_packed", W4A8_DTYPE);
  const WsTables pk = {offsets, tiles, ntiles, tiles_bound};
  return ws_run<W4A8Fmt, false>({"tutel_amd_expert_gemm_w4a8_packed", W4_SMALL}, {{Wq, w_stride_e, Ws, s_stride_e}, a_scale, lda, 0}, nullptr,
                                &pk, Aq, lda, a_rows, T, zero_row, bias, bias_stride_e, D, ldd, E, rows_bound, N, K, dtype, act, stream);
}

extern "C" int tutel_amd_expert_gemm_w4a8_glu_packed(const void *Aq, const float *a_scale, int lda, const int32_t *a_rows, int T,
                                                     const void *zero_row, const void *Wq_gu, int64_t w_stride_e, const void *Ws_gu,
                                                     int64_t s_stride_e, void *D, int ldd, int E, int rows_bound, int H, int K, int dtype,
                                                     int act, const int32_t *offsets, const int32_t *tiles, const int32_t *ntiles,
                                                     int tiles_bound, tutel_stream_t stream) {
  if (!ws_dtype_ok(dtype)) return tutel_notsup("tutel_amd_expert_gemm_w4a8_glu_packed", W4A8_DTYPE);
  const WsTables pk = {offsets, tiles, ntiles, tiles_bound};
  return ws_run<W4A8Fmt, true>({"tutel_amd_expert_gemm_w4a8_glu_packed", W4_SMALL_GU}, {{Wq_gu, w_stride_e, Ws_gu, s_stride_e}, a_scale, lda, 0},
                               nullptr, &pk, Aq, lda, a_rows, T, zero_row, nullptr, 0, D, ldd, E, rows_bound, H, K, dtype, act, stream);
}
