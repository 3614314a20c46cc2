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
// The packed dropless layout (tutel_amd_expert_gemm_w8a8_packed / _glu_packed): the same tile over row windows read from the device
// tables, as two 128-row halves or as one WIDE 256-row window per table tile (a8_tile's MG; the kernels stand behind the padded one).
// The wide window's panel is two stages of 256 rows x 64 bytes (32 KB) and thread `tid` moves chunk tid & 3 of rows 64 i + (tid >> 2),
// i < 4: four 16-byte global loads per K-tile, two tiles ahead.  The swizzle over rows 128 .. 255: f reads bits 1 .. 4 of r only, so
// f(r + 32 j) = f(r), and 32 rows are 2048 bytes, a multiple of both bank periods (128 and 256 bytes): group mi's fragment read hits
// the banks of group 0's, and pass i's store those of pass 0's.  Checked by enumeration as well -- for both bank models, every
// (group mi < 8, K-step q, kg) ds_read_b64 taken 16 (32) lanes at a time and every (pass i < 4, wave) ds_write_b128 taken 8 (16) lanes
// at a time touches each 8-byte (16-byte) unit of the bank period once: conflict-free across all 256 rows.
//
// SwiGLU experts (tutel_amd_expert_gemm_w8a8_glu): D = round_T( round_T(act(gacc sa sg)) * (uacc sa su) ) over the interleaved gate / up
// image, register against register as in the W8A16 kernel.
#include "gemm_wstream.h"

#ifndef W8A8_WIDE_WG
#define W8A8_WIDE_WG 2   // workgroups per CU the wide packed kernel is compiled for (1: measured once)
#endif
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

// the storing thread's chunks of NPASS token passes into a stage (file header: the halves of a chunk swap places where f(r) is odd)
template <int NPASS, int NP>
__device__ __forceinline__ void a8_tstore(unsigned char *stage, const u32x4 (&t)[NP], const int ldst, const bool tswap) {
#pragma unroll
  for (int i = 0; i < NPASS; ++i) {
    u32x4 v = t[i];
    if (tswap) v = u32x4{t[i][2], t[i][3], t[i][0], t[i][1]};
    *reinterpret_cast<u32x4 *>(stage + i * (64 * WS_BK) + ldst) = v;
  }
}

// The K loop for NMI live 32-row groups; NMI = 0: the loop that is not specialised, reads the four groups' fragments and tests each
// group against nmi (the 128-row tile's).  A K-tile is 4 NB STEPS: step (q, b) issues operand q against batch b of GB groups -- the
// batch's ds_read_b64 were asked for one step earlier, in front of the previous step's matrix instructions.  Up to four live groups
// one batch holds them all (GB = 4: the 128-row tile's cadence).  Above four a batch is TWO groups: the fragments in flight are then
// two batches of two (8 registers, not the 32 of eight groups double-buffered), and the operands are the ring slot's own registers,
// each half of the slot refilled behind the last step that reads it (no copies: another 8) -- with 128 accumulators, 32 ring and 32
// token registers that is what the 256-row window's budget leaves.  The operand order seen by one accumulator is q = 0 .. 3 of
// K-tile 0, 1, ..: K ascending, whatever NMI.
template <int MG, int NMI>
__device__ __forceinline__ void a8_kloop(u32x4 (&w)[WS_DEPTH][2], const __amdgpu_buffer_rsrc_t rs, const int wl, f32x16 (&acc)[MG],
                                         u32x4 (&treg)[2][MG / 2], const unsigned char *const (&rowp)[MG / 2], unsigned char *smem,
                                         const unsigned char *frag, const int ldst, const bool tswap, const int nk, const int nmi,
                                         const int kg, const int lf) {
  constexpr int NF = NMI == 0 ? 4 : NMI;                                    // groups whose fragments are read
  constexpr int GB = NF <= 4 ? 4 : 2;                                       // groups per batch
  constexpr int NB = (NF + GB - 1) / GB;                                    // batches per operand
  constexpr int NP = MG / 2, STAGE = MG * 32 * WS_BK;
  constexpr int np = NMI <= 4 ? 2 : NP;                                     // token passes per K-tile
  for (int kt0 = 0; kt0 < nk; kt0 += WS_DEPTH) {
#pragma unroll
    for (int d = 0; d < WS_DEPTH; ++d) {
      const int kt = kt0 + d;   // kt & 1 == d & 1: kt0 is a multiple of the even ring depth
      if (kt >= nk) break;  // block-uniform
      // token tile kt + 2 (behind the last tile: that tile again -- it is stored into the free stage and never read)
      const long long tnext = (long long)min(kt + 2, nk - 1) * WS_BK;
#pragma unroll
      for (int i = 0; i < np; ++i) treg[d & 1][i] = *reinterpret_cast<const u32x4 *>(rowp[i] + tnext);
      // the K-tile's four operands: operand q = 2 h + s holds k = 64 kt + 16 q + 8 kg .. + 7; then the slot's refill
      a8_op wa[4];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int s = 0; s < 2; ++s) wa[2 * h + s] = a8_op{w[d][h][2 * s], w[d][h][2 * s + 1]};
      if constexpr (NF <= 4) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
          w[d][h] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, wl, (kt + WS_DEPTH) * 2048 + h * 1024, 2));
      }
      // operand q multiplies slot 2 q + kg of every row; the fragments of step s + 1 are asked for before the matrix instructions
      // of step s
      const unsigned char *st = frag + (kt & 1) * STAGE;
      a8_op tb[2][GB];
#pragma unroll
      for (int mi = 0; mi < GB; ++mi)
        if (mi < NF) tb[0][mi] = *reinterpret_cast<const a8_op *>(st + mi * (32 * WS_BK) + ((kg ^ lf) << 3));
#pragma unroll
      for (int s = 0; s < 4 * NB; ++s) {
        const int q = s / NB, b = s % NB;   // (constants of the unrolled step)
        if (s + 1 < 4 * NB) {
          const int q1 = (s + 1) / NB, b1 = (s + 1) % NB;
#pragma unroll
          for (int mi = 0; mi < GB; ++mi)
            if (GB * b1 + mi < NF)
              tb[(s + 1) & 1][mi] = *reinterpret_cast<const a8_op *>(st + (GB * b1 + mi) * (32 * WS_BK) + (((2 * q1 + kg) ^ lf) << 3));
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mi = 0; mi < GB; ++mi)
          if (GB * b + mi < NF && (NMI != 0 || mi < nmi))
            acc[GB * b + mi] = a8_mma(NF > 4 ? a8_op{w[d][q >> 1][2 * (q & 1)], w[d][q >> 1][2 * (q & 1) + 1]} : wa[q], tb[s & 1][mi], acc[GB * b + mi]);
        // above four groups the operand is read from the ring slot's own registers at its step (wa is not used: the window's register
        // budget), so each half of the slot is refilled behind the last step that reads it
        if constexpr (NF > 4) {
          if (s == 2 * NB - 1 || s == 4 * NB - 1)
            w[d][q >> 1] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, wl, (kt + WS_DEPTH) * 2048 + (q >> 1) * 1024, 2));
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // the other stage is free since the last barrier (behind the last tile nobody reads what is stored)
      a8_tstore<np>(smem + ((kt + 1) & 1) * STAGE, treg[(d + 1) & 1], ldst, tswap);
      __syncthreads();
    }
  }
}

// One (expert, 32 MG rows, 128 image channels) work item: expert e, rows [m0, min(m0 + 32 MG, rend)), channel tile tn; slot0: the slot
// -- and the index of the row scale -- of the layout's row 0 (e * R in the bucket, 0 on the packed layout, whose rows are absolute).
// GLU: p.N = 2 H image channels, and only the epilogue differs.
//   MG = 4: the 128-row tile of the padded kernels and of the packed kernels' halves form; ONE K loop that tests each 32-row group
//           against the live count.
//   MG = 8: the WIDE window of the packed layout, a whole 256-row table tile: the K loop is compiled per live-group count 1 .. 8 (a8_kloop): a 129-row expert
//           pays for five groups.  Counts 1 .. 4 move two token passes (rows 128 .. 255 of the panel are neither written nor read).
// Whatever MG and the count: one fp32 accumulator per output, K ascending in steps of 16, the same operands, the same epilogue -- the
// same bits.
template <typename T, int ACT, bool GLU, int MG>
__device__ __forceinline__ void a8_tile(const A8Args &p, unsigned char *smem, const int e, const int tn, const int m0, const int rend,
                                        const long long slot0) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, kg = lane >> 5;
  const int n0 = tn * WS_BN;
  const int nk = p.K / WS_BK;
  const int NT = p.N >> 5;
  constexpr int NP = MG / 2;                       // token passes of 64 rows
  constexpr int STAGE = MG * 32 * WS_BK;           // one stage of the token panel
  const int nmi = min(MG, (rend - m0 + 31) >> 5);  // live 32-row groups of this tile
  const bool wide = MG > 4 && nmi > 4;             // (block-uniform) the token passes 2 .. NP - 1 are live

  // ---- token rows: thread `tid` moves chunk (tid & 3) of rows 64 i + (tid >> 2), i < NP, of every K-tile; rows past the window's end
  // read the last row again (their outputs are masked) ------------------------------------------------------------------------------------
  const unsigned char *rowp[NP];
  const int tr = tid >> 2, tc = tid & 3;
  const int tf = a8_f(tr);                                           // (rows tr + 64 i share it)
  const int ldst = tr * WS_BK + ((2 * tc) ^ (tf & 6)) * 8;           // + i * 64 rows
  const bool tswap = (tf & 1) != 0;
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
  if (wide) a8_tstore<NP>(smem, treg[0], ldst, tswap);
  else a8_tstore<2>(smem, treg[0], ldst, tswap);
  __syncthreads();

  const int lf = a8_f(l31);                      // (rows 32 mi + l31 share it)
  const unsigned char *frag = smem + l31 * WS_BK;   // + mi * 32 rows

  if constexpr (MG == 4) {
    a8_kloop<MG, 0>(w, rs, wl, acc, treg, rowp, smem, frag, ldst, tswap, nk, nmi, kg, lf);
  } else {
    auto kloop = [&](auto nmi_c) __attribute__((always_inline)) {
      a8_kloop<MG, decltype(nmi_c)::value>(w, rs, wl, acc, treg, rowp, smem, frag, ldst, tswap, nk, nmi, kg, lf);
    };
    switch (nmi) {   // (block-uniform)
      case 1: kloop(std::integral_constant<int, 1>{}); break;
      case 2: kloop(std::integral_constant<int, 2>{}); break;
      case 3: kloop(std::integral_constant<int, 3>{}); break;
      case 4: kloop(std::integral_constant<int, 4>{}); break;
      case 5: kloop(std::integral_constant<int, 5>{}); break;
      case 6: kloop(std::integral_constant<int, 6>{}); break;
      case 7: kloop(std::integral_constant<int, 7>{}); break;
      default: kloop(std::integral_constant<int, 8>{}); break;
    }
  }

  // ---- epilogue: lane = row m0 + 32 mi + l31; register 4 rg + r of accumulator mi = channel 32 nt + 8 rg + 4 kg + r ---------------------
  if (!wave_live) return;
  // the lane's row scales, channel scales and bias, all fetched before the first is used
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
    for (int mi = 0; mi < MG; ++mi) {
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
  for (int mi = 0; mi < MG; ++mi) {
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
  a8_tile<T, ACT, GLU, 4>(p, smem, e, tn, tm * WS_BM, p.R, (long long)e * p.R);
}

// ---- the packed dropless layout: gemm_wstream.h's work-item order (ws_packed_window), always cut from the live pairs, in two forms -----
// WIDE: one work item per (table tile, channel tile) owns all live rows of the 256-row window, so an expert above 128 rows streams its
// weights once and splits each K-tile into its operands once (file header).  2 x 16 KB of LDS per workgroup.
// HALVES: the 128-row tile over the two halves of a table tile, the halves that are not live at the end of every XCD's queue.
// Both write the padded kernels' bits (a8_tile); TUTEL_AMD_W8A8_PACKED_TILE below picks one at every call.
template <typename T, int ACT, bool GLU>
__global__ __launch_bounds__(WS_THREADS, W8A8_WIDE_WG) void expert_gemm_w8a8_packed_kernel(const A8Args p, const WsTables t) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * A8_STAGE];   // two stages of 256 rows
  WsWindow w;
  if (!ws_packed_window<1>(p.ntn, t.offsets, t.tiles, t.ntiles, t.tiles_bound, w)) return;
  a8_tile<T, ACT, GLU, 8>(p, smem, w.e, w.tn, w.m0, w.rend, 0);
}

template <typename T, int ACT, bool GLU>
__global__ __launch_bounds__(WS_THREADS, 2) void expert_gemm_w8a8_packed_halves_kernel(const A8Args p, const WsTables t) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * A8_STAGE];
  WsWindow w;
  if (!ws_packed_window<2>(p.ntn, t.offsets, t.tiles, t.ntiles, t.tiles_bound, w)) return;
  a8_tile<T, ACT, GLU, 4>(p, smem, w.e, w.tn, w.m0, w.rend, 0);
}

// TUTEL_AMD_W8A8_PACKED_TILE below.  The rule: wide is the default only if it has no scratch AND is faster at 64 x 160 rows AND at 64 x 128
// rows is not slower than halves by more than the halves arm's own min - max spread.  Measured (tools/packed_w8a8_bench.py, one MI355X,
// bf16, N = K = 2048, fc1): wide 99.8 us against halves 129.7 us at 64 x 160 rows, 80.6 against 79.1 us at 64 x 128 rows (inside the
// halves arm's spread of 76.9 - 81.8 us) -- the timing half holds.  The resource half does not: the wide kernels are 254 VGPRs and 20
// bytes of scratch (one 16-byte spill around a specialised K loop; profiles/expert_gemm_w8a8_packed_kernel_resources.txt).  A form that
// spills is not the default: HALVES, and wide stays selectable.  (One workgroup per CU, W8A8_WIDE_WG = 1, has no scratch -- 183 VGPRs +
// 128 AGPRs -- but takes 100.2 us against halves' 77.1 us at 64 x 128 rows: it fails the rule's second clause.)
#define W8A8_PACKED_DEFAULT_HALVES 1

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
      {"rows of Aq must stay 16-byte aligned (lda, a_stride_e % 16), rows of D and bias 8-byte aligned (% 4), w_stride_e % 16",
       "rows of Aq must stay 16-byte aligned (lda % 16), rows of D and bias 8-byte aligned (% 4), w_stride_e % 16"},
      {"E_loc * R and the tile count must stay below 2^31", "the work item count tiles_bound * 2 * ceil(channels / 128) must stay below 2^31"},
      "%s: Aq, Wq and scale must be 16-byte aligned, D and bias 8-byte aligned, a_scale 4-byte aligned"};
  // The form of the packed kernels, read at EVERY call: TUTEL_AMD_W8A8_PACKED_TILE=halves | wide; anything else is the default: halves
  // (the numbers stand at W8A8_PACKED_DEFAULT_HALVES above and in DESIGN 4.4)
  static bool packed_halves() {
    const char *s = getenv("TUTEL_AMD_W8A8_PACKED_TILE");
    if (s != nullptr && strcmp(s, "halves") == 0) return true;
    if (s != nullptr && strcmp(s, "wide") == 0) return false;
    return W8A8_PACKED_DEFAULT_HALVES != 0;
  }
  template <typename T, int ACT, bool GLU>
  static void launch(const A8Args &a, const WsTables *pk, bool halves, unsigned grid, hipStream_t st) {
    if (pk == nullptr) hipLaunchKernelGGL((expert_gemm_w8a8_kernel<T, ACT, GLU>), dim3(grid), dim3(WS_THREADS), 0, st, a);
    else if (halves) hipLaunchKernelGGL((expert_gemm_w8a8_packed_halves_kernel<T, ACT, GLU>), dim3(grid), dim3(WS_THREADS), 0, st, a, *pk);
    else hipLaunchKernelGGL((expert_gemm_w8a8_packed_kernel<T, ACT, GLU>), dim3(grid), dim3(WS_THREADS), 0, st, a, *pk);
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

// The two GEMMs above over the packed dropless layout (the contract: include/tutel_amd.h): the row ranges come from the device tables,
// a_scale is indexed by the packed row, or by the token where a_rows gathers
extern "C" int tutel_amd_expert_gemm_w8a8_packed(const void *Aq, const float *a_scale, int lda, const int32_t *a_rows, int T,
                                                 const void *zero_row, const void *Wq, int64_t w_stride_e, const float *scale,
                                                 const void *bias, int64_t bias_stride_e, void *D, int ldd, int E, int rows_bound, int N, int K,
                                                 int dtype, int act, const int32_t *offsets, const int32_t *tiles, const int32_t *ntiles,
                                                 int tiles_bound, tutel_stream_t stream) {
  const WsTables pk = {offsets, tiles, ntiles, tiles_bound};
  return ws_run<A8Fmt, false>({"tutel_amd_expert_gemm_w8a8_packed", "w_stride_e is smaller than one expert's image (N * K bytes)"},
                              {Wq, w_stride_e, scale, a_scale, lda, 0}, nullptr, &pk, Aq, lda, a_rows, T, zero_row, bias, bias_stride_e, D,
                              ldd, E, rows_bound, N, K, dtype, act, stream);
}

extern "C" int tutel_amd_expert_gemm_w8a8_glu_packed(const void *Aq, const float *a_scale, int lda, const int32_t *a_rows, int T,
                                                     const void *zero_row, const void *Wq_gu, int64_t w_stride_e, const float *scale_gu,
                                                     void *D, int ldd, int E, int rows_bound, int H, int K, int dtype, int act,
                                                     const int32_t *offsets, const int32_t *tiles, const int32_t *ntiles, int tiles_bound,
                                                     tutel_stream_t stream) {
  const WsTables pk = {offsets, tiles, ntiles, tiles_bound};
  return ws_run<A8Fmt, true>({"tutel_amd_expert_gemm_w8a8_glu_packed", "w_stride_e is smaller than one expert's image (2 * H * K bytes)"},
                             {Wq_gu, w_stride_e, scale_gu, a_scale, lda, 0}, nullptr, &pk, Aq, lda, a_rows, T, zero_row, nullptr, 0, D, ldd,
                             E, rows_bound, H, K, dtype, act, stream);
}
