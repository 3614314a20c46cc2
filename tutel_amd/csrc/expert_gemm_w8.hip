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
// The launch is a weight-streaming problem (<= 128 rows per expert: every weight byte is used once), so the shape of the kernel
// follows the bytes:
//   * the weight image is the kernel's own layout (include/tutel_amd.h, tutel_amd/experts/w8.py::pack): blocked by (32 channels,
//     32 k, lane) so that ONE global_load_dwordx4 per lane fetches 1 KB contiguous per wave -- the MFMA fragments of two K-steps of
//     16 for the lane's channel -- and a wave walks its 32 channels' whole K extent as one contiguous run of K * 32 bytes.
//     Weight bytes go global -> VGPR -> convert -> MFMA operand and never touch LDS; a register ring keeps W8_DEPTH K-tiles
//     (2 KB per wave each) in flight;
//   * one 4-wave workgroup per (expert, 128 rows, 128 channels): wave w owns channels 32 w .. 32 w + 31 of the tile and all 128
//     rows (4 accumulators of 32 x 32; 32-row groups past R are skipped);
//   * token rows go through LDS, K-tiles of 64 in two stages of 16 KB, in the swizzled 128-byte-row panel of the other GEMMs
//     (16-byte chunk c of row r at c ^ ((r >> 1) & 7)): 16-byte global loads into registers, issued two tiles ahead, stored after the
//     previous tile's matrix instructions, one barrier per K-tile.  Rows: the plain [E_loc, R, K] form, or gathered from the tokens through the
//     slot map (negative slot: the zero row);
//   * weights are the A operand of the matrix instruction and token rows the B operand: a lane ends with ONE row and, per
//     register group, 4 consecutive channels -- 8-byte stores, scale and bias as 4-vectors fetched once per lane in front of the epilogue;
//   * R > 128 runs as several row tiles that each stream the weights again: correct, not the design point.
//   * ragged tiles: rows past R and channel groups past N clamp their loads (to the last row / the last 32-channel group) and mask
//     their stores; nothing is read or written outside the operands.
//
// SwiGLU experts (tutel_amd_expert_gemm_w8_glu): D = round_T( round_T(act(gacc * scale_gate)) * (uacc * scale_up) ), the gate and up
// products of one launch.  The image holds both matrices, interleaved by 16 channels (experts/w8.py::interleave_gate_up): in every
// 32-channel group positions 0 .. 15 are gate channels 16 g .. 16 g + 15 and positions 16 .. 31 the up channels of the same indices.
// A lane's accumulator registers rg = 0, 1 are then gate channels and rg + 2 the up channels of the SAME outputs, so the gating
// product is register against register: same K loop over 2 H image channels (w8_tile), token rows read once, the gate never written
// to memory, no LDS and no cross-lane move in the epilogue.  One workgroup is 128 image channels = 64 output channels x 128 rows.
#include "gemm_dev.h"  // Mma<T>, activate<ACT>

#define W8_BM 128
#define W8_BN 128
#define W8_BK 64
#define W8_THREADS 256
#define W8_DEPTH 4       // K-tiles of weights in flight per wave (even: the token registers alternate with it); 8 measured the same
#define W8_STAGE (W8_BM * W8_BK * 2)

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

// One (expert, 128 rows, 128 image channels) work item; both kernels below are this function.  GLU: the image holds a SwiGLU expert's
// gate and up channels interleaved by 16 (experts/w8.py::interleave_gate_up), p.N = 2 H image channels, and only the epilogue differs.
//
// The work item is a ROW WINDOW: expert e (its weights, scale and bias), rows [m0, min(m0 + 128, rend)) and channel tile tn.  Rows are
// numbered as the caller's layout numbers them -- within the expert's bucket for the padded kernels (row r of A at e * a_stride_e +
// r * lda, its slot at slot0 + r with slot0 = e * R), absolute packed rows for the packed ones (a_stride_e = d_stride_e = 0, slot0 = 0,
// rend = offsets[e + 1]: the rows from rend on are the NEXT expert's and are neither read nor written).
template <typename T, int ACT, bool GLU>
__device__ __forceinline__ void w8_tile(const W8Args &p, unsigned char *smem, const int e, const int tn, const int m0, const int rend,
                                        const long long slot0) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, kg = lane >> 5;
  const int n0 = tn * W8_BN;
  const int nk = p.K / W8_BK;
  const int NT = p.N >> 5, KT32 = p.K >> 5;
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
  // The group's run of K * 32 bytes is read through a buffer descriptor of exactly that size: every load of the K loop is
  // UNCONDITIONAL (a load under a branch makes the compiler wait for all loads in flight where the branches join), and the refills
  // past the last K-tile are out of the descriptor's range -- they fetch nothing and return zeros that are never used.
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<unsigned char *>(p.Wq + (long long)e * p.w_stride_e + (long long)nt * KT32 * 1024), 0, KT32 * 1024, 0x00020000);
  const int wl = lane * 16;
  u32x4 wreg[W8_DEPTH][2];
#pragma unroll
  for (int d = 0; d < W8_DEPTH; ++d) {
#pragma unroll
    for (int h = 0; h < 2; ++h) wreg[d][h] = w8_wload(rs_w, wl, d * 2048 + h * 1024);
  }

  f32x16 acc[4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mi][r] = 0.f;

  // Token rows run TWO tiles ahead in registers (treg[j]: a tile of parity j): the memory counter retires loads in order, so waiting
  // for a token tile asked for only one step ago would also wait for every weight refill issued before it -- the ring would be one
  // tile deep whatever W8_DEPTH says.  Tile 0 goes to LDS here, tile 1 waits in treg[1]
  u32x4 treg[2][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) treg[0][i] = *reinterpret_cast<const u32x4 *>(rowp[i]);
#pragma unroll
  for (int i = 0; i < 4; ++i) treg[1][i] = *reinterpret_cast<const u32x4 *>(rowp[i] + (long long)min(1, nk - 1) * (W8_BK * 2));
#pragma unroll
  for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4 *>(smem + ldst[i]) = treg[0][i];
  __syncthreads();

  const int sw = (l31 >> 1) & 7;
  const int frag = l31 * 128;  // + mi * 32 rows

  for (int kt0 = 0; kt0 < nk; kt0 += W8_DEPTH) {
#pragma unroll
    for (int d = 0; d < W8_DEPTH; ++d) {
      const int kt = kt0 + d;
      if (kt >= nk) break;  // block-uniform
      // token tile kt + 2 (behind the last tile: that tile again -- it is stored into the free stage and never read)
      const long long tnext = (long long)min(kt + 2, nk - 1) * (W8_BK * 2);
#pragma unroll
      for (int i = 0; i < 4; ++i) treg[d & 1][i] = *reinterpret_cast<const u32x4 *>(rowp[i] + tnext);
      // the K-tile's four operands of 8 k: word pair s of load h holds k = 64 kt + 32 h + 16 s + 8 kg .. + 7
      u32x4 wa[4];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int s = 0; s < 2; ++s) wa[2 * h + s] = w8_widen<T>(wreg[d][h][2 * s], wreg[d][h][2 * s + 1]);
#pragma unroll
      for (int h = 0; h < 2; ++h) wreg[d][h] = w8_wload(rs_w, wl, (kt + W8_DEPTH) * 2048 + h * 1024);
      // operand q multiplies token chunk 2 q + kg of every row; the fragments of operand q + 1 are asked for before the matrix
      // instructions of operand q (two sets of four in registers, not all sixteen)
      const unsigned char *st = smem + (kt & 1) * W8_STAGE + frag;
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
          if (mi < nmi) acc[mi] = Mma<T>::run(wa[q], tb[q & 1][mi], acc[mi]);
        __builtin_amdgcn_sched_barrier(0);
      }
      {  // the other stage is free since the last barrier (behind the last tile nobody reads what is stored)
        unsigned char *nx = smem + ((kt + 1) & 1) * W8_STAGE;
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4 *>(nx + ldst[i]) = treg[(d + 1) & 1][i];
      }
      __syncthreads();
    }
  }

  // ---- epilogue: lane = row m0 + 32 mi + l31; register 4 rg + r of accumulator mi = channel 32 nt + 8 rg + 4 kg + r ---------------------
  if (!wave_live) return;
  // scale and bias of the lane's channels 32 nt + 8 rg + 4 kg .. + 3, all fetched before the first is used
  float4 sc[4];
  uint2 bi[4];
#pragma unroll
  for (int rg = 0; rg < 4; ++rg) {
    const int n = nt * 32 + rg * 8 + kg * 4;
    sc[rg] = *reinterpret_cast<const float4 *>(p.scale + (long long)e * p.N + n);
    bi[rg] = p.bias != nullptr ? *reinterpret_cast<const uint2 *>(p.bias + (long long)e * p.bias_stride_e + n) : make_uint2(0u, 0u);
  }
  if constexpr (GLU) {
    // Registers rg = 0, 1 are gate channels 16 nt + 8 rg + 4 kg + r of the expert, registers rg + 2 the up channels of the same
    // indices (the image's interleave): the gating product is register against register in this lane.  g = act(gacc * scale_gate)
    // rounded to T, u = uacc * scale_up, D = round_T(float(g) * u) -- tutel_amd_expert_gemm_gate_up's order; no bias
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const int m = m0 + mi * 32 + l31;
      if (m >= rend) continue;
      uint16_t *drow = p.D + (long long)e * p.d_stride_e + (long long)m * p.ldd + nt * 16 + kg * 4;
#pragma unroll
      for (int rg = 0; rg < 2; ++rg) {
        const float sg[4] = {sc[rg].x, sc[rg].y, sc[rg].z, sc[rg].w};
        const float su[4] = {sc[rg + 2].x, sc[rg + 2].y, sc[rg + 2].z, sc[rg + 2].w};
        uint16_t o[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float a = activate<ACT>(__fmul_rn(acc[mi][rg * 4 + r], sg[r]));
          asm("" : "+v"(a));  // the fp32 activation exists before it is rounded
          const T g = Elem<T>::from_f32(a);
          const float u = __fmul_rn(acc[mi][(rg + 2) * 4 + r], su[r]);
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
      const float s4[4] = {sc[rg].x, sc[rg].y, sc[rg].z, sc[rg].w};
      const uint16_t b4[4] = {(uint16_t)(bi[rg].x & 0xffff), (uint16_t)(bi[rg].x >> 16), (uint16_t)(bi[rg].y & 0xffff), (uint16_t)(bi[rg].y >> 16)};
      uint16_t o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = __fmul_rn(acc[mi][rg * 4 + r], s4[r]);
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

// The padded window: (expert, row tile tm of the bucket [E_loc, R, *], channel tile).  The channel tiles of one (expert, row tile) are
// consecutive work items: on ONE XCD, so that its L2 fetches the tile's token rows once (placed round-robin, the eight XCDs each
// fetched them: 1.6 x the algorithmic bytes, measured with FETCH_SIZE)
template <typename T, int ACT, bool GLU>
__device__ __forceinline__ void w8_padded(const W8Args &p, unsigned char *smem) {
  const int b = xcd_work_item((int)gridDim.x);
  const int tn = b % p.ntn, tm = (b / p.ntn) % p.ntm, e = b / (p.ntn * p.ntm);
  w8_tile<T, ACT, GLU>(p, smem, e, tn, tm * W8_BM, p.R, (long long)e * p.R);
}

template <typename T, int ACT>
__global__ __launch_bounds__(W8_THREADS, 2) void expert_gemm_w8_kernel(const W8Args p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * W8_STAGE];
  w8_padded<T, ACT, false>(p, smem);
}

// SwiGLU gate and up products in one launch: 128 image channels = 64 output channels x 128 rows per workgroup
template <typename T, int ACT>
__global__ __launch_bounds__(W8_THREADS, 2) void expert_gemm_w8_glu_kernel(const W8Args p) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * W8_STAGE];
  w8_padded<T, ACT, true>(p, smem);
}

// ---- the packed dropless layout (dropless.hip: tutel_amd_packed_layout) -------------------------------------------------------------------
// The device tables give the windows: table tile t is rows [tiles[2t+1], +256) of expert tiles[2t], clipped by offsets[e + 1]; a
// 256-row table tile is two 128-row halves of this kernel.  A work item is (table tile, channel tile, half); the grid is the host's
// bound, tiles_bound x 2 x ntn of them (rounded up to a multiple of 16: every XCD gets the same number of blocks), the live ones belong
// to the first *ntiles table tiles.
//
// Order.  The (table tile, channel tile) pairs, channel tile fastest, are cut into eight contiguous chunks, one per XCD (the channel
// tiles of a table tile on ONE XCD: its L2 fetches the token rows once, as above); the blocks of an XCD run the FIRST halves of its chunk,
// then the SECOND halves.  So the two halves of a table tile are work items of the same XCD, and the halves that are not live -- every
// second half when no expert is above 128 rows -- sit at the end of the XCD's queue, where they return at once.  Measured
// (tools/packed_w8_bench.py): with the halves as neighbouring work items instead, live and dead blocks alternate in the
// dispatch order and a launch of 64 x 128 rows took 148 us against the padded kernel's 85 us for the same FETCH_SIZE.
// live_map: the chunks are cut from the LIVE pairs (*ntiles x ntn, uniform per launch: one scalar load), so the live work is spread over
// all eight XCDs; without it they are cut from the bound and the live tiles, which sit at the front of the table, land on the first XCDs.
// A block returns in front of every barrier when its table tile is not live or its half starts at or past the expert's end.
struct W8Tables { const int32_t *off, *tiles, *ntiles; int tiles_bound, live_map; };

template <typename T, int ACT, bool GLU>
__global__ __launch_bounds__(W8_THREADS, 2) void expert_gemm_w8_packed_kernel(const W8Args p, const W8Tables t) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * W8_STAGE];
  const int live = min(__builtin_amdgcn_readfirstlane(*t.ntiles), t.tiles_bound);
  const int pairs = (t.live_map ? live : t.tiles_bound) * p.ntn;   // <= tiles_bound * ntn: the host sized the grid for it
  const int xcd = blockIdx.x & 7, pos = blockIdx.x >> 3;
  const int q = pairs >> 3, r = pairs & 7;
  const int len = q + (xcd < r ? 1 : 0), start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  if (pos >= 2 * len) return;
  const int half = pos >= len ? 1 : 0, it = start + pos - half * len;
  const int tn = it % p.ntn, ti = it / p.ntn;
  if (ti >= live) return;
  const int e = __builtin_amdgcn_readfirstlane(t.tiles[2 * ti]);
  const int m0 = __builtin_amdgcn_readfirstlane(t.tiles[2 * ti + 1]) + half * W8_BM;
  const int rend = __builtin_amdgcn_readfirstlane(t.off[e + 1]);
  if (m0 >= rend) return;
  w8_tile<T, ACT, GLU>(p, smem, e, tn, m0, rend, 0);
}

static bool w8_dtype_ok(int dtype) { return dtype == TUTEL_BF16 || dtype == TUTEL_F16; }
static bool w8_shape_ok(int N, int K) { return N >= 32 && N % 32 == 0 && K >= W8_BK && K % W8_BK == 0; }

extern "C" int tutel_amd_expert_gemm_w8_supported(int dtype, int N, int K) { return w8_dtype_ok(dtype) && w8_shape_ok(N, K) ? 1 : 0; }
// the gate / up image has 2 H channels: H a multiple of 16
extern "C" int tutel_amd_expert_gemm_w8_glu_supported(int dtype, int H, int K) {
  return w8_dtype_ok(dtype) && H >= 16 && H % 16 == 0 && w8_shape_ok(2 * H, K) ? 1 : 0;
}

// what differs between the two entry points on the host: the names in the messages, and the image's channels per output channel
struct W8Entry { const char *name, *bad_n, *small_image; int per_out; };
static const W8Entry W8_PLAIN = {"tutel_amd_expert_gemm_w8", "N must be a multiple of 32", "w_stride_e is smaller than one expert's image (N * K bytes)", 1};
static const W8Entry W8_GLU = {"tutel_amd_expert_gemm_w8_glu", "H must be a multiple of 16",
                               "w_stride_e is smaller than one expert's image (2 * H * K bytes)", 2};

// (the activations last to first: the compiler instantiates the list's kernels from its end, and they keep their order in the code object)
template <typename T, bool GLU> static int w8_launch(const W8Entry &en, const W8Args &a, int act, unsigned grid, hipStream_t st) {
  return dispatch_act<TUTEL_ACT_SILU, TUTEL_ACT_GELU, TUTEL_ACT_RELU, TUTEL_ACT_NONE>(
      act,
      [&](auto ac) {
        if constexpr (GLU) hipLaunchKernelGGL((expert_gemm_w8_glu_kernel<T, decltype(ac)::value>), dim3(grid), dim3(W8_THREADS), 0, st, a);
        else hipLaunchKernelGGL((expert_gemm_w8_kernel<T, decltype(ac)::value>), dim3(grid), dim3(W8_THREADS), 0, st, a);
        TUTEL_CHECK_LAUNCH(en.name);
        return 0;
      },
      [&] { return tutel_notsup(en.name, "the activation must be none, relu, gelu or silu"); });
}

static const W8Entry W8_PLAIN_PK = {"tutel_amd_expert_gemm_w8_packed", "N must be a multiple of 32",
                                    "w_stride_e is smaller than one expert's image (N * K bytes)", 1};
static const W8Entry W8_GLU_PK = {"tutel_amd_expert_gemm_w8_glu_packed", "H must be a multiple of 16",
                                  "w_stride_e is smaller than one expert's image (2 * H * K bytes)", 2};

template <typename T, bool GLU>
static int w8_launch_packed(const W8Entry &en, const W8Args &a, const W8Tables &t, int act, unsigned grid, hipStream_t st) {
  return dispatch_act<TUTEL_ACT_SILU, TUTEL_ACT_GELU, TUTEL_ACT_RELU, TUTEL_ACT_NONE>(
      act,
      [&](auto ac) {
        hipLaunchKernelGGL((expert_gemm_w8_packed_kernel<T, decltype(ac)::value, GLU>), dim3(grid), dim3(W8_THREADS), 0, st, a, t);
        TUTEL_CHECK_LAUNCH(en.name);
        return 0;
      },
      [&] { return tutel_notsup(en.name, "the activation must be none, relu, gelu or silu"); });
}

// TUTEL_AMD_W8_PACKED_MAP=bound: cut the XCD chunks of the packed kernels from the grid, not from the live tile count (A/B runs only)
static int w8_packed_live_map() {
  static const int v = [] {
    const char *s = getenv("TUTEL_AMD_W8_PACKED_MAP");
    return s != nullptr && strcmp(s, "bound") == 0 ? 0 : 1;
  }();
  return v;
}

// The packed entry points: the padded ones' checks (minus the bucket strides the packed layout does not have), every one in front of
// the first HIP call
template <bool GLU>
static int w8_run_packed(const W8Entry &en, const void *A, int lda, const int32_t *a_rows, int T, const void *zero_row, const void *Wq,
                         int64_t w_stride_e, const float *scale, const void *bias, int64_t bias_stride_e, void *D, int ldd, int E,
                         int rows_bound, int N, int K, int dtype, int act, const int32_t *offsets, const int32_t *tiles,
                         const int32_t *ntiles, int tiles_bound, tutel_stream_t stream) {
  TUTEL_REQUIRE(E >= 0 && rows_bound >= 0 && tiles_bound >= 0 && N >= 1 && K >= 1, "%s: bad sizes E=%d rows_bound=%d tiles_bound=%d %s=%d K=%d",
                en.name, E, rows_bound, tiles_bound, GLU ? "H" : "N", N, K);
  if (!w8_dtype_ok(dtype)) return tutel_notsup(en.name, "the activations must be bf16 or fp16");
  if (K % W8_BK != 0) return tutel_notsup(en.name, "K must be a multiple of 64");
  if (N % (32 / en.per_out) != 0) return tutel_notsup(en.name, en.bad_n);
  if (act != TUTEL_ACT_NONE && act != TUTEL_ACT_RELU && act != TUTEL_ACT_GELU && act != TUTEL_ACT_SILU)
    return tutel_notsup(en.name, "the activation must be none, relu, gelu or silu");
  if (lda % 8 != 0 || ldd % 4 != 0 || bias_stride_e % 4 != 0 || w_stride_e % 16 != 0)
    return tutel_notsup(en.name, "rows of A must stay 16-byte aligned (lda % 8), rows of D and bias 8-byte aligned (% 4), w_stride_e % 16");
  const long long NI = (long long)en.per_out * N;   // image channels
  if (w_stride_e < NI * K) return tutel_notsup(en.name, en.small_image);
  const long long ntn = (NI + W8_BN - 1) / W8_BN;
  const long long grid = ((long long)tiles_bound * ntn + 7) / 8 * 16;   // 2 halves x the pairs, a whole number of blocks per XCD
  if (grid > 0x7fffffffLL || NI > 0x7fffffffLL)
    return tutel_notsup(en.name, "the work item count tiles_bound * 2 * ceil(channels / 128) must stay below 2^31");
  if (E == 0 || rows_bound == 0 || tiles_bound == 0) return 0;
  TUTEL_REQUIRE(A && Wq && scale && D && offsets && tiles && ntiles, "%s: null pointer", en.name);
  TUTEL_REQUIRE(((uintptr_t)A % 16) == 0 && ((uintptr_t)Wq % 16) == 0 && ((uintptr_t)scale % 16) == 0 && ((uintptr_t)D % 8) == 0 &&
                    ((uintptr_t)bias % 8) == 0,
                "%s: A, Wq and scale must be 16-byte aligned, D and bias 8-byte aligned", en.name);
  if (a_rows != nullptr)
    TUTEL_REQUIRE(T >= 1 && zero_row != nullptr && ((uintptr_t)zero_row % 16) == 0,
                  "%s: a slot map needs T >= 1 and a 16-byte aligned zero row", en.name);

  W8Args a;
  a.A = (const unsigned char *)A; a.a_stride_e = 0; a.lda = lda;
  a.Wq = (const unsigned char *)Wq; a.w_stride_e = w_stride_e;
  a.scale = scale;
  a.bias = (const uint16_t *)bias; a.bias_stride_e = bias_stride_e;
  a.D = (uint16_t *)D; a.d_stride_e = 0; a.ldd = ldd;
  a.R = rows_bound; a.N = (int)NI; a.K = K; a.ntm = 0; a.ntn = (int)ntn;
  a.slot_map = a_rows; a.T = T; a.zero_row = (const unsigned char *)zero_row;
  const W8Tables t = {offsets, tiles, ntiles, tiles_bound, w8_packed_live_map()};
  hipStream_t st = (hipStream_t)stream;
  StageScope stage(GLU || act != TUTEL_ACT_NONE ? TUTEL_STAGE_FC1 : TUTEL_STAGE_FC2, st);
  return dtype == TUTEL_BF16 ? w8_launch_packed<bf16_t, GLU>(en, a, t, act, (unsigned)grid, st)
                             : w8_launch_packed<f16_t, GLU>(en, a, t, act, (unsigned)grid, st);
}

// Both entry points: N output channels per row of D, en.per_out * N image channels.  Every check stands in front of the first HIP call
template <bool GLU>
static int w8_run(const W8Entry &en, const void *A, int64_t a_stride_e, int64_t a_stride_w, int a_rows_per_w, int lda, const void *Wq,
                  int64_t w_stride_e, const float *scale, const void *bias, int64_t bias_stride_e, void *D, int64_t d_stride_e,
                  int64_t d_stride_w, int d_rows_per_w, int ldd, int E_loc, int R, int N, int K, int dtype, int act,
                  const int32_t *row_counts, const int32_t *slot_map, int T, const void *zero_row, tutel_stream_t stream) {
  TUTEL_REQUIRE(E_loc >= 0 && R >= 0 && N >= 1 && K >= 1, "%s: bad sizes E_loc=%d R=%d %s=%d K=%d", en.name, E_loc, R, GLU ? "H" : "N", N, K);
  if (!w8_dtype_ok(dtype)) return tutel_notsup(en.name, "the activations must be bf16 or fp16");
  if (K % W8_BK != 0) return tutel_notsup(en.name, "K must be a multiple of 64");
  if (N % (32 / en.per_out) != 0) return tutel_notsup(en.name, en.bad_n);
  if (act != TUTEL_ACT_NONE && act != TUTEL_ACT_RELU && act != TUTEL_ACT_GELU && act != TUTEL_ACT_SILU)
    return tutel_notsup(en.name, "the activation must be none, relu, gelu or silu");
  if (row_counts != nullptr) return tutel_notsup(en.name, "row_counts (megablocks) are not covered");
  if ((slot_map == nullptr && (a_rows_per_w < R || a_stride_w != 0)) || d_rows_per_w < R || d_stride_w != 0)
    return tutel_notsup(en.name, "the [W, E_loc, C, *] exchange layouts are not covered (rows_per_w >= R and stride_w == 0)");
  if (lda % 8 != 0 || ldd % 4 != 0 || a_stride_e % 8 != 0 || d_stride_e % 4 != 0 || bias_stride_e % 4 != 0 || w_stride_e % 16 != 0)
    return tutel_notsup(en.name, "rows of A must stay 16-byte aligned (lda, a_stride_e % 8), rows of D and bias 8-byte aligned (% 4), w_stride_e % 16");
  const long long NI = (long long)en.per_out * N;   // image channels
  if (w_stride_e < NI * K) return tutel_notsup(en.name, en.small_image);
  const long long ntm = (R + W8_BM - 1) / W8_BM, ntn = (NI + W8_BN - 1) / W8_BN;
  if ((long long)E_loc * R > 0x7fffffffLL || (long long)E_loc * ntm * ntn > 0x7fffffffLL || NI > 0x7fffffffLL)
    return tutel_notsup(en.name, "E_loc * R and the tile count must stay below 2^31");
  if (E_loc == 0 || R == 0) return 0;
  TUTEL_REQUIRE(A && Wq && scale && D, "%s: null pointer", en.name);
  TUTEL_REQUIRE(((uintptr_t)A % 16) == 0 && ((uintptr_t)Wq % 16) == 0 && ((uintptr_t)scale % 16) == 0 && ((uintptr_t)D % 8) == 0 &&
                    ((uintptr_t)bias % 8) == 0,
                "%s: A, Wq and scale must be 16-byte aligned, D and bias 8-byte aligned", en.name);
  if (slot_map != nullptr)
    TUTEL_REQUIRE(T >= 1 && zero_row != nullptr && ((uintptr_t)zero_row % 16) == 0,
                  "%s: a slot map needs T >= 1 and a 16-byte aligned zero row", en.name);

  W8Args a;
  a.A = (const unsigned char *)A; a.a_stride_e = a_stride_e; a.lda = lda;
  a.Wq = (const unsigned char *)Wq; a.w_stride_e = w_stride_e;
  a.scale = scale;
  a.bias = (const uint16_t *)bias; a.bias_stride_e = bias_stride_e;
  a.D = (uint16_t *)D; a.d_stride_e = d_stride_e; a.ldd = ldd;
  a.R = R; a.N = (int)NI; a.K = K; a.ntm = (int)ntm; a.ntn = (int)ntn;
  a.slot_map = slot_map; a.T = T; a.zero_row = (const unsigned char *)zero_row;
  hipStream_t st = (hipStream_t)stream;
  StageScope stage(GLU || act != TUTEL_ACT_NONE ? TUTEL_STAGE_FC1 : TUTEL_STAGE_FC2, st);
  const unsigned grid = (unsigned)((long long)E_loc * ntm * ntn);
  return dtype == TUTEL_BF16 ? w8_launch<bf16_t, GLU>(en, a, act, grid, st) : w8_launch<f16_t, GLU>(en, a, act, grid, st);
}

extern "C" int tutel_amd_expert_gemm_w8(const void *A, int64_t a_stride_e, int64_t a_stride_w, int a_rows_per_w, int lda, const void *Wq,
                                        int64_t w_stride_e, const float *scale, const void *bias, int64_t bias_stride_e, void *D,
                                        int64_t d_stride_e, int64_t d_stride_w, int d_rows_per_w, int ldd, int E_loc, int R, int N, int K,
                                        int dtype, int act, const int32_t *row_counts, const int32_t *slot_map, int T,
                                        const void *zero_row, tutel_stream_t stream) {
  return w8_run<false>(W8_PLAIN, A, a_stride_e, a_stride_w, a_rows_per_w, lda, Wq, w_stride_e, scale, bias, bias_stride_e, D, d_stride_e,
                       d_stride_w, d_rows_per_w, ldd, E_loc, R, N, K, dtype, act, row_counts, slot_map, T, zero_row, stream);
}

// SwiGLU gate and up products of FP8 weights in one launch (the contract: include/tutel_amd.h).  No bias: these experts have none
extern "C" int tutel_amd_expert_gemm_w8_glu(const void *A, int64_t a_stride_e, int64_t a_stride_w, int a_rows_per_w, int lda,
                                            const void *Wq_gu, int64_t w_stride_e, const float *scale_gu, void *D, int64_t d_stride_e,
                                            int64_t d_stride_w, int d_rows_per_w, int ldd, int E_loc, int R, int H, int K, int dtype, int act,
                                            const int32_t *row_counts, const int32_t *slot_map, int T, const void *zero_row,
                                            tutel_stream_t stream) {
  return w8_run<true>(W8_GLU, A, a_stride_e, a_stride_w, a_rows_per_w, lda, Wq_gu, w_stride_e, scale_gu, nullptr, 0, D, d_stride_e,
                      d_stride_w, d_rows_per_w, ldd, E_loc, R, H, K, dtype, act, row_counts, slot_map, T, zero_row, stream);
}


// The two GEMMs above over the packed dropless layout (the contract: include/tutel_amd.h): the row ranges come from the device tables
extern "C" int tutel_amd_expert_gemm_w8_packed(const void *A, int lda, const int32_t *a_rows, int T, const void *zero_row, const void *Wq,
                                               int64_t w_stride_e, const float *scale, const void *bias, int64_t bias_stride_e, void *D,
                                               int ldd, int E, int rows_bound, int N, int K, int dtype, int act, const int32_t *offsets,
                                               const int32_t *tiles, const int32_t *ntiles, int tiles_bound, tutel_stream_t stream) {
  return w8_run_packed<false>(W8_PLAIN_PK, A, lda, a_rows, T, zero_row, Wq, w_stride_e, scale, bias, bias_stride_e, D, ldd, E, rows_bound, N,
                              K, dtype, act, offsets, tiles, ntiles, tiles_bound, stream);
}

extern "C" int tutel_amd_expert_gemm_w8_glu_packed(const void *A, int lda, const int32_t *a_rows, int T, const void *zero_row,
                                                   const void *Wq_gu, int64_t w_stride_e, const float *scale_gu, void *D, int ldd, int E,
                                                   int rows_bound, int H, int K, int dtype, int act, const int32_t *offsets,
                                                   const int32_t *tiles, const int32_t *ntiles, int tiles_bound, tutel_stream_t stream) {
  return w8_run_packed<true>(W8_GLU_PK, A, lda, a_rows, T, zero_row, Wq_gu, w_stride_e, scale_gu, nullptr, 0, D, ldd, E, rows_bound, H, K,
                             dtype, act, offsets, tiles, ntiles, tiles_bound, stream);
}
