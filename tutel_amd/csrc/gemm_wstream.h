// gemm_wstream.h -- the weight-streaming tile of the quantised-weight expert GEMMs (expert_gemm_w8.hip: W8A16, expert_gemm_w4.hip: W4A16),
// its packed work-item mapping and the host path of their entry points, each written ONCE over a weight-format policy.
//
// The launch is a weight-streaming problem (<= 128 rows per expert: every weight byte is used once), so the shape of the kernel follows
// the bytes:
//   * the weight image is the kernel's own layout (include/tutel_amd.h), blocked by (32 channels, K-tile of 64, lane): a lane's loads of
//     one K-tile are contiguous per wave, and a wave walks its 32 channels' whole K extent as one contiguous run.  Weight bytes go
//     global -> VGPR -> convert -> MFMA operand and never touch LDS; a register ring keeps WS_DEPTH K-tiles in flight;
//   * one 4-wave workgroup per (expert, 128 rows, 128 image channels): wave w owns channels 32 w .. 32 w + 31 of the tile and all its
//     rows (one accumulator of 32 x 32 per 32-row group; groups past the window's end are skipped);
//   * token rows go through LDS, K-tiles of 64 in two stages, in the swizzled 128-byte-row panel of the other GEMMs (16-byte chunk c of
//     row r at c ^ ((r >> 1) & 7)): 16-byte global loads into registers, issued two tiles ahead, stored after the previous tile's matrix
//     instructions, one barrier per K-tile.  Rows: the plain [E_loc, R, K] form, or gathered from the tokens through the slot map
//     (negative slot: the zero row);
//   * weights are the A operand of the matrix instruction and token rows the B operand: a lane ends with ONE row and, per register
//     group, 4 consecutive channels -- 8-byte stores, scale and bias as 4-vectors fetched once per lane in front of the epilogue;
//   * R > 128 runs as several row tiles that each stream the weights again: correct, not the design point;
//   * ragged tiles: rows past the window's end and channel groups past N clamp their loads (to the last row / the last 32-channel
//     group) and mask their stores; nothing is read or written outside the operands.
//
// SwiGLU experts (GLU): the image holds both matrices, interleaved by 16 channels (experts/w8.py::interleave_gate_up): in every
// 32-channel group positions 0 .. 15 are gate channels 16 g .. 16 g + 15 and positions 16 .. 31 the up channels of the same indices.
// A lane's accumulator registers rg = 0, 1 are then gate channels and rg + 2 the up channels of the SAME outputs, so the gating product
// is register against register: the same K loop over 2 H image channels, token rows read once, the gate never written to memory, no
// LDS and no cross-lane move in the epilogue.  One workgroup is 128 image channels = 64 output channels x 128 rows.
//
// What a format supplies (struct Fmt; W8Fmt and W4Fmt in the two .hip files):
//   Fmt::Args            the kernel argument struct: the fields ws_tile reads below plus the format's own weight operands
//   Fmt::Ring<T>         the per-lane ring of K-tiles and its buffer descriptors: open(p, e, nt, lane), load(d, t) -- K-tile t into
//                        slot d, the prime and the refill alike -- and widen(d, wa): slot d as the four 8-element operands
//   Fmt::Scale           the epilogue's per-channel scale: fetch(p, e, n, rg) and apply(acc, rg, r)
//   Fmt::Weights, TEXT, packed_halves(), launch<T, ACT, GLU>()      the host side, see ws_run
#pragma once
#include "gemm_dev.h"  // Mma<T>, activate<ACT>

#define WS_BM 128
#define WS_BN 128
#define WS_BK 64
#define WS_THREADS 256
#define WS_DEPTH 4       // K-tiles of weights in flight per wave (even: the token registers alternate with it); 8 measured the same
#define WS_STAGE (WS_BM * WS_BK * 2)   // one stage of the 128-row token panel

// The K loop of ws_tile for NMI live 32-row groups (the dead groups' accumulators stay zero and their stores are masked); NMI = 0: the
// loop that is not specialised and tests each group against nmi
template <typename Fmt, typename T, int MG, int NMI>
__device__ __forceinline__ void ws_kloop(typename Fmt::template Ring<T> &ring, f32x16 (&acc)[MG], u32x4 (&treg)[2][MG],
                                         const unsigned char *const (&rowp)[MG], const int (&ldst)[MG], unsigned char *smem, const int nk,
                                         const int nmi, const int kg, const int sw, const int frag) {
  constexpr int STAGE = MG * 32 * WS_BK * 2;   // one stage of the token panel
  constexpr int NP = NMI <= 4 ? 4 : MG;   // token passes per K-tile; NF fragments per operand (the 128-row loop reads all four)
  constexpr int NF = NMI <= 4 ? 4 : NMI;
  for (int kt0 = 0; kt0 < nk; kt0 += WS_DEPTH) {
#pragma unroll
    for (int d = 0; d < WS_DEPTH; ++d) {
      const int kt = kt0 + d;   // kt & 1 == d & 1: kt0 is a multiple of the even ring depth
      if (kt >= nk) break;  // block-uniform
      // token tile kt + 2 (behind the last tile: that tile again -- it is stored into the free stage and never read)
      const long long tnext = (long long)min(kt + 2, nk - 1) * (WS_BK * 2);
#pragma unroll
      for (int i = 0; i < NP; ++i) treg[d & 1][i] = *reinterpret_cast<const u32x4 *>(rowp[i] + tnext);
      // the K-tile's four operands of 8 k: operand q holds k = 64 kt + 16 q + 8 kg .. + 7; then the slot's refill
      u32x4 wa[4];
      ring.widen(d, wa);
      ring.load(d, kt + WS_DEPTH);
      // operand q multiplies token chunk 2 q + kg of every row; the fragments of operand q + 1 are asked for before the matrix
      // instructions of operand q (two sets of NF in registers, not all of them)
      const unsigned char *st = smem + (kt & 1) * STAGE + frag;
      u32x4 tb[2][NF];
#pragma unroll
      for (int mi = 0; mi < NF; ++mi) tb[0][mi] = *reinterpret_cast<const u32x4 *>(st + mi * (32 * 128) + ((kg ^ sw) << 4));
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q < 3) {
#pragma unroll
          for (int mi = 0; mi < NF; ++mi)
            tb[(q + 1) & 1][mi] = *reinterpret_cast<const u32x4 *>(st + mi * (32 * 128) + (((2 * (q + 1) + kg) ^ sw) << 4));
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int mi = 0; mi < NF; ++mi)
          if (NMI != 0 ? mi < NMI : mi < nmi) acc[mi] = Mma<T>::run(wa[q], tb[q & 1][mi], acc[mi]);
        __builtin_amdgcn_sched_barrier(0);
      }
      {  // the other stage is free since the last barrier (behind the last tile nobody reads what is stored)
        unsigned char *nx = smem + ((kt + 1) & 1) * STAGE;
#pragma unroll
        for (int i = 0; i < NP; ++i) *reinterpret_cast<u32x4 *>(nx + ldst[i]) = treg[(d + 1) & 1][i];
      }
      __syncthreads();
    }
  }
}

// One (expert, 32 MG rows, 128 image channels) work item; every kernel of the two files is this function.  GLU: p.N = 2 H image channels,
// and only the epilogue differs.
//
// The work item is a ROW WINDOW: expert e (its weights, scale and bias), rows [m0, min(m0 + 32 MG, rend)) and channel tile tn.  Rows are
// numbered as the caller's layout numbers them -- within the expert's bucket for the padded kernels (row r of A at e * a_stride_e +
// r * lda, its slot at slot0 + r with slot0 = e * R), absolute packed rows for the packed ones (a_stride_e = d_stride_e = 0, slot0 = 0,
// rend = offsets[e + 1]: the rows from rend on are the NEXT expert's and are neither read nor written).
//   MG = 4: the 128-row tile of the padded kernels and of the packed kernels' halves form.
//   MG = 8: the WIDE window, a whole 256-row table tile.  Each operand of 8 k is widened ONCE and issued against up to eight 32-row
//           groups.  Live-group counts 1 .. 4 run the 128-row loop itself (four token passes, four fragments: rows 128 .. 255 of the
//           panel are neither written nor read); counts 5 .. 8 move eight token passes per K-tile into the 256-row panel (two stages of
//           32 KB) and read exactly the live groups' fragments.
//   SPEC:   the K loop is compiled once per live-group count (straight-line matrix instructions, no branch around any of them) and
//           chosen by a switch; without it ONE loop tests `group < live count` at run time (MG = 4 only).
// Whatever the format, MG, SPEC and the count: one fp32 accumulator per output, K ascending, the same widen, the same epilogue -- the
// same bits.
template <typename Fmt, typename T, int ACT, bool GLU, int MG, bool SPEC>
__device__ __forceinline__ void ws_tile(const typename Fmt::Args &p, unsigned char *smem, const int e, const int tn, const int m0,
                                        const int rend, const long long slot0) {
  static_assert(SPEC || MG == 4, "the wide window needs the specialised K loop");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, kg = lane >> 5;
  const int n0 = tn * WS_BN;
  const int nk = p.K / WS_BK;
  const int NT = p.N >> 5;
  const int nmi = min(MG, (rend - m0 + 31) >> 5);  // live 32-row groups of this tile
  const bool wide = MG > 4 && nmi > 4;             // (block-uniform) the token passes 4 .. MG - 1 are live

  // ---- token rows: thread `tid` moves chunk (tid & 7) of rows 32 i + (tid >> 3), i < MG, of every K-tile ------------------------------
  const unsigned char *rowp[MG];
  int ldst[MG];
  {
    int slot[MG];
#pragma unroll
    for (int i = 0; i < MG; ++i) slot[i] = 0;
    if (p.slot_map != nullptr) {  // the slots first, so that their loads are in flight together
#pragma unroll
      for (int i = 0; i < MG; ++i) slot[i] = p.slot_map[slot0 + min(m0 + 32 * i + (tid >> 3), rend - 1)];
    }
#pragma unroll
    for (int i = 0; i < MG; ++i) {
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
  // The group's run is read through buffer descriptors of exactly its size: every load of the K loop is UNCONDITIONAL (a load under a
  // branch makes the compiler wait for all loads in flight where the branches join), and the refills past the last K-tile are out of
  // the descriptors' range -- they fetch nothing and return zeros that are never used.
  typename Fmt::template Ring<T> ring;
  ring.open(p, e, nt, lane);
#pragma unroll
  for (int d = 0; d < WS_DEPTH; ++d) ring.load(d, d);

  f32x16 acc[MG];
#pragma unroll
  for (int mi = 0; mi < MG; ++mi)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mi][r] = 0.f;

  // Token rows run TWO tiles ahead in registers (treg[j]: a tile of parity j): the memory counter retires loads in order, so waiting
  // for a token tile asked for only one step ago would also wait for every weight refill issued before it -- the ring would be one
  // tile deep whatever WS_DEPTH says.  Tile 0 goes to LDS here, tile 1 waits in treg[1]
  u32x4 treg[2][MG];
#pragma unroll
  for (int i = 0; i < MG; ++i)
    if (i < 4 || wide) treg[0][i] = *reinterpret_cast<const u32x4 *>(rowp[i]);
#pragma unroll
  for (int i = 0; i < MG; ++i)
    if (i < 4 || wide) treg[1][i] = *reinterpret_cast<const u32x4 *>(rowp[i] + (long long)min(1, nk - 1) * (WS_BK * 2));
#pragma unroll
  for (int i = 0; i < MG; ++i)
    if (i < 4 || wide) *reinterpret_cast<u32x4 *>(smem + ldst[i]) = treg[0][i];
  __syncthreads();

  const int sw = (l31 >> 1) & 7;
  const int frag = l31 * 128;  // + mi * 32 rows

  // (the specialised loops are reached through a lambda and the unspecialised one is not: with these two call forms the compiler
  // schedules each format's K-tile and epilogue as it did when each file had its own tile)
  auto kloop = [&](auto nmi_c) __attribute__((always_inline)) {
    ws_kloop<Fmt, T, MG, decltype(nmi_c)::value>(ring, acc, treg, rowp, ldst, smem, nk, nmi, kg, sw, frag);
  };
  if constexpr (!SPEC) {
    ws_kloop<Fmt, T, MG, 0>(ring, acc, treg, rowp, ldst, smem, nk, nmi, kg, sw, frag);
  } else {
    switch (nmi) {
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
  }

  // ---- epilogue: lane = row m0 + 32 mi + l31; register 4 rg + r of accumulator mi = channel 32 nt + 8 rg + 4 kg + r ---------------------
  if (!wave_live) return;
  // scale and bias of the lane's channels 32 nt + 8 rg + 4 kg .. + 3, all fetched before the first is used
  typename Fmt::Scale sc;
  uint2 bi[4];
#pragma unroll
  for (int rg = 0; rg < 4; ++rg) {
    const int n = nt * 32 + rg * 8 + kg * 4;
    sc.fetch(p, e, n, rg);
    if constexpr (!GLU)
      bi[rg] = p.bias != nullptr ? *reinterpret_cast<const uint2 *>(p.bias + (long long)e * p.bias_stride_e + n) : make_uint2(0u, 0u);
  }
  if constexpr (GLU) {
    // Registers rg = 0, 1 are gate channels 16 nt + 8 rg + 4 kg + r of the expert, registers rg + 2 the up channels of the same
    // indices (the image's interleave): the gating product is register against register in this lane.  g = act(gacc * scale_gate)
    // rounded to T, u = uacc * scale_up, D = round_T(float(g) * u) -- tutel_amd_expert_gemm_gate_up's order; no bias
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
          float a = activate<ACT>(sc.apply(acc[mi][rg * 4 + r], rg, r));
          asm("" : "+v"(a));  // the fp32 activation exists before it is rounded
          const T g = Elem<T>::from_f32(a);
          const float u = sc.apply(acc[mi][(rg + 2) * 4 + r], rg + 2, r);
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
        float v = sc.apply(acc[mi][rg * 4 + r], rg, r);
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
template <typename Fmt, typename T, int ACT, bool GLU, bool SPEC>
__device__ __forceinline__ void ws_padded(const typename Fmt::Args &p, unsigned char *smem) {
  const int b = xcd_work_item((int)gridDim.x);
  const int tn = b % p.ntn, tm = (b / p.ntn) % p.ntm, e = b / (p.ntn * p.ntm);
  ws_tile<Fmt, T, ACT, GLU, 4, SPEC>(p, smem, e, tn, tm * WS_BM, p.R, (long long)e * p.R);
}

// ---- the packed dropless layout (dropless.hip: tutel_amd_packed_layout) -------------------------------------------------------------------
// The device tables give the windows: table tile t is rows [tiles[2t+1], +256) of expert tiles[2t], clipped by offsets[e + 1].  The grid
// is the host's bound (ws_run), the live work items belong to the first *ntiles table tiles.  Two forms compute a table tile:
//   HALVES (MG = 4): a work item is (table tile, channel tile, half), a 128-row half of the table tile; two workgroups per CU.
//   WIDE (MG = 8):   a work item is (table tile, channel tile) and owns ALL live rows of the window, so an expert above 128 rows
//                    streams its weights and runs its converts once.
//
// Order.  The (table tile, channel tile) pairs, channel tile fastest, are cut into eight contiguous chunks, one per XCD (the channel
// tiles of a table tile on ONE XCD: its L2 fetches the token rows once, as above); the blocks of an XCD run the FIRST halves of its chunk,
// then the SECOND halves.  So the two halves of a table tile are work items of the same XCD, and the halves that are not live -- every
// second half when no expert is above 128 rows -- sit at the end of the XCD's queue, where they return at once.  Measured
// (tools/packed_w8_bench.py): with the halves as neighbouring work items instead, live and dead blocks alternate in the
// dispatch order and a launch of 64 x 128 rows took 148 us against the padded kernel's 85 us for the same FETCH_SIZE.
// live_map: the chunks are cut from the LIVE pairs (*ntiles x ntn, uniform per launch: one scalar load), so the live work is spread over
// all eight XCDs; without it they are cut from the bound and the live tiles, which sit at the front of the table, land on the first XCDs.
// -> this block's window, run; nothing when it has none: its position is past its XCD's chunk, its table tile is not live, or its half
// starts at or past the expert's end -- every return stands in front of the first barrier.  MG = 4: halves, MG = 8: wide
template <typename Fmt, typename T, int ACT, bool GLU, int MG, bool SPEC>
__device__ __forceinline__ void ws_packed(const typename Fmt::Args &p, const int32_t *off, const int32_t *tiles, const int32_t *ntiles,
                                          int tiles_bound, int live_map, unsigned char *smem) {
  constexpr int NH = 8 / MG;   // work items per pair
  const int live = min(__builtin_amdgcn_readfirstlane(*ntiles), tiles_bound);
  const int pairs = (live_map ? live : tiles_bound) * p.ntn;   // <= tiles_bound * ntn: the host sized the grid for it
  const int xcd = blockIdx.x & 7, pos = blockIdx.x >> 3;
  const int q = pairs >> 3, r = pairs & 7;
  const int len = q + (xcd < r ? 1 : 0), start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  if (pos >= NH * len) return;
  const int half = pos >= len ? 1 : 0, it = start + pos - half * len;
  const int tn = it % p.ntn, ti = it / p.ntn;
  if (ti >= live) return;
  const int e = __builtin_amdgcn_readfirstlane(tiles[2 * ti]);
  const int m0 = __builtin_amdgcn_readfirstlane(tiles[2 * ti + 1]) + half * WS_BM;
  const int rend = __builtin_amdgcn_readfirstlane(off[e + 1]);
  if (m0 >= rend) return;
  ws_tile<Fmt, T, ACT, GLU, MG, SPEC>(p, smem, e, tn, m0, rend, 0);
}

// ws_packed's mapping alone, always cut from the live pairs, for a kernel whose tile is not ws_tile (expert_gemm_w4a8.hip): NH work items
// per pair (2: halves, 1: wide), ntn channel tiles -> false where this block has no window.  (ws_packed keeps its own copy: routed
// through this function the W8A16 and W4A16 packed kernels compile to different code, and those kernels are measured as they are)
struct WsWindow { int e, tn, m0, rend; };   // expert, channel tile, rows [m0, rend): the tile clips them to its form's extent

template <int NH>
__device__ __forceinline__ bool ws_packed_window(int ntn, const int32_t *off, const int32_t *tiles, const int32_t *ntiles, int tiles_bound,
                                                 WsWindow &w) {
  const int live = min(__builtin_amdgcn_readfirstlane(*ntiles), tiles_bound);
  const int pairs = live * ntn;   // <= tiles_bound * ntn: the host sized the grid for it
  const int xcd = blockIdx.x & 7, pos = blockIdx.x >> 3;
  const int q = pairs >> 3, r = pairs & 7;
  const int len = q + (xcd < r ? 1 : 0), start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  if (pos >= NH * len) return false;
  const int half = pos >= len ? 1 : 0, it = start + pos - half * len;
  const int ti = it / ntn;
  w.tn = it % ntn;
  if (ti >= live) return false;
  w.e = __builtin_amdgcn_readfirstlane(tiles[2 * ti]);
  w.m0 = __builtin_amdgcn_readfirstlane(tiles[2 * ti + 1]) + half * WS_BM;
  w.rend = __builtin_amdgcn_readfirstlane(off[w.e + 1]);
  return w.m0 < w.rend;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
static bool ws_dtype_ok(int dtype) { return dtype == TUTEL_BF16 || dtype == TUTEL_F16; }
static bool ws_shape_ok(int N, int K) { return N >= 32 && N % 32 == 0 && K >= WS_BK && K % WS_BK == 0; }
static int ws_supported(int dtype, int N, int K) { return ws_dtype_ok(dtype) && ws_shape_ok(N, K) ? 1 : 0; }
// the gate / up image has 2 H channels: H a multiple of 16
static int ws_glu_supported(int dtype, int H, int K) { return ws_dtype_ok(dtype) && H >= 16 && H % 16 == 0 && ws_shape_ok(2 * H, K) ? 1 : 0; }

// what differs between the entry points of one format: the name in the messages and the image-size refusal
struct WsEntry { const char *name, *small_image; };
// a format's refusals that name its weight operands; [0] the padded entry points', [1] the packed ones'
struct WsText { const char *strides[2], *limit[2], *aligned; };
// where the rows are: the bucket [E_loc, R, *] of the padded entry points, or the packed layout's device tables
struct WsBucket { int64_t a_stride_e, a_stride_w; int a_rows_per_w; int64_t d_stride_e, d_stride_w; int d_rows_per_w; const int32_t *row_counts; };
struct WsTables { const int32_t *offsets, *tiles, *ntiles; int tiles_bound; };

// Every entry point of the two files: N output channels per row of D, (GLU ? 2 : 1) * N image channels; exactly one of bk (padded: E
// experts of R rows) and pk (packed: R = rows_bound) is given.  Every check stands in front of the first HIP call, a refusal in front of
// the empty-problem return.  The format's part:
//   Fmt::Weights   the weight operands as the entry point got them: strides_ok(), image_ok(image channels, K), run_ok(K) -- the 2^31
//                  limit of one channel group's run --, present(), aligned() and fill(args)
//   Fmt::TEXT      the messages of those checks
//   Fmt::packed_halves(), Fmt::launch<T, ACT, GLU>(args, pk, halves, grid, stream)      the packed form and the kernel launch
// (the activations last to first: the compiler instantiates the list's kernels from its end, and they keep their order in the code object)
template <typename Fmt, bool GLU>
static int ws_run(const WsEntry &en, const typename Fmt::Weights &w, const WsBucket *bk, const WsTables *pk, const void *A, int lda,
                  const int32_t *slot_map, int T, const void *zero_row, const void *bias, int64_t bias_stride_e, void *D, int ldd, int E,
                  int R, int N, int K, int dtype, int act, tutel_stream_t stream) {
  const int packed = pk != nullptr ? 1 : 0;
  if (packed)
    TUTEL_REQUIRE(E >= 0 && R >= 0 && pk->tiles_bound >= 0 && N >= 1 && K >= 1, "%s: bad sizes E=%d rows_bound=%d tiles_bound=%d %s=%d K=%d",
                  en.name, E, R, pk->tiles_bound, GLU ? "H" : "N", N, K);
  else
    TUTEL_REQUIRE(E >= 0 && R >= 0 && N >= 1 && K >= 1, "%s: bad sizes E_loc=%d R=%d %s=%d K=%d", en.name, E, R, GLU ? "H" : "N", N, K);
  if (!ws_dtype_ok(dtype)) return tutel_notsup(en.name, "the activations must be bf16 or fp16");
  if (K % WS_BK != 0) return tutel_notsup(en.name, "K must be a multiple of 64");
  if (N % (GLU ? 16 : 32) != 0) return tutel_notsup(en.name, GLU ? "H must be a multiple of 16" : "N must be a multiple of 32");
  if (act != TUTEL_ACT_NONE && act != TUTEL_ACT_RELU && act != TUTEL_ACT_GELU && act != TUTEL_ACT_SILU)
    return tutel_notsup(en.name, "the activation must be none, relu, gelu or silu");
  if (!packed) {   // (the packed layout has no bucket strides)
    if (bk->row_counts != nullptr) return tutel_notsup(en.name, "row_counts (megablocks) are not covered");
    if ((slot_map == nullptr && (bk->a_rows_per_w < R || bk->a_stride_w != 0)) || bk->d_rows_per_w < R || bk->d_stride_w != 0)
      return tutel_notsup(en.name, "the [W, E_loc, C, *] exchange layouts are not covered (rows_per_w >= R and stride_w == 0)");
  }
  const long long a_stride_e = packed ? 0 : bk->a_stride_e, d_stride_e = packed ? 0 : bk->d_stride_e;
  if (lda % 8 != 0 || ldd % 4 != 0 || a_stride_e % 8 != 0 || d_stride_e % 4 != 0 || bias_stride_e % 4 != 0 || !w.strides_ok())
    return tutel_notsup(en.name, Fmt::TEXT.strides[packed]);
  const long long NI = (GLU ? 2LL : 1LL) * N;   // image channels
  if (!w.image_ok(NI, K)) return tutel_notsup(en.name, en.small_image);
  const long long ntm = (R + WS_BM - 1) / WS_BM, ntn = (NI + WS_BN - 1) / WS_BN;
  // packed: a whole number of blocks per XCD; the halves form has two work items per (table tile, channel tile) pair, and the limit
  // is the halves form's whichever form runs
  const bool halves = packed && Fmt::packed_halves();
  const long long per_xcd = packed ? ((long long)pk->tiles_bound * ntn + 7) / 8 : 0;
  const long long grid = packed ? per_xcd * (halves ? 16 : 8) : (long long)E * ntm * ntn;
  if ((packed ? per_xcd * 16 > 0x7fffffffLL : (long long)E * R > 0x7fffffffLL || grid > 0x7fffffffLL) || NI > 0x7fffffffLL ||
      !Fmt::Weights::run_ok(K))
    return tutel_notsup(en.name, Fmt::TEXT.limit[packed]);
  if (E == 0 || R == 0 || (packed && pk->tiles_bound == 0)) return 0;
  if (packed) TUTEL_REQUIRE(A && w.present() && D && pk->offsets && pk->tiles && pk->ntiles, "%s: null pointer", en.name);
  else TUTEL_REQUIRE(A && w.present() && D, "%s: null pointer", en.name);
  TUTEL_REQUIRE(((uintptr_t)A % 16) == 0 && w.aligned() && ((uintptr_t)D % 8) == 0 && ((uintptr_t)bias % 8) == 0, Fmt::TEXT.aligned, en.name);
  if (slot_map != nullptr)
    TUTEL_REQUIRE(T >= 1 && zero_row != nullptr && ((uintptr_t)zero_row % 16) == 0,
                  "%s: a slot map needs T >= 1 and a 16-byte aligned zero row", en.name);

  typename Fmt::Args a;
  a.A = (const unsigned char *)A; a.a_stride_e = a_stride_e; a.lda = lda;
  w.fill(a);
  a.bias = (const uint16_t *)bias; a.bias_stride_e = bias_stride_e;
  a.D = (uint16_t *)D; a.d_stride_e = d_stride_e; a.ldd = ldd;
  a.R = R; a.N = (int)NI; a.K = K; a.ntm = packed ? 0 : (int)ntm; a.ntn = (int)ntn;
  a.slot_map = slot_map; a.T = T; a.zero_row = (const unsigned char *)zero_row;
  hipStream_t st = (hipStream_t)stream;
  StageScope stage(GLU || act != TUTEL_ACT_NONE ? TUTEL_STAGE_FC1 : TUTEL_STAGE_FC2, st);
  return dispatch_act<TUTEL_ACT_SILU, TUTEL_ACT_GELU, TUTEL_ACT_RELU, TUTEL_ACT_NONE>(
      act,
      [&](auto ac) {
        if (dtype == TUTEL_BF16) Fmt::template launch<bf16_t, decltype(ac)::value, GLU>(a, pk, halves, (unsigned)grid, st);
        else Fmt::template launch<f16_t, decltype(ac)::value, GLU>(a, pk, halves, (unsigned)grid, st);
        TUTEL_CHECK_LAUNCH(en.name);
        return 0;
      },
      [&] { return tutel_notsup(en.name, "the activation must be none, relu, gelu or silu"); });
}
