// expert_gemm_f32.hip -- the grouped GEMM of FP32 experts on the exact-f32 matrix instruction of gfx950.
//
//   D[e, r, n] = act( chain(e, r, n) + bias[e, n] )
//   chain(e, r, n) = fmaf(a[K-1], w[K-1], ... fmaf(a[1], w[1], fmaf(a[0], w[0], 0.f)))        a = A[e, r, :], w = column n of op(W[e])
//
// v_mfma_f32_32x32x2_f32 is bit for bit a k-ordered fmaf chain (D = fma(a1, b1, fma(a0, b0, C)), one rounding per product, no wider
// accumulator), so the output of this kernel is a CONTRACT (include/tutel_amd.h), replayable on a CPU: one accumulator per output, k
// ascending from 0 starting at 0.f, no split-K, no rotated K order; then ONE fp32 add of the bias (skipped without a bias) and the
// activation in fp32 with the formulas of gemm_dev.h::activate (the library builds with -ffp-contract=off).  Nothing depends on the
// tile an output falls into, on E_loc, R or the launch.
//
// Shape of the kernel (one form in two tile sizes, no planner):
//   * one 4-wave workgroup per 128 x 128 tile of one expert; wave (wm, wn) owns 64 x 64 as 2 x 2 accumulators of 32 x 32 -- one wave
//     per SIMD with four independent accumulators already reaches the instruction's issue rate (64 cycles each), and at <= 256
//     registers two workgroups share a CU and hide each other's barriers and fragment reads.  Where 128 x 128 tiles are fewer than
//     the compute units (xf_tile), the same code runs 64 x 64 tiles, one accumulator per wave: the chain admits no split-K, so more
//     and smaller tiles are the only parallelism a short problem has (configs[0]'s fc1: 16 tiles of 128 x 128);
//   * K-tiles of 32 through two LDS stages (32 KB each; 16 KB for the small tile), filled by 16-byte LDS-DMA (global_load_lds, 1 KB
//     per wave instruction): tile p + 1 is issued once every wave has asked for its fragments of tile p and lands under the matrix
//     instructions of tile p;
//   * LDS image of a [row][k] operand (the activations; k-major weights, batched_fc1_w): the byte panel of gate_proj.hip -- [128 rows]
//     [128 B], 16-byte chunk c of row r at c ^ ((r >> 1) & 7); the lane picks the global chunk, the LDS side of the DMA is linear.
//     Lanes 0..31 of an instruction carry the even k and lanes 32..63 the odd k: a lane reads whole 16-byte chunks (conflict-free
//     ds_read_b128) and keeps the two words of its parity;
//   * LDS image of n-major weights (batched_fc2_w, [K][N] as stored -- no k-major copy): plain [32 k][128 n], one DMA piece = two k
//     rows of 512 B; the fragment of instruction j is ONE ds_read_b32 per lane at [2 j + parity][n], 32 consecutive words per lane
//     group: conflict-free (the 64 x 64 tile: 64 rows, [32 k][64 n], four k rows of 256 B per piece);
//   * activation rows are the A operand, weights the B operand: a lane ends with ONE column n and 16 rows per accumulator, so the
//     bias is one scalar per lane and tile, and every store instruction writes two full 128-byte row segments;
//   * rows: tutel_amd_expert_gemm's addressing on both sides (the raw all-to-all buffers work), or gathered from the tokens through the
//     slot map (fast_encode fused); ragged last tiles clamp their loads to the last row / column chunk and mask their stores, so
//     nothing is read or written outside the operands;
//   * every address is a 64-bit byte offset from its operand; what is refused instead of wrapped: E_loc * R or the grid past 2^31 - 1.
#include "gemm_dev.h"  // activate<ACT>: the 16-bit GEMMs' activation formulas

#define XF_BM 128
#define XF_BN 128
#define XF_BK 32
#define XF_THREADS 256
#define XF_CUS 256   // compute units of the MI355X: the grid below which the small tile is taken

typedef __attribute__((ext_vector_type(4))) float xf_f32x4;

struct XfArgs {
  const unsigned char *A; long long a_stride_e, a_stride_w; int a_rpw, lda;  // strides and leading dimensions in elements
  const unsigned char *W; long long w_stride_e; int ldw;
  const float *bias; long long bias_stride_e;
  float *D; long long d_stride_e, d_stride_w; int d_rpw, ldd;
  int R, N, K, ntm, ntn;
  const int32_t *slot_map; int T; const unsigned char *zero_row;
};

__device__ __forceinline__ void xf_dma16(const unsigned char *g, unsigned char *l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g, (__attribute__((address_space(3))) void *)l, 16, 0, 0);
}

// WK: 1 = W[e] is [N][K] (k-major), 0 = [K][N].  TT: 32 x 32 accumulators per wave and dimension -- 2: the 128 x 128 tile, 1: 64 x 64
template <int WK, int ACT, int TT>
__global__ __launch_bounds__(XF_THREADS, 2) void expert_gemm_f32_kernel(const XfArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr int BT = 64 * TT;         // rows and columns of the tile
  constexpr int TILE = BT * XF_BK * 4;  // bytes of one operand's K-tile: [BT][32] or [32][BT] fp32
  constexpr int STAGE = 2 * TILE;
  constexpr int PW = 2 * TT;          // DMA pieces (1 KB) per wave, operand and K-tile
  constexpr int RB = BT * 4;          // bytes of a k row of the [k][n] image
  constexpr int LPR = RB / 16;        // lanes of a DMA piece per k row of it
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x;
  const int tn = b % p.ntn, tm = (b / p.ntn) % p.ntm, e = b / (p.ntn * p.ntm);
  const int m0 = tm * BT, n0 = tn * BT;
  const int nk = p.K / XF_BK;

  // ---- DMA sources: wave `wid` fills pieces PW wid .. PW wid + PW - 1 (1 KB each) of both operands' tiles -------------------------
  const unsigned char *as[PW], *ws[PW];
  const long long w_step = WK ? (long long)XF_BK * 4 : (long long)XF_BK * p.ldw * 4;
  int slot[PW];
#pragma unroll
  for (int i = 0; i < PW; ++i) slot[i] = 0;
  if (p.slot_map != nullptr) {  // the slots first, so that their loads are in flight together
#pragma unroll
    for (int i = 0; i < PW; ++i) slot[i] = p.slot_map[(long long)e * p.R + min(m0 + 8 * (wid * PW + i) + (lane >> 3), p.R - 1)];
  }
#pragma unroll
  for (int i = 0; i < PW; ++i) {
    const int q = wid * PW + i;
    {  // piece q of a [row][k] tile: rows 8 q .. 8 q + 7, the lane's LDS chunk (lane & 7) holds global chunk (lane & 7) ^ swizzle(row)
      const int r = 8 * q + (lane >> 3);
      const int c = (lane & 7) ^ ((r >> 1) & 7);
      const int gr = min(m0 + r, p.R - 1);
      const unsigned char *row;
      if (p.slot_map != nullptr) {
        row = slot[i] < 0 ? p.zero_row : p.A + (long long)(slot[i] % p.T) * p.lda * 4;
      } else {
        int qw = 0, rw = gr;
        if (p.a_rpw < p.R) { qw = gr / p.a_rpw; rw = gr - qw * p.a_rpw; }
        row = p.A + ((long long)e * p.a_stride_e + (long long)qw * p.a_stride_w + (long long)rw * p.lda) * 4;
      }
      as[i] = row + c * 16;
      if (WK) {
        const int gn = min(n0 + r, p.N - 1);
        ws[i] = p.W + ((long long)e * p.w_stride_e + (long long)gn * p.ldw) * 4 + c * 16;
      }
    }
    if (!WK) {  // piece q of the [k][n] tile: 64 / LPR whole k rows, the lane's 16 bytes are columns 4 (lane % LPR) .. + 3 of its row
      const int kr = q * (64 / LPR) + lane / LPR;
      const int gn = min(n0 + 4 * (lane % LPR), p.N - 4);
      ws[i] = p.W + ((long long)e * p.w_stride_e + (long long)kr * p.ldw + gn) * 4;
    }
  }
#define XF_ISSUE(P)                                                                                                    \
  do {                                                                                                                 \
    unsigned char *st_ = smem + ((P) & 1) * STAGE;                                                                     \
    _Pragma("unroll") for (int i = 0; i < PW; ++i) xf_dma16(as[i] + (long long)(P) * (XF_BK * 4), st_ + (wid * PW + i) * 1024);          \
    _Pragma("unroll") for (int i = 0; i < PW; ++i) xf_dma16(ws[i] + (long long)(P) * w_step, st_ + TILE + (wid * PW + i) * 1024);        \
  } while (0)
  XF_ISSUE(0);

  const int wm = wid & 1, wn = wid >> 1;
  const int l31 = lane & 31, kg = lane >> 5;
  const int sw = (l31 >> 1) & 7;
  const int a_row = (wm * 32 * TT + l31) * 128;                                                    // + mt * 32 rows
  const int w_row = TILE + (WK ? (wn * 32 * TT + l31) * 128 : kg * RB + (wn * 32 * TT + l31) * 4);  // + nt * 32 rows / columns

  // the lane's bias scalars, fetched before the K loop (clamped, branch-free) and USED here: the compiler then waits for them
  // once, beside the first tile's DMA.  Left to the epilogue, it would put a vmcnt(0) -- which also drains every earlier store -- in
  // front of each of the masked stores
  float bv[TT];
#pragma unroll
  for (int nt = 0; nt < TT; ++nt) {
    bv[nt] = 0.f;
    if (p.bias != nullptr) bv[nt] = p.bias[(long long)e * p.bias_stride_e + min(n0 + wn * 32 * TT + nt * 32 + l31, p.N - 1)];
  }
#pragma unroll
  for (int nt = 0; nt < TT; ++nt) asm volatile("" : "+v"(bv[nt]));

  f32x16 acc[TT][TT];
#pragma unroll
  for (int mt = 0; mt < TT; ++mt)
#pragma unroll
    for (int nt = 0; nt < TT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

  for (int kt = 0; kt < nk; ++kt) {
    // this wave's pieces of tile kt have landed and its fragment reads of tile kt - 1 are back; after the barrier every wave's have,
    // so tile kt is whole and the other stage is free
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    const unsigned char *st = smem + (kt & 1) * STAGE;
    // The whole K-tile's fragments (8 chunks per row: 16 instructions per accumulator) are asked for at once and the matrix
    // instructions start as the first chunks arrive (counted lgkmcnt waits): 2 - 3 % faster, measured, than reading and multiplying
    // half a tile at a time, and still under 256 registers (231 / 200 for the 128 x 128 tile, k-major / n-major)
    xf_f32x4 fa[TT][8];  // chunk cc: k = 4 cc .. + 3
    xf_f32x4 fw[TT][8];  // k-major weights: as fa; n-major: word j of [.][j >> 2][j & 3] is k = 2 j + kg
#pragma unroll
    for (int mt = 0; mt < TT; ++mt)
#pragma unroll
      for (int cc = 0; cc < 8; ++cc) fa[mt][cc] = *reinterpret_cast<const xf_f32x4 *>(st + a_row + mt * (32 * 128) + ((cc ^ sw) << 4));
#pragma unroll
    for (int nt = 0; nt < TT; ++nt) {
      if (WK) {
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) fw[nt][cc] = *reinterpret_cast<const xf_f32x4 *>(st + w_row + nt * (32 * 128) + ((cc ^ sw) << 4));
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) fw[nt][j >> 2][j & 3] = *reinterpret_cast<const float *>(st + w_row + 2 * j * RB + nt * (32 * 4));
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    // the other stage is free since the barrier; issued here, behind this wave's reads, so that no wait the compiler may put in
    // front of an LDS read for a DMA in flight can land on them
    if (kt + 1 < nk) XF_ISSUE(kt + 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 16; ++j) {  // instruction j of the tile: k = 32 kt + 2 j + kg, ascending
      float av[TT], wv[TT];
#pragma unroll
      for (int mt = 0; mt < TT; ++mt) av[mt] = kg ? fa[mt][j >> 1][2 * (j & 1) + 1] : fa[mt][j >> 1][2 * (j & 1)];
#pragma unroll
      for (int nt = 0; nt < TT; ++nt) {
        if (WK) wv[nt] = kg ? fw[nt][j >> 1][2 * (j & 1) + 1] : fw[nt][j >> 1][2 * (j & 1)];
        else wv[nt] = fw[nt][j >> 2][j & 3];
      }
#pragma unroll
      for (int mt = 0; mt < TT; ++mt)
#pragma unroll
        for (int nt = 0; nt < TT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt], wv[nt], acc[mt][nt], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
#undef XF_ISSUE

  // ---- epilogue: lane = column n0 + 32 TT wn + 32 nt + l31; register g of tile mt = row m0 + 32 TT wm + 32 mt + 8 (g >> 2) + 4 kg + (g & 3)
#pragma unroll
  for (int mt = 0; mt < TT; ++mt)
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int r = m0 + wm * 32 * TT + mt * 32 + 8 * (g >> 2) + 4 * kg + (g & 3);
      if (r >= p.R) continue;
      int qw = 0, rw = r;
      if (p.d_rpw < p.R) { qw = r / p.d_rpw; rw = r - qw * p.d_rpw; }
      float *row = p.D + (long long)e * p.d_stride_e + (long long)qw * p.d_stride_w + (long long)rw * p.ldd;
#pragma unroll
      for (int nt = 0; nt < TT; ++nt) {
        const int n = n0 + wn * 32 * TT + nt * 32 + l31;
        if (n >= p.N) continue;
        float v = acc[mt][nt][g];
        if (p.bias != nullptr) v = v + bv[nt];
        row[n] = activate<ACT>(v);
      }
    }
}

static bool xf_shape_ok(int N, int K) { return N >= 4 && N % 4 == 0 && K >= XF_BK && K % XF_BK == 0; }

extern "C" int tutel_amd_expert_gemm_f32_supported(int N, int K) { return xf_shape_ok(N, K) ? 1 : 0; }

static const char XF_ENTRY[] = "tutel_amd_expert_gemm_f32";
static int xf_bad_act() { return tutel_notsup(XF_ENTRY, "the activation must be none, relu, gelu or silu"); }

// (the activations last to first: the compiler instantiates the list's kernels from its end, and they keep their order in the code object)
template <int WK, int TT> static int xf_launch(const XfArgs &a, int act, unsigned grid, hipStream_t st) {
  return dispatch_act<TUTEL_ACT_SILU, TUTEL_ACT_GELU, TUTEL_ACT_RELU, TUTEL_ACT_NONE>(
      act,
      [&](auto ac) {
        hipLaunchKernelGGL((expert_gemm_f32_kernel<WK, decltype(ac)::value, TT>), dim3(grid), dim3(XF_THREADS), 4 * (64 * TT) * XF_BK * 4, st, a);
        TUTEL_CHECK_LAUNCH(XF_ENTRY);
        return 0;
      },
      xf_bad_act);
}

// The tile: a pure function of (E_loc, R, N).  128 x 128 where that fills the chip (one tile per CU or more); 64 x 64 below that --
// four times the workgroups, each wave one accumulator (its dependent latency equals the issue interval, so a wave alone still
// issues back to back).  Without split-K a K loop cannot be shared out, so a small grid is what a short problem costs; the bits
// do not depend on the tile.
static int xf_tile(int E_loc, int R, int N) {
  const long long t128 = (long long)E_loc * ((R + XF_BM - 1) / XF_BM) * ((N + XF_BN - 1) / XF_BN);
  return t128 >= XF_CUS ? 128 : 64;
}

extern "C" int tutel_amd_expert_gemm_f32(const void *A, int64_t a_stride_e, int64_t a_stride_w, int a_rows_per_w, int lda, const void *W,
                                         int w_kmajor, int64_t w_stride_e, int ldw, const void *bias, int64_t bias_stride_e, void *D,
                                         int64_t d_stride_e, int64_t d_stride_w, int d_rows_per_w, int ldd, int E_loc, int R, int N, int K,
                                         int act, const int32_t *slot_map, int T, const void *zero_row, tutel_stream_t stream) {
  // every check stands in front of the first HIP call
  TUTEL_REQUIRE(E_loc >= 0 && R >= 0 && N >= 1 && K >= 1, "tutel_amd_expert_gemm_f32: bad sizes E_loc=%d R=%d N=%d K=%d", E_loc, R, N, K);
  if (K % XF_BK != 0) return tutel_notsup(XF_ENTRY, "K must be a multiple of 32");
  if (N % 4 != 0) return tutel_notsup(XF_ENTRY, "N must be a multiple of 4");
  if (act != TUTEL_ACT_NONE && act != TUTEL_ACT_RELU && act != TUTEL_ACT_GELU && act != TUTEL_ACT_SILU)
    return xf_bad_act();
  if (lda % 4 != 0 || ldw % 4 != 0 || ldd % 4 != 0 || a_stride_e % 4 != 0 || a_stride_w % 4 != 0 || w_stride_e % 4 != 0 || d_stride_e % 4 != 0 ||
      d_stride_w % 4 != 0)
    return tutel_notsup(XF_ENTRY, "leading dimensions and strides must keep rows 16-byte aligned (multiples of 4)");
  const int tile = xf_tile(E_loc, R, N);
  const long long ntm = (R + tile - 1) / tile, ntn = (N + tile - 1) / tile;
  if ((long long)E_loc * R > 0x7fffffffLL || (long long)E_loc * ntm * ntn > 0x7fffffffLL)
    return tutel_notsup(XF_ENTRY, "E_loc * R and the tile count must stay below 2^31");
  if (E_loc == 0 || R == 0) return 0;
  TUTEL_REQUIRE(A && W && D, "tutel_amd_expert_gemm_f32: null pointer");
  TUTEL_REQUIRE(((uintptr_t)A % 16) == 0 && ((uintptr_t)W % 16) == 0 && ((uintptr_t)D % 4) == 0 && ((uintptr_t)bias % 4) == 0,
                "tutel_amd_expert_gemm_f32: A and W must be 16-byte aligned, D and bias 4-byte aligned");
  if (slot_map != nullptr)
    TUTEL_REQUIRE(T >= 1 && zero_row != nullptr && ((uintptr_t)zero_row % 16) == 0,
                  "tutel_amd_expert_gemm_f32: a slot map needs T >= 1 and a 16-byte aligned zero row");
  else
    TUTEL_REQUIRE(a_rows_per_w >= 1, "tutel_amd_expert_gemm_f32: a_rows_per_w must be >= 1");
  TUTEL_REQUIRE(d_rows_per_w >= 1, "tutel_amd_expert_gemm_f32: d_rows_per_w must be >= 1");

  XfArgs a;
  a.A = (const unsigned char *)A; a.a_stride_e = a_stride_e; a.a_stride_w = a_stride_w; a.a_rpw = a_rows_per_w < 1 ? 1 : a_rows_per_w; a.lda = lda;
  a.W = (const unsigned char *)W; a.w_stride_e = w_stride_e; a.ldw = ldw;
  a.bias = (const float *)bias; a.bias_stride_e = bias_stride_e;
  a.D = (float *)D; a.d_stride_e = d_stride_e; a.d_stride_w = d_stride_w; a.d_rpw = d_rows_per_w; a.ldd = ldd;
  a.R = R; a.N = N; a.K = K; a.ntm = (int)ntm; a.ntn = (int)ntn;
  a.slot_map = slot_map; a.T = T; a.zero_row = (const unsigned char *)zero_row;
  hipStream_t st = (hipStream_t)stream;
  StageScope stage(act != TUTEL_ACT_NONE ? TUTEL_STAGE_FC1 : TUTEL_STAGE_FC2, st);
  const unsigned grid = (unsigned)((long long)E_loc * ntm * ntn);
  if (tile == 128) return w_kmajor ? xf_launch<1, 2>(a, act, grid, st) : xf_launch<0, 2>(a, act, grid, st);
  return w_kmajor ? xf_launch<1, 1>(a, act, grid, st) : xf_launch<0, 1>(a, act, grid, st);
}
