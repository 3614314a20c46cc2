// packed_train.hip -- the backward of the packed dropless ffn layer (dropless.hip's layout) that the forward kernels lack:
//
//   dW[e] = A[rows(e)]^T . B[rows(e)]       rows(e) = [off[e], off[e+1]) read from the device offsets      (weight gradient)
//   db[e] = sum over rows(e) of B            (bias gradient: a segmented column sum)
//
// The contraction runs over the packed ROW index, whose extent per expert only the device knows, so the ATen batched GEMM of the
// padded path (hid^T @ gy on [E, C, *] with a host C) has no packed equivalent.  Both operands are row-major over that index.
//
// Weight-gradient tile: 128 (N_a) x 128 (N_b) outputs per 4-wave workgroup, each wave 64 x 64 = 2 x 2 v_mfma_f32_32x32x16
// accumulators, 64 rows per step.  The MFMA wants 8 consecutive rows of one column per lane, so each operand tile lands in LDS
// TRANSPOSED, [column][row] (row pitch 64 + 8 elements: the 16-byte fragment reads of 32 consecutive columns are conflict-free):
// one thread fetches an 8-row x 8-column block (eight 16-byte loads down the rows), transposes it in registers and writes 8
// 16-byte LDS rows.  The B fragment is the MFMA's "A" so that a lane ends up with 4 consecutive N_b outputs of one N_a row:
// 8-byte stores, the layout of the parameters [E, N_a, N_b].  With OT = float (the *_f32 entry points: fp32 master weights under
// autocast) the same four accumulators leave unrounded as one 16-byte store; everything before the epilogue is shared, so the
// fp32 form is the 16-bit form's sum without its final rounding.
// One workgroup owns one output tile and walks its expert's rows in order: fp32 sums in a fixed order, no atomics, the same bits
// run after run.  An expert without rows stores zeros; nothing at or past off[E] is read.  One operand may be gathered through
// the packed slot map (pad rows -> the zero row), as the forward fc1 gathers its rows, so no packed copy of x exists.
// ACC (the *_acc_f32 entry points, OT = float only: gradient accumulation into an fp32 main_grad over micro-batches): the epilogue
// reads the 16 bytes of D it owns, adds the four accumulators (one fp32 add each; -ffp-contract=off, and nothing to fuse with)
// and stores them back -- D += G with G the *_f32 form's bits.  The tile has one owner, so the read-modify-write needs no atomic.
// An expert without rows returns before the epilogue: its part of D is neither read nor written.
#include <climits>

#include "common.h"

#include "gemm_dev.h"

#define WG_T 128     // output tile edge
#define WG_BK 64     // rows per step
#define WG_LD (WG_BK + 8)
#define WG_THREADS 256

// OT: the output element, T's 16 bits (D as uint16_t) or float; ACC: D += the sums instead of D = them
template <typename T, typename OT, bool ACC = false>
__global__ __launch_bounds__(WG_THREADS, 2) void packed_wgrad_kernel(const uint16_t *__restrict__ A, int lda, const uint16_t *__restrict__ B, int ldb,
                                                                    const int32_t *__restrict__ rows_map, int gather_b, int t_mod,
                                                                    const uint16_t *__restrict__ zero_row, OT *__restrict__ D, int Na,
                                                                    int Nb, int tna, int tnb, const int32_t *__restrict__ off) {
  __shared__ __attribute__((aligned(16))) uint16_t sA[WG_T * WG_LD];
  __shared__ __attribute__((aligned(16))) uint16_t sB[WG_T * WG_LD];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wa = wid >> 1, wb = wid & 1;
  const int bid = blockIdx.x;
  const int e = bid / (tna * tnb), ta = (bid / tnb) % tna, tb = bid % tnb;
  const int i0 = ta * WG_T, j0 = tb * WG_T;
  const int r_begin = __builtin_amdgcn_readfirstlane(off[e]), r_end = __builtin_amdgcn_readfirstlane(off[e + 1]);
  if constexpr (ACC) {
    static_assert(sizeof(OT) == 4, "the accumulating form is fp32 only");
    if (r_begin >= r_end) return;  // no rows (uniform over the workgroup): D keeps its bits, untouched
  }

  // loader: threads 0..127 the A tile, 128..255 the B tile; thread -> (8-row block rb, 8-column chunk cb)
  const bool is_a = tid < 128;
  const int lt = tid & 127, rb = lt >> 4, cb = lt & 15;
  const int col = (is_a ? i0 : j0) + cb * 8;
  const bool col_ok = col < (is_a ? Na : Nb);  // N % 8 == 0: a chunk is wholly inside or outside
  uint16_t *sdst = (is_a ? sA : sB) + (cb * 8) * WG_LD + rb * 8;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int l31 = lane & 31, kg = lane >> 5;
  u32x4 v[8];
  auto fetch = [&](int r0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int r = r0 + rb * 8 + q;
      const uint16_t *src = nullptr;
      if (col_ok && r < r_end) {
        const uint16_t *base = is_a ? A : B;
        const int ld = is_a ? lda : ldb;
        if (rows_map != nullptr && is_a != (gather_b != 0)) {  // the gathered operand: token rows_map[r] % T, the zero row for -1
          const int s = rows_map[r];
          src = s >= 0 ? base + (size_t)(s % t_mod) * ld + col : zero_row;
        } else {
          src = base + (size_t)r * ld + col;
        }
      }
      v[q] = src != nullptr ? *reinterpret_cast<const u32x4 *>(src) : u32x4{0u, 0u, 0u, 0u};
    }
  };
  auto stash = [&]() {
    // 8 x 8 transpose: LDS row c (column col + c of the operand) gets the 8 rows' elements c
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      uint32_t w[4];
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const uint32_t lo = (v[2 * h][c >> 1] >> ((c & 1) * 16)) & 0xffffu;
        const uint32_t hi = (v[2 * h + 1][c >> 1] >> ((c & 1) * 16)) & 0xffffu;
        w[h] = lo | (hi << 16);
      }
      *reinterpret_cast<u32x4 *>(sdst + c * WG_LD) = u32x4{w[0], w[1], w[2], w[3]};
    }
  };

  for (int r0 = r_begin; r0 < r_end; r0 += WG_BK) {
    fetch(r0);
    __syncthreads();  // the previous step's fragment reads are done
    stash();
    __syncthreads();
    u32x4 fa[WG_BK / 16][2], fb[WG_BK / 16][2];
#pragma unroll
    for (int kk = 0; kk < WG_BK / 16; ++kk)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        fa[kk][s] = *reinterpret_cast<const u32x4 *>(sA + (wa * 64 + s * 32 + l31) * WG_LD + kk * 16 + kg * 8);
        fb[kk][s] = *reinterpret_cast<const u32x4 *>(sB + (wb * 64 + s * 32 + l31) * WG_LD + kk * 16 + kg * 8);
      }
#pragma unroll
    for (int kk = 0; kk < WG_BK / 16; ++kk)
#pragma unroll
      for (int nj = 0; nj < 2; ++nj)
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) acc[nj][mi] = Mma<T>::run(fb[kk][nj], fa[kk][mi], acc[nj][mi]);
  }

  // lane: output row i = i0 + wa*64 + mi*32 + l31, columns j = j0 + wb*64 + nj*32 + rg*8 + kg*4 + 0..3
  OT *De = D + (size_t)e * Na * Nb;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const int i = i0 + wa * 64 + mi * 32 + l31;
    if (i >= Na) continue;
#pragma unroll
    for (int nj = 0; nj < 2; ++nj)
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const int j = j0 + wb * 64 + nj * 32 + rg * 8 + kg * 4;
        if (j >= Nb) continue;
        if constexpr (ACC) {  // fp32 read-modify-write of the 16 bytes this lane owns
          float4 *dp = reinterpret_cast<float4 *>(De + (size_t)i * Nb + j);
          float4 d = *dp;
          d.x += acc[nj][mi][rg * 4];
          d.y += acc[nj][mi][rg * 4 + 1];
          d.z += acc[nj][mi][rg * 4 + 2];
          d.w += acc[nj][mi][rg * 4 + 3];
          *dp = d;
        } else if constexpr (sizeof(OT) == 4) {  // fp32: the accumulators as they are, 16 bytes (N_b % 8 == 0 and D 16-byte aligned)
          *reinterpret_cast<float4 *>(De + (size_t)i * Nb + j) =
              float4{acc[nj][mi][rg * 4], acc[nj][mi][rg * 4 + 1], acc[nj][mi][rg * 4 + 2], acc[nj][mi][rg * 4 + 3]};
        } else {
          uint16_t o[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            T tv = Elem<T>::from_f32(acc[nj][mi][rg * 4 + r]);
            __builtin_memcpy(&o[r], &tv, 2);
          }
          uint2 ov;
          ov.x = (uint32_t)o[0] | ((uint32_t)o[1] << 16);
          ov.y = (uint32_t)o[2] | ((uint32_t)o[3] << 16);
          *reinterpret_cast<uint2 *>(De + (size_t)i * Nb + j) = ov;
        }
      }
  }
}

// db[e][n] = sum of B[r][n] over rows(e): one thread per (expert, column), the rows in order (fp32, rounded once; OT = float: not at all)
// ACC (OT = float): D[e][n] += the sum; an expert without rows leaves D untouched
template <typename T, typename OT, bool ACC = false>
__global__ __launch_bounds__(256) void packed_bgrad_kernel(const T *__restrict__ B, int ldb, OT *__restrict__ D, int N,
                                                           const int32_t *__restrict__ off) {
  const int e = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int r0 = off[e], r1 = off[e + 1];
  float s = 0.f;
  for (int r = r0; r < r1; ++r) s += Elem<T>::to_f32(B[(size_t)r * ldb + n]);
  if constexpr (ACC) {
    static_assert(sizeof(OT) == 4, "the accumulating form is fp32 only");
    if (r0 >= r1) return;
    D[(size_t)e * N + n] += s;
  } else if constexpr (sizeof(OT) == 4) D[(size_t)e * N + n] = s;
  else D[(size_t)e * N + n] = Elem<T>::from_f32(s);
}

// the three entry points of each gradient share their checks and launches: `what` names the caller in errors, out_f32 picks the
// output form, acc (with out_f32) the accumulating epilogue
static int wgrad_packed(const char *what, bool out_f32, bool acc, const void *A, int lda, const void *B, int ldb, const int32_t *rows_map, int gather, int T,
                        const void *zero_row, void *D, int E, int rows_bound, int Na, int Nb, int dtype, const int32_t *offsets,
                        tutel_stream_t stream) {
  TUTEL_REQUIRE(E >= 1 && rows_bound >= 0 && Na >= 1 && Nb >= 1 && lda >= Na && ldb >= Nb && gather >= 0 && gather <= 2 &&
                    (gather == 0 || (rows_map != nullptr && T >= 1)),
                "%s: bad sizes E=%d rows=%d Na=%d Nb=%d lda=%d ldb=%d gather=%d T=%d", what, E, rows_bound, Na, Nb, lda, ldb, gather, T);
  if (dtype != TUTEL_BF16 && dtype != TUTEL_F16) return tutel_notsup(what, "16-bit operands only");
  if (Na % 8 != 0 || Nb % 8 != 0 || lda % 8 != 0 || ldb % 8 != 0)
    return tutel_notsup(what, "N_a, N_b and the leading dimensions must be multiples of 8");
  const long long tiles = (long long)E * ((Na + WG_T - 1) / WG_T) * ((Nb + WG_T - 1) / WG_T);
  if (tiles >= 0x7fffffffLL) return tutel_notsup(what, "more than 2^31 output tiles");
  TUTEL_REQUIRE(A && B && D && offsets && (gather == 0 || zero_row), "%s: null pointer", what);
  auto al16 = [](const void *p) { return ((uintptr_t)p & 15) == 0; };
  TUTEL_REQUIRE(al16(A) && al16(B) && al16(zero_row) && ((uintptr_t)D & (out_f32 ? 15 : 7)) == 0,
                "%s: A, B and the zero row must be 16-byte aligned, D %d-byte", what, out_f32 ? 16 : 8);
  hipStream_t st = (hipStream_t)stream;
  StageScope stage(TUTEL_STAGE_OTHER, st);
  const int tna = (Na + WG_T - 1) / WG_T, tnb = (Nb + WG_T - 1) / WG_T;
  const int32_t *map = gather != 0 ? rows_map : nullptr;
#define WG_GO(TT, OT, ...)                                                                                                                 \
  hipLaunchKernelGGL((packed_wgrad_kernel<TT, OT, ##__VA_ARGS__>), dim3((unsigned)tiles), dim3(WG_THREADS), 0, st, (const uint16_t *)A, lda, (const uint16_t *)B, \
                     ldb, map, gather == 2 ? 1 : 0, T > 0 ? T : 1, (const uint16_t *)zero_row, (OT *)D, Na, Nb, tna, tnb, offsets)
  if (acc) {
    if (dtype == TUTEL_BF16) WG_GO(bf16_t, float, true);
    else WG_GO(f16_t, float, true);
  } else if (out_f32) {
    if (dtype == TUTEL_BF16) WG_GO(bf16_t, float);
    else WG_GO(f16_t, float);
  } else {
    if (dtype == TUTEL_BF16) WG_GO(bf16_t, uint16_t);
    else WG_GO(f16_t, uint16_t);
  }
#undef WG_GO
  TUTEL_CHECK_LAUNCH(what);
  return 0;
}

extern "C" int tutel_amd_expert_wgrad_packed(const void *A, int lda, const void *B, int ldb, const int32_t *rows_map, int gather, int T,
                                             const void *zero_row, void *D, int E, int rows_bound, int Na, int Nb, int dtype,
                                             const int32_t *offsets, tutel_stream_t stream) {
  return wgrad_packed("tutel_amd_expert_wgrad_packed", false, false, A, lda, B, ldb, rows_map, gather, T, zero_row, D, E, rows_bound, Na, Nb, dtype,
                      offsets, stream);
}

extern "C" int tutel_amd_expert_wgrad_packed_f32(const void *A, int lda, const void *B, int ldb, const int32_t *rows_map, int gather, int T,
                                                 const void *zero_row, float *D, int E, int rows_bound, int Na, int Nb, int dtype,
                                                 const int32_t *offsets, tutel_stream_t stream) {
  return wgrad_packed("tutel_amd_expert_wgrad_packed_f32", true, false, A, lda, B, ldb, rows_map, gather, T, zero_row, D, E, rows_bound, Na, Nb,
                      dtype, offsets, stream);
}

extern "C" int tutel_amd_expert_wgrad_packed_acc_f32(const void *A, int lda, const void *B, int ldb, const int32_t *rows_map, int gather, int T,
                                                     const void *zero_row, float *D, int E, int rows_bound, int Na, int Nb, int dtype,
                                                     const int32_t *offsets, tutel_stream_t stream) {
  return wgrad_packed("tutel_amd_expert_wgrad_packed_acc_f32", true, true, A, lda, B, ldb, rows_map, gather, T, zero_row, D, E, rows_bound, Na,
                      Nb, dtype, offsets, stream);
}

static int bgrad_packed(const char *what, bool out_f32, bool acc, const void *B, int ldb, void *D, int E, int N, int dtype, const int32_t *offsets,
                        tutel_stream_t stream) {
  TUTEL_REQUIRE(E >= 1 && N >= 1 && ldb >= N, "%s: bad sizes E=%d N=%d ldb=%d", what, E, N, ldb);
  if (dtype != TUTEL_BF16 && dtype != TUTEL_F16) return tutel_notsup(what, "16-bit operands only");
  TUTEL_REQUIRE(E <= 65535, "%s: E=%d above the grid's 65535", what, E);
  TUTEL_REQUIRE(B && D && offsets, "%s: null pointer", what);
  TUTEL_REQUIRE(!out_f32 || ((uintptr_t)D & 15) == 0, "%s: D must be 16-byte aligned", what);
  hipStream_t st = (hipStream_t)stream;
  StageScope stage(TUTEL_STAGE_OTHER, st);
  const dim3 grid((unsigned)((N + 255) / 256), (unsigned)E);
#define BG_GO(TT, OT, ...) hipLaunchKernelGGL((packed_bgrad_kernel<TT, OT, ##__VA_ARGS__>), grid, dim3(256), 0, st, (const TT *)B, ldb, (OT *)D, N, offsets)
  if (acc) {
    if (dtype == TUTEL_BF16) BG_GO(bf16_t, float, true);
    else BG_GO(f16_t, float, true);
  } else if (out_f32) {
    if (dtype == TUTEL_BF16) BG_GO(bf16_t, float);
    else BG_GO(f16_t, float);
  } else {
    if (dtype == TUTEL_BF16) BG_GO(bf16_t, bf16_t);
    else BG_GO(f16_t, f16_t);
  }
#undef BG_GO
  TUTEL_CHECK_LAUNCH(what);
  return 0;
}

extern "C" int tutel_amd_expert_bgrad_packed(const void *B, int ldb, void *D, int E, int N, int dtype, const int32_t *offsets,
                                             tutel_stream_t stream) {
  return bgrad_packed("tutel_amd_expert_bgrad_packed", false, false, B, ldb, D, E, N, dtype, offsets, stream);
}

extern "C" int tutel_amd_expert_bgrad_packed_f32(const void *B, int ldb, float *D, int E, int N, int dtype, const int32_t *offsets,
                                                 tutel_stream_t stream) {
  return bgrad_packed("tutel_amd_expert_bgrad_packed_f32", true, false, B, ldb, D, E, N, dtype, offsets, stream);
}

extern "C" int tutel_amd_expert_bgrad_packed_acc_f32(const void *B, int ldb, float *D, int E, int N, int dtype, const int32_t *offsets,
                                                     tutel_stream_t stream) {
  return bgrad_packed("tutel_amd_expert_bgrad_packed_acc_f32", true, true, B, ldb, D, E, N, dtype, offsets, stream);
}

// the grouped GEMM over the packed layout, public form of tutel_expert_gemm_packed (expert_gemm.hip).  N is any multiple of 8
// from 8 up (tutel_gemm_args refuses the rest before a launch): below the plan's 128 columns both kernels clamp every weight, bias
// and gating-operand load of a column tile into [0, N) and store whole 8-column groups below N only (include/tutel_amd.h)
extern "C" int tutel_amd_expert_gemm_packed(const void *A, int lda, const int32_t *a_rows, int T, const void *zero_row, const void *W,
                                            int w_kmajor, int64_t w_stride_e, int ldw, const void *bias, int64_t bias_stride_e, const void *mul,
                                            void *D, int ldd, int E, int rows_bound, int N, int K, int dtype, int act, const int32_t *offsets,
                                            const int32_t *tiles, const int32_t *ntiles, const int32_t *capacity, int tiles_bound,
                                            tutel_stream_t stream) {
  GemmPlanScope scope;
  TUTEL_REQUIRE(E >= 1 && rows_bound >= 1 && tiles_bound >= 1 && N >= 1 && K >= 1, "tutel_amd_expert_gemm_packed: bad sizes E=%d rows=%d tiles=%d N=%d K=%d",
                E, rows_bound, tiles_bound, N, K);
  if (dtype != TUTEL_BF16 && dtype != TUTEL_F16) return tutel_notsup("tutel_amd_expert_gemm_packed", "16-bit operands only");
  if (!w_kmajor && (act != TUTEL_ACT_NONE && act != TUTEL_ACT_RELU))
    return tutel_notsup("tutel_amd_expert_gemm_packed", "n-major weights take act none or relu");
  if (!w_kmajor && mul != nullptr) return tutel_notsup("tutel_amd_expert_gemm_packed", "the gated form takes k-major weights");
  TUTEL_REQUIRE(offsets && tiles && ntiles && capacity, "tutel_amd_expert_gemm_packed: null pointer");
  TUTEL_REQUIRE(((uintptr_t)D & 15) == 0 && ldd % 8 == 0 && ((uintptr_t)mul & 15) == 0,
                "tutel_amd_expert_gemm_packed: D and mul must be 16-byte aligned, ldd a multiple of 8");
  GemmProblem g;
  g.A = A; g.lda = lda;
  g.W = W; g.w_stride_e = w_stride_e; g.ldw = ldw; g.bias = bias; g.bias_stride_e = bias_stride_e;
  g.D = D; g.ldd = ldd;
  g.E_loc = E; g.N = N; g.K = K; g.dtype = dtype;
  g.mul = mul;
  gemm_one_rank(g, rows_bound);
  gemm_gather(g, a_rows, T, zero_row);
  return tutel_expert_gemm_packed(g, w_kmajor, act, PackedTable{offsets, tiles, ntiles, capacity, tiles_bound}, nullptr, (hipStream_t)stream);
}
