// dropless.hip -- the dropless MoE forward (capacity_factor <= 0) without a host synchronisation: the PACKED layout.
//
// The padded dropless path (ep.hip, tutel_amd_moe_forward) shapes the expert buckets [E, C, *] with C = the maximum expert load,
// so it copies that load to the host and synchronises before the expert GEMMs are enqueued (the reference's `int(capacity)`,
// tutel/impls/fast_dispatch.py:191-199), and a batch that needs more rows than the workspace holds is run again.  Here the experts'
// rows lie back to back instead:
//   kept_e = min(dispatch_count[e], L)     L = round_up(capacity_limit, alignment) (none when capacity_limit == 0)
//   rows_e = round_up(kept_e, alignment)   expert e owns rows [off[e], off[e] + rows_e), off = exclusive prefix sum of rows
// L is the limit rounded up because the padded path keeps the entries with loc < C = round_up(min(max load, limit), alignment):
// an entry of expert e is kept there iff loc < min(count_e, round_up(limit, alignment)), whatever the other experts' loads.  The
// device "capacity" max_e rows_e is then exactly that C.
//
// One layout launch (packed_layout_kernel) turns dispatch_count / idx / loc into off, the tile table of the expert GEMMs, the packed
// slot map and the device capacity; the GEMMs (expert_gemm.hip, tutel_expert_gemm_packed) and the decode (dispatch.hip) read them
// on the device.  Buffers and grids are sized by the host bound of tutel_amd_packed_plan, a function of (T, E, k, limit, alignment).
//
// Tile rule: PK_TILE_ROWS = 256 rows per M-tile, for every shape -- the 256 x 256 ping-pong kernel the padded path takes at the
// dropless headline shape (E = 64, T = 4096, k = 2: ~160 rows per expert, gemm_plan).  With 128-row tiles an expert above 128 rows
// streams its weights twice (the gemm_plan comments record fc1 at 214 us vs 118 us); a 256-row tile of an expert with fewer rows
// skips the MFMAs of the empty 32-row groups (the RAGGED form) and its weights are still streamed once.
#include <climits>

#include "common.h"

#define LY_THREADS 1024
#define LY_MAX_E 4096
#define LY_PER (LY_MAX_E / LY_THREADS)  // experts per thread in the scan

static_assert(PK_TILE_ROWS == 256, "the packed GEMM is the 256-row ping-pong kernel");

static inline size_t pk_align(size_t b) { return (b + 255) & ~(size_t)255; }

// Every block recomputes the prefix sums of rows / tiles over the E <= 4096 experts (a few microseconds of LDS work, no
// inter-block dependency), then grid-strides over the (choice, token) entries and the packed rows; block 0 also writes off, the tile
// table, the live tile count and the capacity.  Nothing is read past dispatch_count[E], idx / loc [k*T]; nothing is written past
// off[E + 1], tiles[2 * tiles_bound], slot[rows_bound].
__global__ __launch_bounds__(LY_THREADS) void packed_layout_kernel(const int32_t *__restrict__ cnt, const int32_t *__restrict__ idx,
                                                                   const int32_t *__restrict__ loc, int n, int E, int L, int al,
                                                                   int rows_bound, int tiles_bound, int32_t *__restrict__ off_out,
                                                                   int32_t *__restrict__ tiles, int32_t *__restrict__ ntiles,
                                                                   int32_t *__restrict__ cap, int32_t *__restrict__ slot) {
  __shared__ int s_off[LY_MAX_E + 1];   // exclusive prefix sum of rows_e (s_off[E] = rows used)
  __shared__ int s_toff[LY_MAX_E + 1];  // exclusive prefix sum of the experts' tile counts
  __shared__ int s_part[2][LY_THREADS];
  __shared__ int s_cap;
  const int tid = threadIdx.x;
  int r_loc[LY_PER], t_loc[LY_PER];
  int rsum = 0, tsum = 0, rmax = 0;
#pragma unroll
  for (int i = 0; i < LY_PER; ++i) {
    const int e = tid * LY_PER + i;
    int r = 0;
    if (e < E) {
      const int kept = min(cnt[e], L);
      r = (kept + al - 1) / al * al;
    }
    r_loc[i] = r;
    t_loc[i] = (r + PK_TILE_ROWS - 1) / PK_TILE_ROWS;
    rsum += r;
    tsum += t_loc[i];
    rmax = max(rmax, r);
  }
  s_part[0][tid] = rsum;
  s_part[1][tid] = tsum;
  if (tid == 0) s_cap = 0;
  __syncthreads();
  if (rmax > 0) atomicMax(&s_cap, rmax);
  for (int d = 1; d < LY_THREADS; d <<= 1) {  // inclusive scan of the per-thread sums
    const int a = tid >= d ? s_part[0][tid - d] : 0, b = tid >= d ? s_part[1][tid - d] : 0;
    __syncthreads();
    s_part[0][tid] += a;
    s_part[1][tid] += b;
    __syncthreads();
  }
  {
    int rp = s_part[0][tid] - rsum, tp = s_part[1][tid] - tsum;
#pragma unroll
    for (int i = 0; i < LY_PER; ++i) {
      const int e = tid * LY_PER + i;
      if (e < E) {
        s_off[e] = rp;
        s_toff[e] = tp;
      }
      rp += r_loc[i];
      tp += t_loc[i];
    }
    if (tid == LY_THREADS - 1) {
      s_off[E] = s_part[0][tid];
      s_toff[E] = s_part[1][tid];
    }
  }
  __syncthreads();
  const int used = min(s_off[E], rows_bound);  // (== s_off[E]: the host bound holds for every count vector)

  if (blockIdx.x == 0) {
    for (int e = tid; e <= E; e += LY_THREADS) off_out[e] = s_off[e];
    for (int e = tid; e < E; e += LY_THREADS) {
      const int r0 = s_off[e], r1 = min(s_off[e + 1], used);
      for (int j = 0, t = s_toff[e]; r0 + j * PK_TILE_ROWS < r1 && t < tiles_bound; ++j, ++t) {
        tiles[2 * t] = e;
        tiles[2 * t + 1] = r0 + j * PK_TILE_ROWS;
      }
    }
    if (tid == 0) {
      *ntiles = min(s_toff[E], tiles_bound);
      *cap = s_cap;
    }
  }
  const int gtid = blockIdx.x * LY_THREADS + tid, stride = gridDim.x * LY_THREADS;
  // the kept entries: slot[off[e] + loc] = j*T + t (loc < count_e always, so loc < L is loc < kept_e)
  for (int q = gtid; q < n; q += stride) {
    const int e = idx[q], l = loc[q];
    if (e >= 0 && e < E && l >= 0 && l < L) {
      const int r = s_off[e] + l;
      if (r < s_off[e + 1] && r < used) slot[r] = q;
    }
  }
  // every other row of the bound: -1 (the GEMM's gather reads the zero row there)
  for (int r = gtid; r < rows_bound; r += stride) {
    if (r >= used) {
      slot[r] = -1;
      continue;
    }
    int lo = 0, hi = E;  // s_off[lo] <= r < s_off[hi]: the expert owning row r
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (s_off[mid] <= r) lo = mid;
      else hi = mid;
    }
    if (r - s_off[lo] >= min(cnt[lo], L)) slot[r] = -1;
  }
}

extern "C" int tutel_amd_packed_plan(int T, int E, int k, int M, int H, int M_out, int dtype, int capacity_limit, int alignment,
                                     tutel_amd_packed_plan_t *out) {
  TUTEL_REQUIRE(out != nullptr && T >= 0 && E >= 1 && k >= 1 && M >= 1 && H >= 1 && M_out >= 1 && capacity_limit >= 0 && alignment >= 1,
                "tutel_amd_packed_plan: bad sizes T=%d E=%d k=%d M=%d H=%d M_out=%d limit=%d alignment=%d", T, E, k, M, H, M_out,
                capacity_limit, alignment);
  auto notsup = [](const char *why) { return tutel_notsup("tutel_amd_packed_plan", why); };
  if (dtype != TUTEL_BF16 && dtype != TUTEL_F16) return notsup("16-bit experts only");
  if (k > 16 || k > E || E > LY_MAX_E || (long long)k * E > 8192) return notsup("1 <= k <= min(E, 16), E <= 4096, k * E <= 8192");
  if (M % 64 != 0 || H % 64 != 0) return notsup("M and H must be multiples of 64");
  if (H < 128 || M_out < 128 || M_out % 8 != 0) return notsup("H and M_out must be >= 128 (M_out a multiple of 8)");
  const long long kT = (long long)k * T, nz = kT < E ? kT : E;  // experts that can hold a row
  const long long L = capacity_limit > 0 ? ((long long)capacity_limit + alignment - 1) / alignment * alignment : 0;
  long long rows = kT + nz * (alignment - 1);
  if (L > 0 && rows > nz * L) rows = nz * L;
  const long long tiles = rows / PK_TILE_ROWS + nz;
  const long long wide = H > M_out ? H : M_out;
  if (kT >= INT_MAX || L >= INT_MAX || rows * wide * 2 >= 0x7ffff000LL || (long long)T * M * 2 >= 0x7ffff000LL)
    return notsup("operands of 2 GiB and more");
  out->rows_bound = (int)rows;
  out->tiles_bound = (int)tiles;
  out->tile_rows = PK_TILE_ROWS;
  out->row_limit = (int)L;
  out->ws_bytes = pk_align((size_t)rows * 4) + pk_align((size_t)tiles * 8) + 256 + pk_align((size_t)rows * H * 2) +
                  pk_align((size_t)rows * M_out * 2);
  return 0;
}

// the layout launch (packed_layout_kernel) of tutel_amd_moe_forward_packed, over buffers the caller sized from tutel_amd_packed_plan
static void launch_layout(const int32_t *cnt, const int32_t *idx, const int32_t *loc, int T, int E, int k, int L, int alignment, int rows_bound,
                          int tiles_bound, int32_t *off, int32_t *tiles, int32_t *ntiles, int32_t *cap, int32_t *slot, hipStream_t st) {
  const long long work = (long long)k * T > rows_bound ? (long long)k * T : rows_bound;
  long long grid = (work + 4 * LY_THREADS - 1) / (4 * LY_THREADS);
  grid = grid < 1 ? 1 : (grid > 256 ? 256 : grid);
  hipLaunchKernelGGL(packed_layout_kernel, dim3((unsigned)grid), dim3(LY_THREADS), 0, st, cnt, idx, loc, k * T, E, L, alignment, rows_bound,
                     tiles_bound, off, tiles, ntiles, cap, slot);
}

extern "C" int tutel_amd_packed_layout(const int32_t *dispatch_count, const int32_t *idx, const int32_t *loc, int T, int E, int k,
                                       int capacity_limit, int alignment, int rows_bound, int tiles_bound, int32_t *offsets, int32_t *tiles,
                                       int32_t *ntiles, int32_t *capacity, int32_t *slot_map, tutel_stream_t stream) {
  TUTEL_REQUIRE(T >= 1 && E >= 1 && k >= 1 && capacity_limit >= 0 && alignment >= 1, "tutel_amd_packed_layout: bad sizes T=%d E=%d k=%d limit=%d alignment=%d",
                T, E, k, capacity_limit, alignment);
  tutel_amd_packed_plan_t pl;
  // (M, H, M_out = 128 and bf16: the bounds depend on (T, E, k, limit, alignment) alone)
  const int rc = tutel_amd_packed_plan(T, E, k, 128, 128, 128, TUTEL_BF16, capacity_limit, alignment, &pl);
  if (rc) return rc;
  TUTEL_REQUIRE(rows_bound >= pl.rows_bound && tiles_bound >= pl.tiles_bound, "tutel_amd_packed_layout: buffers below the plan's bounds (rows %d < %d or tiles %d < %d)",
                rows_bound, pl.rows_bound, tiles_bound, pl.tiles_bound);
  TUTEL_REQUIRE(dispatch_count && idx && loc && offsets && tiles && ntiles && capacity && slot_map, "tutel_amd_packed_layout: null pointer");
  hipStream_t st = (hipStream_t)stream;
  StageScope sc(TUTEL_STAGE_OTHER, st);
  launch_layout(dispatch_count, idx, loc, T, E, k, pl.row_limit > 0 ? pl.row_limit : INT_MAX, alignment, rows_bound, tiles_bound, offsets, tiles,
                ntiles, capacity, slot_map, st);
  TUTEL_CHECK_LAUNCH("tutel_amd_packed_layout");
  return 0;
}

extern "C" size_t tutel_amd_moe_packed_workspace_bytes(int T, int E, int k, int M, int H, int M_out, int dtype, int capacity_limit,
                                                       int alignment) {
  tutel_amd_packed_plan_t pl;
  return tutel_amd_packed_plan(T, E, k, M, H, M_out, dtype, capacity_limit, alignment, &pl) == 0 ? pl.ws_bytes : 0;
}

// w_up == NULL: the ffn experts (fc1 = act(x @ w1^T + b1), fc2); else SwiGLU experts: the fused gate/up GEMM on (w1, w_up), then
// w2 (the down projection) -- no biases
static int forward_packed(tutel_amd_ep_comm_t *c, const tutel_amd_moe_args_t *m, const tutel_amd_packed_args_t *pk, const void *w_up,
                          tutel_stream_t stream) {
  GemmPlanScope scope;
  TUTEL_REQUIRE(m != nullptr && pk != nullptr, "tutel_amd_moe_forward_packed: null arguments");
  const tutel_amd_ep_args_t &a = m->ep;
  const int T = a.T, E = a.num_experts, k = a.k, M = a.M, H = a.H, Mo = a.M_out;
  TUTEL_REQUIRE(c == nullptr && a.world == 1, "tutel_amd_moe_forward_packed: single rank only (comm must be NULL, world 1)");
  tutel_amd_packed_plan_t pl;
  int rc = tutel_amd_packed_plan(T, E, k, M, H, Mo, a.dtype, m->capacity_limit, m->alignment, &pl);
  if (rc) return rc;
  if (!a.is_postscore || !a.w2_kmajor)
    return tutel_notsup("tutel_amd_moe_forward_packed", "needs is_postscore (gates in the decode) and k-major fc2 weights");
  TUTEL_REQUIRE(pk->offsets != nullptr && pk->capacity != nullptr && m->dispatch_count != nullptr && m->ws != nullptr,
                "tutel_amd_moe_forward_packed: null pointer");
  TUTEL_REQUIRE(pk->ws != nullptr && ((uintptr_t)pk->ws & 15) == 0 && pk->ws_bytes >= pl.ws_bytes,
                "tutel_amd_moe_forward_packed: packed workspace too small or misaligned (%zu bytes, need %zu)", pk->ws_bytes, pl.ws_bytes);
  const bool project = m->logits == nullptr && m->gate_w != nullptr;
  TUTEL_REQUIRE(m->logits != nullptr || project || T == 0, "tutel_amd_moe_forward_packed: null logits");
  hipStream_t st = (hipStream_t)stream;
  if (T == 0) {
    const hipError_t e0 = hipMemsetAsync(pk->offsets, 0, (size_t)(E + 1) * 4, st), e1 = hipMemsetAsync(pk->capacity, 0, 4, st);
    TUTEL_REQUIRE(e0 == hipSuccess && e1 == hipSuccess, "tutel_amd_moe_forward_packed: memset failed");
    return tutel_amd_compute_location(nullptr, 0, E, k, 1, m->ws, m->ws_bytes, nullptr, m->dispatch_count, m->stats, m->l_aux,
                                      m->logits_dtype, 0, nullptr, 0, stream);
  }
  // every check of the launches below, made before the first of them is enqueued
  TUTEL_REQUIRE(a.x && a.idx && a.loc && a.gates && a.w1 && a.w2 && a.y && a.zero_row, "tutel_amd_moe_forward_packed: null pointer");
  TUTEL_REQUIRE(m->logits_dtype == TUTEL_F32 || m->logits_dtype == TUTEL_F16 || m->logits_dtype == TUTEL_BF16,
                "tutel_amd_moe_forward_packed: bad logits dtype %d", m->logits_dtype);
  TUTEL_REQUIRE(m->ws_bytes >= tutel_amd_routing_workspace_bytes(T, E, k), "tutel_amd_moe_forward_packed: routing workspace too small (%zu bytes, need %zu)",
                m->ws_bytes, tutel_amd_routing_workspace_bytes(T, E, k));
  TUTEL_REQUIRE(a.act >= TUTEL_ACT_NONE && a.act <= TUTEL_ACT_SILU, "tutel_amd_moe_forward_packed: unknown activation %d", a.act);
  TUTEL_REQUIRE(w_up == nullptr || (a.b1 == nullptr && a.b2 == nullptr && ((uintptr_t)w_up & 15) == 0),
                "tutel_amd_moe_forward_packed_glu: SwiGLU experts take no biases, and w_up must be 16-byte aligned");
  if (w_up != nullptr && a.act != TUTEL_ACT_RELU && a.act != TUTEL_ACT_GELU && a.act != TUTEL_ACT_SILU)
    return tutel_notsup("tutel_amd_moe_forward_packed_glu", "the gate activation must be relu, gelu or silu");
  auto al16 = [](const void *p) { return ((uintptr_t)p & 15) == 0; };
  TUTEL_REQUIRE(al16(a.x) && al16(a.w1) && al16(a.w2) && al16(a.y) && al16(a.zero_row) && ((uintptr_t)a.b1 & 7) == 0 && ((uintptr_t)a.b2 & 7) == 0,
                "tutel_amd_moe_forward_packed: x / weights / y / zero_row must be 16-byte aligned (biases 8-byte)");
  int splits = 0;
  if (project) {
    TUTEL_REQUIRE(a.dtype == m->logits_dtype || gate_proj_mixed(a.dtype, m->logits_dtype), "tutel_amd_moe_forward_packed: the in-call gate projection needs the gate in the token dtype");
    splits = tutel_gate_proj_splits_for(T, M, E, a.dtype, m->logits_dtype);
    TUTEL_REQUIRE(splits > 0, "tutel_amd_moe_forward_packed: the in-call gate projection does not cover T=%d, M=%d, E=%d (pass logits)", T, M, E);
    TUTEL_REQUIRE(m->gate_partials != nullptr && m->gate_partial_bytes >= (size_t)splits * T * E * sizeof(float),
                  "tutel_amd_moe_forward_packed: gate_partials must hold %d x %d x %d floats", splits, T, E);
  }

  // workspace: packed slot map | tile table | live tile count | fc1 output [rows, H] | fc2 output [rows, M_out]
  char *w = (char *)pk->ws;
  int32_t *slot = (int32_t *)w;
  w += pk_align((size_t)pl.rows_bound * 4);
  int32_t *tiles = (int32_t *)w;
  w += pk_align((size_t)pl.tiles_bound * 8);
  int32_t *ntiles = (int32_t *)w;
  w += 256;
  void *hid = w;
  w += pk_align((size_t)pl.rows_bound * H * 2);
  void *outb = w;

  // tutel_amd_expert_gemm_plan_next: only the two GEMMs answer (out[0], out[1]); nothing is launched
  const bool ask = gemm_plan_asked(0);
  rc = ask ? 0 : tutel_route_launch(*m, splits, nullptr, stream);
  if (rc) return rc;
  const int L = pl.row_limit > 0 ? pl.row_limit : INT_MAX;
  if (!ask) {
    StageScope sc(TUTEL_STAGE_OTHER, st);
    launch_layout(m->dispatch_count, a.idx, a.loc, T, E, k, L, m->alignment, pl.rows_bound, pl.tiles_bound, pk->offsets, tiles, ntiles,
                  pk->capacity, slot, st);
    TUTEL_CHECK_LAUNCH("tutel_amd_moe_forward_packed (layout)");
  }
  const PackedTable pt{pk->offsets, tiles, ntiles, pk->capacity, pl.tiles_bound};
  GemmProblem fc1, fc2;  // x [T, M] gathered through the packed slot map -> hid [rows, H] -> outb [rows, M_out]
  fc1.A = a.x; fc1.lda = M;
  fc1.W = a.w1; fc1.w_stride_e = (int64_t)H * M; fc1.ldw = M; fc1.bias = a.b1; fc1.bias_stride_e = H;
  fc1.D = hid; fc1.ldd = H;
  fc1.E_loc = E; fc1.N = H; fc1.K = M; fc1.dtype = a.dtype;
  gemm_one_rank(fc1, pl.rows_bound);
  gemm_gather(fc1, slot, T, a.zero_row);
  rc = tutel_expert_gemm_packed(fc1, 1, a.act, pt, w_up, st);
  if (rc) return rc;
  fc2.A = hid; fc2.lda = H;
  fc2.W = a.w2; fc2.w_stride_e = (int64_t)Mo * H; fc2.ldw = H; fc2.bias = a.b2; fc2.bias_stride_e = Mo;
  fc2.D = outb; fc2.ldd = Mo;
  fc2.E_loc = E; fc2.N = Mo; fc2.K = H; fc2.dtype = a.dtype;
  gemm_one_rank(fc2, pl.rows_bound);
  gemm_plan_asked(1);
  rc = tutel_expert_gemm_packed(fc2, 1, TUTEL_ACT_NONE, pt, nullptr, st);
  if (rc || ask) return rc;
  return tutel_decode_packed_launch(outb, a.dtype, a.idx, a.loc, a.gates, m->logits_dtype, T, Mo, k, L, pk->offsets, a.y, st);
}

extern "C" int tutel_amd_moe_forward_packed(tutel_amd_ep_comm_t *c, const tutel_amd_moe_args_t *m, const tutel_amd_packed_args_t *pk,
                                            tutel_stream_t stream) {
  return forward_packed(c, m, pk, nullptr, stream);
}

extern "C" int tutel_amd_moe_forward_packed_glu(tutel_amd_ep_comm_t *c, const tutel_amd_moe_args_t *m, const tutel_amd_packed_args_t *pk,
                                                const void *w_up, tutel_stream_t stream) {
  TUTEL_REQUIRE(w_up != nullptr, "tutel_amd_moe_forward_packed_glu: null w_up");
  return forward_packed(c, m, pk, w_up, stream);
}
