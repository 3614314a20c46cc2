// gemm_plan.hip -- which kernel a grouped expert GEMM runs, and on what grid: the one place that decides (host code only; the kernels
// and the switch that maps a plan to its instantiation are in expert_gemm.hip).  gemm_plan is a pure function: no HIP call, no option
// read, no pointer followed.  tests/test_gemm_plan_cpu.py pins every branch below on both sides of its boundary.
#include "gemm_dev.h"

// LDS of every ping-pong launch, 136 KB: the epilogue staging (8 waves x 64 rows x 272 B) > the two K-tile buffers (128 KB)
static constexpr size_t PP_LDS_BYTES = (size_t)8 * 64 * EP_PITCH;
static_assert(PP_LDS_BYTES >= (size_t)2 * (4 * GL_STAGE) * 2, "LDS request must cover the two K-tile buffers (2 x 4 * GL_STAGE elements)");
static constexpr size_t gemm_lds_bytes(bool kmajor) {
  return (size_t)(2 * GM_BM * (64 + 8) + 2 * (kmajor ? GM_BN * (64 + 8) : 64 * GM_LDN)) * 2;
}

#define GEMM_CHIP_CUS 256       // "the grid covers the chip": at least one workgroup for each CU of the part
#define GEMM_HALF_CHIP_MIN 96   // 96 .. 191 tiles of 256 x 256 cover about half the chip (a pipeline stage of an 8-way expert-parallel rank: 128)
#define GEMM_FULL_GRID_MIN 192  // a one-workgroup-per-CU grid pays from 3/4 of the CUs on; with fewer blocks CUs sit idle
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// tutel_amd_expert_gemm_plan_next (include/tutel_amd.h): armed -> taken by the next public entry point for the length of its call
static thread_local tutel_amd_gemm_plan_t *g_plan_armed = nullptr, *g_plan_out = nullptr;
static thread_local int g_plan_corun = 0, g_plan_slot = 0;
extern "C" int tutel_amd_expert_gemm_plan_next(tutel_amd_gemm_plan_t *out, int corun) {
  TUTEL_REQUIRE(out != nullptr, "tutel_amd_expert_gemm_plan_next: null pointer");
  for (int i = 0; i < 2; ++i) {
    out[i] = tutel_amd_gemm_plan_t{};
    out[i].family = -1;
  }
  g_plan_armed = out;
  g_plan_corun = corun != 0;
  return 0;
}
GemmPlanScope::GemmPlanScope() { g_plan_out = g_plan_armed; g_plan_armed = nullptr; g_plan_slot = 0; }
GemmPlanScope::~GemmPlanScope() { g_plan_out = nullptr; }
bool gemm_plan_asked(int slot) {
  if (slot >= 0) g_plan_slot = slot;
  return g_plan_out != nullptr;
}
bool gemm_plan_report(const GemmPlan &pl, const GemmArgs &a, int covered) {
  if (g_plan_out == nullptr) return false;
  tutel_amd_gemm_plan_t &o = g_plan_out[g_plan_slot];
  o = pl;
  o.rot_on = a.rot_on; o.fits32 = a.fits32; o.d_store = a.d_store; o.covered = covered;
  return true;
}

GemmKnobs gemm_knobs() {
  return GemmKnobs{tutel_get_option(TUTEL_OPT_GEMM_IMPL), tutel_get_option(TUTEL_OPT_GEMM_TILE), tutel_get_option(TUTEL_OPT_GEMM_PERSIST),
                   tutel_get_option(TUTEL_OPT_GEMM_SPLITK), g_plan_out != nullptr ? g_plan_corun : tutel_gemm_corun()};
}

// ---- the PLAIN form of the 128 x 256 ring kernel: who takes it -------------------------------------------------------------------------
// Yes only for the one layout the lean instantiation serves (gemm_plain.h): the 128-row ring plan; every row of an operand in one
// source rank (so row m sits m * ld past the expert's base); no peer rows, gating operand or row counts; 32-bit offsets, 16-byte output
// rows, write-through stores; whole 256-column tiles; the rotation computable in 32 bits.  Everything else takes the general kernel.
// The plan record (tutel_amd_gemm_plan_t) is the same either way: the form is a property of the launch, not of the plan.
bool gemm_plain_admits(const GemmPlan &pl, const GemmArgs &a) {
  const bool ring128 = pl.status == GEMM_PLAN_LAUNCH && pl.family == TUTEL_GEMM_RING && pl.bm == 128 && pl.ni == 4 && pl.ns == 3 && pl.buf && pl.w_kmajor;
  return ring128 && a.a_rpw >= a.R && a.d_rpw >= a.R && a.d_peer == nullptr && a.mul == nullptr && a.row_counts == nullptr && a.fits32 &&
         gemm_out_rows16(a) && a.d_store == 1 && a.N % 256 == 0 && a.K % GL_BK == 0 && gemm_plain_rot_fits(pl.ntn, a.E_loc, a.K / GL_BK);
}
// Not one of the numbered TUTEL_OPT_* knobs: an entry point of its own (tutel_amd_gemm_plain), seeded once from TUTEL_AMD_GEMM_PLAIN.
// -1 (automatic) and 1: the PLAIN kernel wherever the predicate holds; 0: never.
static int g_plain_mode = -2;
int gemm_plain_mode() {
  if (g_plain_mode == -2) {
    const char *s = getenv("TUTEL_AMD_GEMM_PLAIN");
    g_plain_mode = s ? atoi(s) : -1;
  }
  return g_plain_mode;
}
extern "C" int tutel_amd_gemm_plain(int value) {
  TUTEL_REQUIRE(value >= -2 && value <= 1, "tutel_amd_gemm_plain: value %d out of range", value);
  const int was = gemm_plain_mode();
  if (value != -2) g_plain_mode = value;
  return was;
}
static thread_local int g_last_form = TUTEL_GEMM_FORM_NONE, g_form_launches[2] = {0, 0};
void gemm_form_note(int form) {
  g_last_form = form;
  if (g_plan_out == nullptr) ++g_form_launches[form == TUTEL_GEMM_FORM_PLAIN];   // (an armed call launches nothing)
}
extern "C" int tutel_amd_expert_gemm_last_form(int *launches) {
  if (launches != nullptr) { launches[0] = g_form_launches[0]; launches[1] = g_form_launches[1]; }
  return g_last_form;
}

static GemmPlan plan_refused(int status, const char *error) {
  GemmPlan p = {};
  p.status = status; p.family = -1; p.error = error;
  return p;
}
// the 128 x 128 kernels on the argument block's own tiles: register-staged (2 x (tokens + weights), padded rows) or LDS-DMA (64 KB)
static GemmPlan plan_128(const GemmArgs &a, int family, bool km) {
  GemmPlan p = {};
  p.family = family; p.w_kmajor = km; p.ntm = a.ntm; p.ntn = a.ntn; p.threads = GM_THREADS;
  p.lds_bytes = family == TUTEL_GEMM_GLDS_128 ? 4 * GL_STAGE * 2 : (int)gemm_lds_bytes(km);
  return p;
}
// the ring tile (gemm_big_tile): bm rows x ni * 64 columns on ns slots; LDS = the ring [+ 16 KB of the fused-location scan] or, if larger,
// the epilogue's staging
static GemmPlan plan_ring(const GemmArgs &a, bool km, int ni, int ns, bool buf, int bm, bool fl) {
  GemmPlan p = {};
  p.family = TUTEL_GEMM_RING; p.w_kmajor = km; p.ni = ni; p.ns = ns; p.buf = buf; p.bm = bm; p.fl = fl;
  p.ntm = cdiv(a.R, bm); p.ntn = cdiv(a.N, ni * 64); p.threads = bm * 2;
  const size_t lds_k = (size_t)ns * (bm / 128 + ni / 2) * GL_STAGE * 2 + (fl ? 16384 : 0), lds_e = buf ? (size_t)(bm / 32) * 64 * (ni * 64 + 16) : 0;
  p.lds_bytes = (int)(lds_k > lds_e ? lds_k : lds_e);
  p.lds_epilogue = buf && gemm_out_rows16(a);
  return p;
}
static GemmPlan plan_pp(const GemmArgs &a, int ntm, int ntn) {
  GemmPlan p = {};
  p.family = TUTEL_GEMM_PINGPONG; p.w_kmajor = 1; p.ntm = ntm; p.ntn = ntn; p.threads = GB_THREADS; p.lds_bytes = (int)PP_LDS_BYTES;
  p.lds_epilogue = gemm_out_rows16(a);
  return p;
}
static GemmPlan plan_on_grid(GemmPlan p, long long grid, const char *entry, const char *too_large) {
  if (grid < 1 || grid >= 0x7fffffffLL) return plan_refused(-1, too_large);
  p.grid = (int)grid; p.entry = entry;
  return p;
}

// Fused location: only the 128 x 256 ring kernel has the form (capacity <= 128 rows per expert, slot map written by the kernel itself).
// K >= 128: the prologue's `s_waitcnt vmcnt(16)` counts the weight DMA of TWO K-tiles behind the idx bytes (with one
// K-tile only 8 follow and the wait would not cover them).
static bool gemm_fl_eligible(const GemmArgs &a) {
  return a.a_rows != nullptr && a.row_counts == nullptr && a.fl_n >= 1 && a.fl_n <= 15360 && a.E_loc <= 128 && a.K >= 2 * GL_BK;
}

GemmPlan gemm_plan(const GemmArgs &a, bool km, bool gate_up, int tiles_bound, const GemmKnobs &k) {
  const int ntm256 = cdiv(a.R, GB_BM), ntn256 = cdiv(a.N, 256), ntn128 = cdiv(a.N, GM_BN);
  auto covers_chip = [&](int ntn) { return (long long)a.E_loc * ntn >= GEMM_CHIP_CUS; };

  // ---- the packed dropless layout and the fused gate/up GEMM: one kernel per form, the tile table (tiles_bound entries) sizes the grid.
  if (tiles_bound > 0 && !km) {
    // n-major weights over the packed layout: the register-staged 128 x 128 kernel (its transposing LDS read takes W [K][N] as stored),
    // two 128-row M-tiles per entry of the 256-row tile table
    GemmPlan p = plan_128(a, TUTEL_GEMM_PACKED_NMAJOR, false);
    p.ntm = 1;
    return plan_on_grid(p, (long long)tiles_bound * 2 * p.ntn, "tutel_amd_expert_gemm_packed", "tutel_amd_expert_gemm_packed: grid too large");
  }
  if (tiles_bound > 0 || gate_up) {
    // Always the RAGGED ping-pong form (an expert's last tile is partial; dropless row counts).  Gate/up: 256 x 128 output tiles.
    // W_ONCE by the padded rule with one tile per expert, which is what the grid shape says when the experts cover the chip -- every
    // weight byte is then fetched by one block; an expert with more rows than one tile streams its weights once per tile, as padded
    // does.  The padded gate/up entry point never takes it (one instantiation fewer per activation; the hint changes no bits).
    const bool packed = tiles_bound > 0;
    GemmPlan p = plan_pp(a, packed ? 1 : ntm256, gate_up ? ntn128 : ntn256);
    p.ragged = 1; p.packed = packed; p.gate_up = gate_up; p.w_once = packed && covers_chip(p.ntn);
    if (gate_up) p.lds_epilogue = 1;  // (its entry points take 16-byte output rows only: the direct-store epilogue is not instantiated)
    const long long grid = packed ? (long long)tiles_bound * p.ntn : (long long)a.E_loc * p.ntm * p.ntn;
    return gate_up ? plan_on_grid(p, grid, "tutel_amd_expert_gemm_gate_up", "tutel_amd_expert_gemm_gate_up: grid too large")
                   : plan_on_grid(p, grid, "tutel_expert_gemm_packed", "tutel_expert_gemm_packed: grid too large");
  }

  // ---- padded: every kernel's grid is E_loc x its own M-tiles x N-tiles, never more blocks than the 128 x 128 tiling checked here
  auto padded = [&](const GemmPlan &p) {
    return plan_on_grid(p, (long long)a.E_loc * p.ntm * p.ntn, "tutel_amd_expert_gemm", "tutel_amd_expert_gemm: grid too large");
  };
  if ((long long)a.E_loc * a.ntm * a.ntn >= 0x7fffffffLL) return plan_refused(-1, "tutel_amd_expert_gemm: grid too large");
  const bool auto_tile = k.tile < 0, many_rows = a.R > GM_BM;
  // Round 4: all rows of an expert in one M-tile (R <= 128: weight streaming from HBM is the bound) and k-major weights -> the
  // 128 x 256 tile on a three-slot ring, one 4-wave block per CU: the token tile crosses L2 -> LDS once per 256 columns instead of
  // once per 128 and 96 KB of DMA are in flight per CU.  Headline shape (64 x 128 rows, 2048^2): fc1 112.4 -> 108.1 us, fc2
  // 111.9 -> 106.6 us, the forward 264.0 -> 258.4 us, same bits (profiles/r04_headline_ab.json).  Only when the grid still covers
  // the chip (one 144 KB block per CU): with fewer tiles the 128 x 128 kernel's twice as many blocks keep more CUs busy.
  // TUTEL_OPT_GEMM_IMPL = 4 forces it (where it applies), 1 forces the 128 x 128 LDS-DMA kernel.
  const bool ring128 = km && a.fits32 && a.N >= 256 && !many_rows && (k.impl == 4 || (k.impl < 0 && covers_chip(ntn256)));
  // Fused location FIRST: a request for it (or the eligibility query, fl_loc == NULL) must never fall into one of the launches
  // below, and a query launches nothing.
  if (a.fl_idx8 != nullptr) {
    if (!(ring128 && k.tile <= 0 && gemm_fl_eligible(a)))
      return plan_refused(TUTEL_AMD_ENOTSUP, "tutel_expert_gemm_gather_fl: this launch does not take the fused-location ring kernel");
    GemmPlan p = padded(plan_ring(a, true, 4, 3, true, 128, true));
    if (a.fl_loc == nullptr && p.status == GEMM_PLAN_LAUNCH) p.status = GEMM_PLAN_FL_QUERY;
    return p;
  }
  // R > 128 rows per expert: the 256-row tiles (more flop per byte crossing L2 -> CU) -- provided the grid
  // still covers the chip: one such block occupies a CU, so with fewer than ~3/4 x 256 blocks CUs sit idle.
  // 256 x 256 first, 256 x 128 when only that fills the chip (a pipeline stage of the overlapped
  // all-to-all is half a GEMM), else the 128-tile kernels.  tile = 1 forces 256 x 256, 2 / 3 force 256 x 128, 4 the ping-pong kernel.
  // More than one 128-row tile per expert (R > 128) already pays: the 128-tile kernels would stream every
  // weight tile once per M-tile (dropless capacity 157 at the headline shape: fc1 214 us vs 118 at R = 128).
  if (a.N >= GM_BN && k.tile != 0) {
    const long long mt256 = (long long)a.E_loc * ntm256, t256 = mt256 * ntn256, t128 = mt256 * ntn128;
    const bool half_chip = many_rows && t256 >= GEMM_HALF_CHIP_MIN && t256 < GEMM_FULL_GRID_MIN;
    const bool full_grid = auto_tile && many_rows && t256 >= GEMM_FULL_GRID_MIN;
    // Round 5: half the chip CAN run two workgroups per tile, each over half of K (expert_gemm_pp_kernel<.., SPLITK>).  Built, correct
    // (tests/test_ops_gpu.py::test_split_k_pingpong_kernel) and measured SLOWER than what it was to replace: the stage GEMM
    // 4 x 1024 x 2048^2 takes 52.6-58.6 us split against 40.8 us on the 256 x 128 ring and 50.5 us on the unsplit half-chip grid -- the
    // hand-over of 128 KB out + 128 KB in per workgroup through system-scope accesses costs more than the half K loop it saves
    // (profiles/r05_splitk_probe.json).  So it is opt-in only: TUTEL_OPT_GEMM_SPLITK = 1.  Whole 256-row tiles only (no ragged
    // variant), an even number of K-tiles with at least four per half (the steady-state loop), a multiple of four tiles (so that the
    // two workgroups of a tile are neighbours on one XCD in the work order), no rotation, 16-byte rows.
    const int nk = a.K / GL_BK;
    if (km && a.fits32 && a.mul == nullptr && half_chip && (auto_tile || k.tile == 4) && k.splitk == 1 && a.row_counts == nullptr &&
        a.R % GB_BM == 0 && !(nk & 1) && nk >= 8 && !(t256 & 3) && !a.rot_on && gemm_out_rows16(a)) {
      GemmPlan p = plan_pp(a, ntm256, ntn256);
      p.splitk = 1;
      return plan_on_grid(p, 2 * t256, "tutel_amd_expert_gemm", "tutel_amd_expert_gemm: grid too large");
    }
    // Beside a co-running collective (a stage of the overlapped pipeline: RCCL's kernels hold whole CUs on the other stream) a grid of
    // one workgroup per CU turns into two rounds as soon as a few CUs are taken: the 256 x 128 ring kernel at 4 x 1024 x 2048^2 goes
    // from 42 us to 70 us with 16 CUs held and to 57 us beside a device copy, the 128-block 256 x 256 grid stays at 52 us
    // (tools/contention_probe.py, profiles/r03_contention.json).  So with the co-run hint the half-filled 256 x 256 grid wins.
    const bool corun_pp = k.corun && auto_tile && half_chip;
    // What the split-K A/B did show: with 129 .. 191 tiles the 256 x 128 ring needs TWO rounds of workgroups (2 x t256 > 256 CUs) where
    // the unsplit 256 x 256 grid needs one at 1.5 x the flop per byte -- 5 x 1024 x 2048 x 4096: 124 us on the ring, 88.5 us on 160
    // ping-pong tiles (695 -> 971 TFLOP/s).  At <= 128 tiles the ring's single round wins (40.8 vs 50.5 us at 128).
    const bool pp_one_round = auto_tile && half_chip && 2 * t256 > GEMM_CHIP_CUS;
    if (km && a.fits32 && (k.tile == 4 || corun_pp || pp_one_round || full_grid)) {
      GemmPlan p = plan_pp(a, ntm256, ntn256);
      // a last M-tile with >= 32 padding rows, or per-expert row counts: the variant that skips padded 32-row groups
      const int tail_rows = a.R % GB_BM;
      p.ragged = a.row_counts != nullptr || (tail_rows != 0 && tail_rows <= GB_BM - 32);
      // bias fetched before the K loop (full tiles; +0.5-1.7 % on every MFMA-bound shape, profiles/r03_pp_bias_ab.json); 0 = after it, for A/B
      p.early_bias = !p.ragged && k.persist != 0;
      // one M-tile per expert and the chip covered: every weight byte is fetched by exactly one block -> no-allocate loads
      p.w_once = ntm256 == 1 && covers_chip(ntn256);
      return padded(p);
    }
    if (k.tile == 1 || k.tile == 4 || full_grid) return padded(plan_ring(a, km, 4, 2, false, GB_BM, false));
    // 256 x 128: a three-slot ring (3 x 48 KB of LDS) keeps two tiles in flight: +3-4 % over two slots on the
    // stage shapes it is chosen for (tools/stage_probe.py); tile = 2 forces the two-slot form for A/B runs, impl = 2 the direct-store epilogue
    if (km && k.tile == 2) return padded(plan_ring(a, true, 2, 2, false, GB_BM, false));
    if (km && (k.tile == 3 || (auto_tile && many_rows && t128 >= GEMM_FULL_GRID_MIN)))
      return padded(plan_ring(a, true, 2, 3, a.fits32 && k.impl != 2, GB_BM, false));
  }
  if (ring128) return padded(plan_ring(a, true, 4, 3, true, 128, false));
  // Kernel choice per weight layout, from on-hardware A/B at the headline shape and at R = 1024
  // rows/expert (tools/gemm_sweep.py, MI355X, round 1):
  //   k-major W (fc1): LDS-DMA kernel          126-132 us  (register-staged: 136-140 us)
  //   n-major W (fc2): register-staged kernel  124-128 us  (LDS-DMA: 128-130 us; its tr-read image
  //                                                         has residual bank conflicts)
  // both with non-temporal weight loads and the rotated K order (rows are 4 KB apart in both layouts;
  // without the per-block stagger all resident blocks sit at the same k offset: k-major 158 -> 143 us,
  // n-major 142 -> 130 us when the weights really come from HBM, i.e. fc1/fc2 alternating as in the
  // layer -- a warm Infinity Cache hides this, so A/B runs must alternate the two weight sets).  What did NOT pay (kept out of the tree,
  // see git history): BK=128, single LDS buffer at 3 blocks/CU, prefetch distance 2 (two register sets), a 128x256 8-wave 3-stage
  // LDS-DMA ring, a single-stage LDS-DMA variant at 4 blocks/CU.  Ablation: compute alone 69 us, loads+staging alone 80-115 us -- the
  // remaining loss is phase serialisation inside a block, not DRAM (pure loads of the same pattern: 77-90 us).
  // TUTEL_OPT_GEMM_IMPL = 0 | 1 forces register-staged | LDS-DMA for A/B runs.
  const bool use_dma = k.impl < 0 ? km : (k.impl == 1 || k.impl == 4);
  return padded(plan_128(a, use_dma ? TUTEL_GEMM_GLDS_128 : TUTEL_GEMM_STAGED_128, km));
}

