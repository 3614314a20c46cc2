// ep.hip -- the expert-parallel pipeline of the MoE forward behind ONE native call.
//
//   fast_encode -> all-to-all -> expert FFN (2 grouped GEMMs) -> all-to-all -> fast_decode
//
// The reference drives its overlapped exchange from C++ on a PRIVATE NCCL communicator with an event
// table and a pooled communication stream (tutel/custom/custom_kernel.cpp:341-365 unique id + init,
// :433-461 streams / events, :520-654 async scatter / gather, one Python call per chunk).  Round 1 of
// this repo drove the same pipeline from Python through torch.distributed: ~20 enqueues per forward
// and 0.32-0.46 ms of host time against 0.2 ms of GPU work per rank.  Here:
//   * the transports -- an RCCL communicator of our own, or peer stores over xGMI with no collective on the hot path at
//     all (the IPC transport) -- are ep_comm.hip; ep_comm.h is what this file uses of them;
//   * one call enqueues the whole pipeline on two HIP streams -- ncclAllToAll on the caller's stream, the
//     GEMMs of the overlapped stages on a side stream owned by the communicator -- with events from a
//     table created once; the call returns after enqueueing (no Python in between) and the whole call can
//     be captured in a HIP graph (the caller's stream is the capture origin, where RCCL can be captured);
//   * the stage layouts are those of tutel_amd/impls/overlap.py::OverlapPlan (expert-sliced when
//     a2a_ffn_overlap_degree divides the local expert count, capacity-chunked otherwise); the GEMMs
//     address the raw exchange buffers, so there are no permute copies (communicate.py:606-622) and no
//     torch.cat; tutel_amd_ep_plan() exposes the arithmetic so a CPU test pins it to the Python plan;
//   * degree 1 is the same plan with one stage, issued on the caller's stream alone: the same schedule, whose fork and
//     join do nothing when a stage's stream is the caller's;
//   * world size 1 without a communicator: the exchange is the identity (stage buffers alias), and
//     with is_postscore the first GEMM gathers its rows from the tokens (fused fast_encode).
// Every step is one of the C-ABI entry points of this library; this file adds orchestration only.
#include "ep_comm.h"
#include "routing_dev.h"


// ---- stage layouts (== tutel_amd/impls/overlap.py::OverlapPlan) ------------------------------------------------
extern "C" int tutel_amd_ep_plan(int E, int W, int capacity, int degree, int allow_sliced, tutel_amd_ep_plan_t *out) {
  TUTEL_REQUIRE(out != nullptr && E >= 1 && W >= 1 && E % W == 0 && degree >= 1 && degree <= EP_MAX_SPLIT && capacity >= 0,
                "tutel_amd_ep_plan: bad sizes E=%d W=%d C=%d degree=%d", E, W, capacity, degree);
  const int E_loc = E / W;
  out->sliced = (allow_sliced && E_loc >= degree && E_loc % degree == 0) ? 1 : 0;
  if (out->sliced) {
    out->experts_per_stage = E_loc / degree;
    out->chunk = capacity;
  } else {
    TUTEL_REQUIRE(capacity % degree == 0, "tutel_amd_ep_plan: capacity %d is not a multiple of a2a_ffn_overlap_degree %d", capacity, degree);
    out->experts_per_stage = E_loc;
    out->chunk = capacity / degree;
  }
  out->rows = out->experts_per_stage * out->chunk;  // bucket rows per (stage, rank) block
  out->gemm_rows = W * out->chunk;                  // GEMM rows per expert and stage
  return 0;
}

// ---- the expert stage of the single-rank routes ------------------------------------------------------------------------------
// fc1 of a single rank without a bucket array: X [T, M] gathered through the slot map (fast_encode fused) -> hid [E, C, H], with the
// megablocks row counts where the caller gave some.  idx8 != NULL: fused location, the kernel works out the slot map and `loc` [n]
// itself (loc == NULL: the eligibility query)
static GemmProblem stage_fc1(const tutel_amd_ep_args_t &a, const uint8_t *idx8, int n, int32_t *loc) {
  GemmProblem g;
  g.A = a.x; g.lda = a.M;
  g.W = a.w1; g.w_stride_e = (int64_t)a.H * a.M; g.ldw = a.M; g.bias = a.b1; g.bias_stride_e = a.H;
  g.D = a.hid; g.d_stride_e = (int64_t)a.capacity * a.H; g.ldd = a.H;
  g.E_loc = a.num_experts; g.N = a.H; g.K = a.M; g.dtype = a.dtype;
  g.row_counts = a.row_counts; g.row_align = a.row_counts != nullptr && a.row_align >= 1 ? a.row_align : 1;
  gemm_one_rank(g, a.capacity);
  gemm_gather(g, a.slot_map, a.T, a.zero_row);
  g.fl_idx8 = idx8; g.fl_n = n; g.fl_loc = loc;
  return g;
}
// fc1 -> activation -> fc2 into a.send [E, C, M_out]: one persistent launch where the shape takes it (expert_ffn.hip), else the two
// GEMM launches.  fc2's problem is looked at only after fc1 has been enqueued.  idx8 != NULL: fc1 with the fused location
static int expert_stage(const tutel_amd_ep_args_t &a, const uint8_t *idx8, int n, hipStream_t st) {
  const int C = a.capacity, H = a.H, Mo = a.M_out;
  const GemmProblem fc1 = stage_fc1(a, idx8, n, idx8 != nullptr ? const_cast<int32_t *>(a.loc) : nullptr);
  GemmProblem fc2;
  fc2.A = a.hid; fc2.a_stride_e = (int64_t)C * H; fc2.lda = H;
  fc2.W = a.w2; fc2.w_stride_e = (int64_t)H * Mo; fc2.ldw = a.w2_kmajor ? H : Mo; fc2.bias = a.b2; fc2.bias_stride_e = Mo;
  fc2.D = a.send; fc2.d_stride_e = (int64_t)C * Mo; fc2.ldd = Mo;
  fc2.E_loc = a.num_experts; fc2.N = Mo; fc2.K = H; fc2.dtype = a.dtype;
  fc2.row_counts = fc1.row_counts; fc2.row_align = fc1.row_align;
  gemm_one_rank(fc2, C);
  int rc = TUTEL_AMD_ENOTSUP;
  if (a.row_counts == nullptr && a.w2_kmajor) {
    Range r("tutel_amd.expert_ffn");
    rc = tutel_expert_ffn(fc1, fc2, a.act, 0, st);
    if (rc != 0 && rc != TUTEL_AMD_ENOTSUP) return rc;
  }
  if (rc == TUTEL_AMD_ENOTSUP) {
    Range r("tutel_amd.expert_fc1");
    rc = tutel_expert_gemm(fc1, 1, a.act, st);
    if (rc) return rc;
    Range r2("tutel_amd.expert_fc2");
    rc = tutel_expert_gemm(fc2, a.w2_kmajor, TUTEL_ACT_NONE, st);
  }
  return rc;
}

// ---- the pipeline ---------------------------------------------------------------------------------------------
extern "C" int tutel_amd_ep_forward(tutel_amd_ep_comm_t *c, const tutel_amd_ep_args_t *a, tutel_stream_t stream) {
  TUTEL_REQUIRE(a != nullptr, "tutel_amd_ep_forward: null arguments");
  const int W = a->world, E = a->num_experts, C = a->capacity, T = a->T, M = a->M, H = a->H, Mo = a->M_out, k = a->k;
  TUTEL_REQUIRE(W >= 1 && E >= 1 && E % W == 0 && T >= 0 && M >= 1 && H >= 1 && Mo >= 1 && k >= 1 && C >= 0,
                "tutel_amd_ep_forward: bad sizes");
  TUTEL_REQUIRE(c == nullptr ? W == 1 : c->world == W, "tutel_amd_ep_forward: communicator world size does not match (%d)", W);
  TUTEL_REQUIRE(a->dtype == TUTEL_BF16 || a->dtype == TUTEL_F16, "tutel_amd_ep_forward: bf16 / fp16 experts only (got dtype %d)", a->dtype);
  TUTEL_REQUIRE((T == 0 || (a->x && a->idx && a->loc && a->y)) && (a->slot_map || C == 0) && a->w1 && a->w2, "tutel_amd_ep_forward: null pointer");
  // a rank without tokens still owes its peers every collective of the pipeline (they block in ncclAllToAll otherwise):
  // only a single rank without a communicator may leave here.  With a communicator the empty rank encodes all-zero
  // buckets, runs its experts on what the others send and skips nothing but its own (empty) decode.
  if (T == 0 && c == nullptr) return 0;
  const int E_loc = E / W, es = 2;
  hipStream_t cur = (hipStream_t)stream;
  const void *enc_gates = a->is_postscore ? nullptr : a->gates;  // fast_dispatch.py:125,131: gates on one side only
  const void *dec_gates = a->is_postscore ? a->gates : nullptr;
  TUTEL_REQUIRE(a->gates != nullptr || T == 0, "tutel_amd_ep_forward: null gates");
  TUTEL_REQUIRE(a->row_counts == nullptr || (W == 1 && c == nullptr && a->degree <= 1), "tutel_amd_ep_forward: row counts (megablocks) need a single rank");

  if (C == 0) {  // nothing is dispatched (on any rank: the capacity is agreed): every token's output is the zero vector
    if (T > 0) HIP_CHECK(hipMemsetAsync(a->y, 0, (size_t)T * Mo * es, cur), "hipMemsetAsync");
    return 0;
  }

  // single rank, no communicator, pure-copy encode: fc1 gathers its rows from the tokens (no bucket array at all)
  if (c == nullptr && a->degree <= 1 && a->is_postscore && a->fuse_encode) {
    TUTEL_REQUIRE(a->hid && a->send && a->zero_row, "tutel_amd_ep_forward: null workspace");
    const int rc = expert_stage(*a, nullptr, 0, cur);
    if (rc) return rc;
    Range r("tutel_amd.fast_decode");
    return tutel_amd_fast_decode(a->send, a->dtype, a->idx, a->loc, dec_gates, a->gate_dtype, T, Mo, k, C, E, 0, 0, 1, a->y, cur);
  }

  const bool ipc = a->peer_seg != nullptr;
  TUTEL_REQUIRE(a->recv && a->hid && a->back && (ipc || (a->enc && a->send)), "tutel_amd_ep_forward: null workspace");
  TUTEL_REQUIRE(a->row_counts == nullptr, "tutel_amd_ep_forward: row counts need the fused-encode single-rank route (is_postscore, fuse_encode)");
  const int degree = a->degree < 1 ? 1 : a->degree;
  tutel_amd_ep_plan_t pl;
  if (tutel_amd_ep_plan(E, W, C, degree, a->allow_sliced, &pl) != 0) return -1;
  const int s = pl.experts_per_stage, cc = pl.chunk, rows = pl.rows, R = pl.gemm_rows;
  const int chunk_rows = pl.sliced ? 0 : cc, expert_slice = pl.sliced ? s : 0;
  int rc;

  const size_t msg_in = (size_t)W * rows * M * es, msg_out = (size_t)W * rows * Mo * es;  // bytes per stage
  const size_t hid_stage = (size_t)s * R * H * es;
  // IPC transport: where the receive / return arrays sit inside every rank's segment (the same offsets on every rank)
  const tutel_amd_ep_segment *seg = a->peer_seg;
  long long recv_off = 0, back_off = 0;
  if (ipc) {
    if (ipc_check(c, "tutel_amd_ep_forward") != 0) return -1;
    TUTEL_REQUIRE(seg->tab_dev != nullptr && seg->world == W && seg->rank == c->rank, "tutel_amd_ep_forward: the peer segment is not open for this communicator");
    recv_off = (const char *)a->recv - (const char *)seg->local;
    back_off = (const char *)a->back - (const char *)seg->local;
    TUTEL_REQUIRE(recv_off >= 0 && back_off >= 0 && (size_t)recv_off + degree * msg_in <= seg->bytes && (size_t)back_off + degree * msg_out <= seg->bytes &&
                      recv_off % 16 == 0 && back_off % 16 == 0,
                  "tutel_amd_ep_forward: recv / back must lie inside the peer segment");
  }
  auto stage_gemms = [&](int i, hipStream_t st) -> int {
    // GEMM rows addressed in the raw exchange buffer: expert el of the stage, source rank w, row l -> ((w*s + el)*cc + l)
    const char *recv_i = (const char *)a->recv + (size_t)i * msg_in;
    char *hid_i = (char *)a->hid + (size_t)i * hid_stage;
    const int e0 = pl.sliced ? i * s : 0;  // first local expert of the stage
    const char *w1 = (const char *)a->w1 + (size_t)e0 * H * M * es, *w2 = (const char *)a->w2 + (size_t)e0 * H * Mo * es;
    const char *b1 = a->b1 ? (const char *)a->b1 + (size_t)e0 * H * es : nullptr, *b2 = a->b2 ? (const char *)a->b2 + (size_t)e0 * Mo * es : nullptr;
    GemmProblem fc1, fc2;
    fc1.A = recv_i; fc1.a_stride_e = (int64_t)cc * M; fc1.a_stride_w = (int64_t)rows * M; fc1.a_rows_per_w = cc; fc1.lda = M;
    fc1.W = w1; fc1.w_stride_e = (int64_t)H * M; fc1.ldw = M; fc1.bias = b1; fc1.bias_stride_e = H;
    fc1.D = hid_i; fc1.d_stride_e = (int64_t)R * H; fc1.d_rows_per_w = R; fc1.ldd = H;
    fc1.E_loc = s; fc1.R = R; fc1.N = H; fc1.K = M; fc1.dtype = a->dtype;
    {
      Range r("tutel_amd.expert_fc1");
      tutel_stage_hint(TUTEL_STAGE_FC1);
      const int r1 = tutel_expert_gemm(fc1, 1, a->act, st);
      tutel_stage_hint(-1);
      if (r1) return r1;
    }
    Range r("tutel_amd.expert_fc2");
    fc2.A = hid_i; fc2.a_stride_e = (int64_t)R * H; fc2.a_rows_per_w = R; fc2.lda = H;
    fc2.W = w2; fc2.w_stride_e = (int64_t)H * Mo; fc2.ldw = a->w2_kmajor ? H : Mo; fc2.bias = b2; fc2.bias_stride_e = Mo;
    fc2.d_stride_e = (int64_t)cc * Mo; fc2.d_rows_per_w = cc; fc2.ldd = Mo;
    fc2.E_loc = s; fc2.R = R; fc2.N = Mo; fc2.K = H; fc2.dtype = a->dtype;
    const PeerCanary can = producer_canary(ipc ? c : nullptr, seg, 1, i);  // (fc2.d_can points at it: it must outlive the call)
    if (ipc) {  // rows of source rank w go straight to block <my rank> of stage i of rank w's return array
      fc2.d_peer = seg->tab_dev; fc2.d_peer_off = back_off + (long long)(((size_t)i * W + c->rank) * rows * Mo * es); fc2.d_can = &can;
    } else {
      fc2.D = (char *)a->send + (size_t)i * msg_out; fc2.d_stride_w = (int64_t)rows * Mo;
    }
    return tutel_expert_gemm(fc2, a->w2_kmajor, TUTEL_ACT_NONE, st);
  };
  // stage i's bucket rows: plain launch into `enc`, or (IPC) peer stores into the owners' receive arrays
  auto encode_stage = [&](int i, int nst) -> int {
    Range r("tutel_amd.fast_encode");
    EncodePeer pe = {ipc ? seg->tab_dev : nullptr, recv_off, ipc ? c->rank : 0, rows, i * W * rows, producer_canary(ipc ? c : nullptr, seg, 0, i)};
    return tutel_encode_launch(a->x, a->dtype, a->slot_map, enc_gates, a->gate_dtype, T, M, (i + nst) * W * rows, C, E, chunk_rows, expert_slice, W,
                               ipc ? nullptr : a->enc, pe, cur);
  };

  // Forked side streams are joined back on EVERY exit from here on: an early return between a fork and its join would
  // leave the caller's stream unordered against work still running on a side stream -- and, under HIP-graph capture, an unjoined
  // fork (capture then fails at hipStreamEndCapture instead of here, with the real error lost).
  struct ForkGuard {
    hipStream_t cur;
    hipStream_t forked[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    void fork(int slot, hipStream_t ks, hipEvent_t join_ev) { forked[slot] = ks; ev[slot] = join_ev; }
    // every forked stream back into the caller's; the first error, after trying them all
    hipError_t join() {
      hipError_t first = hipSuccess;
      for (int j = 0; j < 2; ++j) {
        if (forked[j] == nullptr) continue;
        hipError_t e = hipEventRecord(ev[j], forked[j]);
        if (e == hipSuccess) e = hipStreamWaitEvent(cur, ev[j], 0);
        if (first == hipSuccess) first = e;
        forked[j] = nullptr;
      }
      return first;
    }
    ~ForkGuard() {
      (void)join();
      tutel_gemm_corun_hint(0);
    }
  } guard{cur};

  // ---- one schedule for both transports and every degree.  Stage i's GEMMs run on kss[i % 2]: the caller's stream (degree 1, or
  // no communicator: fork and join are nothing then -- no event, no wait, no entry in the guard), else the communicator's side
  // streams, so that stage i + 1 is on the links while stage i is in the GEMMs and stage i - 1 travels back.
  //   collective: the COLLECTIVES stay on the caller's stream and the GEMMs go to the communicator's side stream: the
  //     caller's stream is the origin of a HIP-graph capture, and RCCL can be captured there but not on a stream that
  //     joined the capture through an event (segfault inside the library, tools/graph_rccl_probe.py) -- plain kernel
  //     launches are fine on either.  Eager and captured execution take this one path.
  //   IPC: no collective, no send / enc staging arrays.  Per stage: encode (peer stores) -> signal | wait -> fc1 -> fc2 (peer
  //     stores) -> signal; then one wait for every stage's return rows and decode.
  hipStream_t kss[2] = {cur, cur};
  if (degree > 1 && c != nullptr) side_streams_for(c, cur, kss);
  const bool side = kss[0] != cur;
  // Two stages side by side: a stage GEMM whose full grid would be one workgroup per CU takes the half-chip 256 x 256 grid
  // instead (gemm_plan.hip), so that fc1 / fc2 of stage i overlap those of stage i + 1 (IPC: two distinct side streams) or a
  // real collective beside them (the hosted test exchange is synchronous) rather than queueing behind them block by block
  const bool corun = tutel_get_option(TUTEL_OPT_EP_STAGE_GRID) != 0 && (ipc ? kss[0] != kss[1] : side && c->comm != nullptr);

  // dispatch, on the caller's stream: every stage's rows leave, recv_ev[i] marks where stage i's are on their way
  auto dispatched = [&](int i) -> int {
    if (side) HIP_CHECK(hipEventRecord(c->recv_ev[i], cur), "hipEventRecord");
    return 0;
  };
  if (ipc) {
    for (int i = 0; i < degree; ++i) {
      if ((rc = encode_stage(i, 1)) != 0) return rc;
      {
        StageScope sc(TUTEL_STAGE_A2A_DISPATCH, cur);
        if ((rc = ipc_signal(c, 0, i, 1, cur)) != 0) return rc;
      }
      if ((rc = dispatched(i)) != 0) return rc;
    }
  } else {
    if ((rc = encode_stage(0, degree)) != 0) return rc;
    Range r(side ? "tutel_amd.all_to_all(dispatch)" : "tutel_amd.all_to_all");
    for (int i = 0; i < degree; ++i) {
      rc = exchange(c, (const char *)a->enc + (size_t)i * msg_in, (char *)a->recv + (size_t)i * msg_in, (size_t)rows * M * es, W, cur, TUTEL_STAGE_A2A_DISPATCH);
      if (rc != 0 || (rc = dispatched(i)) != 0) return rc;
    }
  }
  // The ENQUEUE order stays stage by stage; the device runs by dependencies, not by enqueue order: stage i + 1 on the other
  // stream only waits for its own recv event.
  for (int i = 0; i < degree; ++i) {
    hipStream_t ks = kss[i & 1];
    if (side) {  // the side stream forks from the caller's
      HIP_CHECK(hipStreamWaitEvent(ks, c->recv_ev[i], 0), "hipStreamWaitEvent");
      guard.fork(i & 1, ks, c->done_ev[i]);
    }
    if (ipc) {
      StageScope sc(TUTEL_STAGE_A2A_DISPATCH, ks);
      if ((rc = ipc_wait(c, 0, i, 1, ks, seg)) != 0) return rc;
    }
    tutel_gemm_corun_hint(corun);
    rc = stage_gemms(i, ks);
    tutel_gemm_corun_hint(0);
    if (rc) return rc;
    if (ipc) {  // the return rows are fc2's own peer stores: the streams stay forked until every stage has signalled
      StageScope sc(TUTEL_STAGE_A2A_COMBINE, ks);
      if ((rc = ipc_signal(c, 1, i, 1, ks)) != 0) return rc;
    } else {
      // GEMMs of stage i, join, return exchange of stage i: every RCCL call is captured with all forked streams joined back
      // (RCCL cannot be captured next to an open fork, tools/graph_rccl_probe.py)
      HIP_CHECK(guard.join(), "tutel_amd_ep_forward (join)");
      Range r(side ? "tutel_amd.all_to_all(combine)" : "tutel_amd.all_to_all");
      rc = exchange(c, (const char *)a->send + (size_t)i * msg_out, (char *)a->back + (size_t)i * msg_out, (size_t)rows * Mo * es, W, cur, TUTEL_STAGE_A2A_COMBINE);
      if (rc) return rc;
    }
  }
  HIP_CHECK(guard.join(), "tutel_amd_ep_forward (join)");
  if (ipc) {
    StageScope sc(TUTEL_STAGE_A2A_COMBINE, cur);
    if ((rc = ipc_wait(c, 1, 0, degree, cur, seg)) != 0) return rc;
  }
  Range r("tutel_amd.fast_decode");
  rc = tutel_amd_fast_decode(a->back, a->dtype, a->idx, a->loc, dec_gates, a->gate_dtype, T, Mo, k, C, E, chunk_rows, expert_slice, W, a->y, cur);
  if (rc != 0 || !ipc || T == 0) return rc;
  // a forward whose exchange gave up must not hand out rows that never arrived: NaNs instead (one load when all is well)
  StageScope sc(TUTEL_STAGE_DECODE, cur);
  return ipc_poison(c, a->y, (size_t)T * Mo * es / 4, cur);
}

// ---- routing + pipeline in one call ------------------------------------------------------------------------------
// internal (common.h): the routing launches both one-call forwards (this one and dropless.hip's packed one) make after their own checks
int tutel_route_launch(const tutel_amd_moe_args_t &m, int splits, int32_t *slot_map, tutel_stream_t stream) {
  const tutel_amd_ep_args_t &a = m.ep;
  const int T = a.T, E = a.num_experts, k = a.k, clear_n = slot_map != nullptr ? E * a.capacity : 0;
  int rc;
  if (splits > 0) {  // the gate projection inside the call (gate_proj.hip)
    rc = tutel_gate_proj_for(a.x, m.gate_w, a.dtype, m.logits_dtype, T, a.M, E, m.gate_partials, m.gate_partial_bytes, stream);
    if (rc) return rc;
    rc = tutel_amd_gate_topk_partials(m.gate_partials, splits, m.logits_dtype, T, E, k, m.normalize_gate, m.logits_out, nullptr,
                                      const_cast<int32_t *>(a.idx), const_cast<void *>(a.gates), m.ws, m.ws_bytes, slot_map, clear_n, stream);
  } else {
    rc = tutel_amd_gate_topk(m.logits, m.logits_dtype, 1, T, E, k, m.normalize_gate, nullptr, const_cast<int32_t *>(a.idx),
                             const_cast<void *>(a.gates), m.ws, m.ws_bytes, slot_map, clear_n, stream);
  }
  if (rc) return rc;
  return tutel_amd_compute_location(a.idx, T, E, k, 1, m.ws, m.ws_bytes, const_cast<int32_t *>(a.loc), m.dispatch_count, m.stats, m.l_aux,
                                    m.logits_dtype, slot_map != nullptr ? a.capacity : 0, slot_map, slot_map != nullptr ? 1 : 0, stream);
}

extern "C" int tutel_amd_moe_forward(tutel_amd_ep_comm_t *c, const tutel_amd_moe_args_t *m, tutel_stream_t stream) {
  GemmPlanScope scope;
  TUTEL_REQUIRE(m != nullptr, "tutel_amd_moe_forward: null arguments");
  const tutel_amd_ep_args_t &a = m->ep;
  const int T = a.T, E = a.num_experts, k = a.k;
  const bool project = m->logits == nullptr && m->gate_w != nullptr;  // the gate projection inside the call (gate_proj.hip)
  TUTEL_REQUIRE((m->logits != nullptr || project || T == 0) && m->ws != nullptr && m->dispatch_count != nullptr, "tutel_amd_moe_forward: null pointer");
  int splits = 0;
  if (project && T > 0) {
    TUTEL_REQUIRE(a.dtype == m->logits_dtype || gate_proj_mixed(a.dtype, m->logits_dtype), "tutel_amd_moe_forward: the in-call gate projection needs the gate in the token dtype (%d vs %d)", m->logits_dtype, a.dtype);
    splits = tutel_gate_proj_splits_for(T, a.M, E, a.dtype, m->logits_dtype);
    TUTEL_REQUIRE(splits > 0, "tutel_amd_moe_forward: the in-call gate projection does not cover T=%d, M=%d, E=%d, dtype=%d (pass logits)", T, a.M, E, a.dtype);
    TUTEL_REQUIRE(a.x != nullptr && m->gate_partials != nullptr && m->gate_partial_bytes >= (size_t)splits * T * E * sizeof(float),
                  "tutel_amd_moe_forward: gate_partials must hold %d x %d x %d floats", splits, T, E);
  }
  TUTEL_REQUIRE(a.slot_map && (T == 0 || (a.idx && a.loc && a.gates)), "tutel_amd_moe_forward: null routing buffers");
  if (T == 0 && c == nullptr) return 0;  // (with a communicator an empty rank still takes part in every exchange, see tutel_amd_ep_forward)
  const bool dropless = a.capacity <= 0;
  TUTEL_REQUIRE(!dropless || (c == nullptr && a.world == 1 && m->stats != nullptr && m->capacity_out != nullptr && m->max_capacity >= 1),
                "tutel_amd_moe_forward: dropless routing needs a single rank, stats, capacity_out and max_capacity");
  int32_t *smap = const_cast<int32_t *>(a.slot_map);
  int rc;
  // ---- fused location (see expert_gemm_big_kernel<.., FL>): no location launch between the top-k kernel and the first expert GEMM
  const int Mo = a.M_out;
  bool fl = !dropless && c == nullptr && a.world == 1 && a.degree <= 1 && a.is_postscore && a.fuse_encode && T > 0 && k <= 8 && E <= 128 &&
            (long long)k * T <= 15360 && m->fl_ws != nullptr && m->fl_ws_bytes >= (((size_t)k * T + 15) & ~(size_t)15) &&
            (a.dtype == TUTEL_BF16 || a.dtype == TUTEL_F16) && a.row_counts == nullptr && a.hid && a.send && a.zero_row && a.loc && a.w1 &&
            ((uintptr_t)m->fl_ws & 15) == 0;
  // the fused-location branch calls tutel_gate_topk_launch directly, i.e. past the public entry point's argument checks: the same
  // ones here (a C caller with an undersized `ws` got an out-of-bounds device write instead of an error)
  if (fl) {
    TUTEL_REQUIRE(k >= 1 && k <= E, "tutel_amd_moe_forward: need 1 <= k <= E (got k=%d, E=%d)", k, E);
    TUTEL_REQUIRE(m->ws_bytes >= tutel_amd_routing_workspace_bytes(T, E, k), "tutel_amd_moe_forward: routing workspace too small (%zu bytes, need %zu)",
                  m->ws_bytes, tutel_amd_routing_workspace_bytes(T, E, k));
    // eligibility query (loc == NULL: nothing is launched); a "no" is an answer, not an error -- last_error keeps what it held
    char keep[512];
    strncpy(keep, tutel_amd_last_error(), sizeof(keep) - 1);
    keep[sizeof(keep) - 1] = 0;
    fl = tutel_expert_gemm(stage_fc1(a, (const uint8_t *)m->fl_ws, k * T, nullptr), 1, a.act, (hipStream_t)stream) == 0;
    if (!fl && !gemm_plan_asked()) tutel_set_error("%s", keep);
  }
  if (gemm_plan_asked(1)) {  // tutel_amd_expert_gemm_plan_next: out[0] holds the query's plan (or its refusal); out[1]: the fc1 launch after a yes
    if (fl) (void)tutel_expert_gemm(stage_fc1(a, (const uint8_t *)m->fl_ws, k * T, const_cast<int32_t *>(a.loc)), 1, a.act, (hipStream_t)stream);
    return fl ? 0 : TUTEL_AMD_ENOTSUP;
  }
  if (fl) {
    hipStream_t st = (hipStream_t)stream;
    uint8_t *idx8 = (uint8_t *)m->fl_ws;
    if (project) {
      rc = tutel_gate_proj_for(a.x, m->gate_w, a.dtype, m->logits_dtype, T, a.M, E, m->gate_partials, m->gate_partial_bytes, stream);
      if (rc) return rc;
    }
    rc = tutel_gate_topk_launch(project ? nullptr : m->logits, project ? m->gate_partials : nullptr, splits, m->logits_dtype, T, E, k,
                                m->normalize_gate, project ? m->logits_out : nullptr, const_cast<int32_t *>(a.idx), const_cast<void *>(a.gates),
                                m->ws, nullptr, 0, idx8, st);
    if (rc) return rc;
    if (m->capacity_out != nullptr) *m->capacity_out = a.capacity;
    rc = expert_stage(a, idx8, k * T, st);
    if (rc) return rc;
    Range r("tutel_amd.fast_decode");
    RouteFinish fin;
    tutel_route_finish_args(T, E, k, m->ws, &fin);
    fin.on = 1;
    fin.dispatch_count = m->dispatch_count;
    fin.stats = m->stats;
    fin.l_aux = m->l_aux;
    fin.l_aux_dtype = m->logits_dtype;
    return tutel_decode_finish_launch(a.send, a.dtype, a.idx, a.loc, a.gates, m->logits_dtype, T, Mo, k, a.capacity, E, a.y, fin, st);
  }
  rc = tutel_route_launch(*m, splits, dropless ? nullptr : smap, stream);
  if (rc) return rc;
  tutel_amd_ep_args_t e = a;
  e.gate_dtype = m->logits_dtype;
  if (dropless) {
    // the one host synchronisation of the dropless API (fast_dispatch.py:192-193), taken here so that nothing but this
    // function stands between the read-back and the next launch
    // the read-back lands in the caller's own slot (m->capacity_out: any host memory; pinned memory makes the copy
    // asynchronous, pageable memory makes the runtime stage it) -- no process-global state, so callers on different
    // threads / streams / devices cannot read each other's capacity
    hipStream_t st = (hipStream_t)stream;
    HIP_CHECK(hipMemcpyAsync(m->capacity_out, m->stats, sizeof(int), hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
    HIP_CHECK(hipStreamSynchronize(st), "hipStreamSynchronize");
    int cap = *m->capacity_out;
    if (m->capacity_limit > 0 && cap > m->capacity_limit) cap = m->capacity_limit;
    const int al = m->alignment >= 1 ? m->alignment : 1;
    cap = (cap + al - 1) / al * al;
    *m->capacity_out = cap;
    if (cap > m->max_capacity) return TUTEL_AMD_EAGAIN;
    if (cap == 0) return hipMemsetAsync(a.y, 0, (size_t)T * a.M_out * 2, st) == hipSuccess ? 0 : -1;
    rc = tutel_amd_slot_map(a.idx, a.loc, T, E, k, cap, smap, stream);
    if (rc) return rc;
    e.capacity = cap;
  } else if (m->capacity_out != nullptr) {
    *m->capacity_out = a.capacity;
  }
  return tutel_amd_ep_forward(c, &e, stream);
}
