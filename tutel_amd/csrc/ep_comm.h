// ep_comm.h -- what the pipeline (ep.hip) needs from the transports (ep_comm.hip).  Internal: not part of the C ABI.
#pragma once
#include <rccl/rccl.h>

#include "common.h"

#define HIP_CHECK(call, what)                                                           \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess) {                                                             \
      tutel_set_error("%s: %s", what, hipGetErrorString(e_));                           \
      return (int)e_;                                                                   \
    }                                                                                   \
  } while (0)

// stage markers: every C-ABI entry point opens a roctx range named after its stage (StageScope, api.hip), so the
// calls below show up as tutel_amd.fast_encode / all_to_all_* / expert_fc1 / expert_fc2 / fast_decode in a marker trace
struct Range {
  explicit Range(const char *name) { tutel_amd_range_push(name); }
  ~Range() { tutel_amd_range_pop(); }
};

// ---- communicator: RCCL comm + the communication stream + the event table -------------------------------
#define EP_MAX_SPLIT 32  // AllToAllStatus.max_num_split of the reference (custom_kernel.cpp:328)
struct tutel_amd_ep_segment;
struct tutel_amd_ep_comm {
  ncclComm_t comm;
  int world, rank, device;
  tutel_amd_exchange_fn hosted;  // bring-up / test communicator: the exchange is a host callback (comm == nullptr then)
  tutel_amd_exchange_v_fn hosted_v;
  void *hosted_user;

  // The GEMMs of the overlapped pipeline run on a side stream (the collectives on the caller's).  HIP multiplexes streams onto a
  // few hardware queues PER PRIORITY LEVEL, and two streams that share a queue run strictly one after the other: every fourth
  // normal-priority stream created in a process lands on the default stream's queue and would then never overlap with it
  // (measured on MI355X, tools/stream_concurrency_check.py, profiles/r03_stream_queues.txt).  Streams of different priority never
  // share a queue, so the communicator owns THREE side streams -- highest, lowest and normal priority -- and a call uses the two
  // whose priority differs from its caller's stream: stage i of the pipeline runs on side stream i % 2, so that the GEMMs of two
  // stages (each a half-chip grid of 128 workgroups at the expert-parallel shapes) run side by side.
  hipStream_t side_stream;      // highest priority
  hipStream_t side_stream_low;  // lowest priority
  hipStream_t side_stream_mid;  // normal priority (used only when the caller's stream is one of the other two)
  hipEvent_t recv_ev[EP_MAX_SPLIT], done_ev[EP_MAX_SPLIT];

  // IPC transport (tutel_amd_ep_comm_attach_ipc): flag words in every rank's flag segment, epoch counters, error word
  tutel_amd_ep_segment *flag_seg;  // [2 directions][EP_FLAG_SLOTS][EP_MAX_PEERS] uint32 per rank, peer-mapped
  uint32_t *epochs;                // device: signalled[2][EP_FLAG_SLOTS], expected[2][EP_FLAG_SLOTS], then ONE error word (see err_word)
  int *err_host, *err_dev;         // pinned + mapped: a wait kernel that gave up leaves its error code here (ep_err_code)
  unsigned selfcheck_seq;          // tutel_amd_ep_ipc_selfcheck: calls so far (tags the pattern)
  long long timeout_ticks;         // of the 100 MHz wall clock
};

// ---- IPC segments: device memory of this rank that every peer of the node maps into its own address space -------------
#define EP_MAX_PEERS 16
#define EP_FLAG_SLOTS (EP_MAX_SPLIT + 1)  // one flag slot per pipeline stage + one for tutel_amd_ep_ipc_exchange
struct tutel_amd_ep_segment {
  void *local;
  size_t bytes;
  int world, rank, device;
  void *peer[EP_MAX_PEERS];    // peer[rank] == local; the others come from hipIpcOpenMemHandle
  uint64_t *tab_dev;           // device copy of peer[]: what the peer-store kernels index by destination rank
  size_t canary_off;           // data segments: byte offset of the epoch canaries behind the user bytes (0: none -- flag segments)
};

// ---- ep_comm.hip, described where they are defined (hidden: short names that stay out of the library's symbol table) ----------
#pragma GCC visibility push(hidden)
void side_streams_for(tutel_amd_ep_comm *c, hipStream_t caller, hipStream_t out[2]);
int exchange(tutel_amd_ep_comm *c, const void *send, void *recv, size_t bytes_per_peer, int world, hipStream_t st, int stage = TUTEL_STAGE_OTHER);
int ipc_check(tutel_amd_ep_comm *c, const char *what);
// what a producer of this rank passes to its kernel for (dir, slot): nullptr epoch = canaries off
PeerCanary producer_canary(const tutel_amd_ep_comm *c, const tutel_amd_ep_segment *seg, int dir, int slot);
int ipc_signal(tutel_amd_ep_comm *c, int dir, int stage0, int nstages, hipStream_t st);
int ipc_wait(tutel_amd_ep_comm *c, int dir, int stage0, int nstages, hipStream_t st, const tutel_amd_ep_segment *seg = nullptr);
int ipc_poison(tutel_amd_ep_comm *c, void *y, size_t n32, hipStream_t st);
#pragma GCC visibility pop
