// ep_comm.hip -- the transports of the expert-parallel pipeline (ep.hip): what moves the bucket rows between the ranks.
//   * an RCCL communicator of our own (ncclCommInitRank from an id the host code broadcasts), resolved
//     with dlopen from the RCCL already in the process (torch ships one): no link-time dependency; with it the side
//     streams and the event table of the pipeline, and the variable-size collectives of tutel.net;
//   * round 4 -- the MI355X-native exchange: xGMI is load / store addressable between the GPUs of a node, so with the IPC
//     transport (tutel_amd_ep_segment_* + tutel_amd_ep_comm_attach_ipc) there is NO collective on the hot path at all:
//     fast_encode writes every bucket row straight into the receive buffer of the rank that owns the expert, the second
//     expert GEMM's epilogue writes every output row straight into the return buffer of the rank the row came from, and
//     one flag word per (direction, stage, peer) -- written by a one-workgroup kernel after the producing kernel, polled
//     by a one-workgroup kernel before the consuming one -- replaces the four ncclAllToAll enqueues (4 x ~30 us of host
//     time), their copy kernels (which hold CUs beside the stage GEMMs) and the send / back staging arrays.  Plain kernel
//     launches and events only: HIP-graph replay safe (the epoch counters live in device memory).
#include <dlfcn.h>
#include <stdlib.h>

#include <vector>

#include "ep_comm.h"

// ---- RCCL, resolved at run time -------------------------------------------------------------
struct RcclApi {
  void *handle;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *);
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int);
  ncclResult_t (*CommDestroy)(ncclComm_t);
  ncclResult_t (*AllToAll)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t);
  const char *(*GetErrorString)(ncclResult_t);
  ncclResult_t (*GroupStart)();
  ncclResult_t (*GroupEnd)();
  ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
  ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
};
static RcclApi g_rccl = {};

extern "C" int tutel_amd_ep_load_rccl(const char *path) {
  if (g_rccl.handle != nullptr) return 0;
  void *h = nullptr;
  // the copy already mapped into the process first (same HIP runtime as the caller's tensors), then the hint, then the loader path
  const char *sonames[] = {"librccl.so.1", "librccl.so"};
  for (const char *n : sonames)
    if (h == nullptr) h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
  if (h == nullptr && path != nullptr && path[0] != 0) h = dlopen(path, RTLD_NOW | RTLD_GLOBAL);
  for (const char *n : sonames)
    if (h == nullptr) h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
  TUTEL_REQUIRE(h != nullptr, "tutel_amd_ep_load_rccl: cannot load librccl (%s)", dlerror());
  RcclApi a;
  a.handle = h;
  a.GetUniqueId = (decltype(a.GetUniqueId))dlsym(h, "ncclGetUniqueId");
  a.CommInitRank = (decltype(a.CommInitRank))dlsym(h, "ncclCommInitRank");
  a.CommDestroy = (decltype(a.CommDestroy))dlsym(h, "ncclCommDestroy");
  a.AllToAll = (decltype(a.AllToAll))dlsym(h, "ncclAllToAll");
  a.GetErrorString = (decltype(a.GetErrorString))dlsym(h, "ncclGetErrorString");
  a.GroupStart = (decltype(a.GroupStart))dlsym(h, "ncclGroupStart");
  a.GroupEnd = (decltype(a.GroupEnd))dlsym(h, "ncclGroupEnd");
  a.Send = (decltype(a.Send))dlsym(h, "ncclSend");
  a.Recv = (decltype(a.Recv))dlsym(h, "ncclRecv");
  TUTEL_REQUIRE(a.GetUniqueId && a.CommInitRank && a.CommDestroy && a.AllToAll && a.GetErrorString && a.GroupStart && a.GroupEnd && a.Send && a.Recv,
                "tutel_amd_ep_load_rccl: librccl lacks ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclAllToAll / ncclSend / ncclRecv / ncclGroupStart / ncclGroupEnd");
  g_rccl = a;
  return 0;
}

#define RCCL_CHECK(call, what)                                                          \
  do {                                                                                  \
    ncclResult_t r_ = (call);                                                           \
    if (r_ != ncclSuccess) {                                                            \
      tutel_set_error("%s: RCCL error %d (%s)", what, (int)r_, g_rccl.GetErrorString(r_)); \
      return (int)r_ ? (int)r_ : -1;                                                    \
    }                                                                                   \
  } while (0)

// epoch canaries (common.h: PeerCanary): uint32 [2 directions][EP_FLAG_SLOTS][EP_MAX_PEERS source ranks][EP_NCAN]
#define EP_CANARY_WORDS (2 * EP_FLAG_SLOTS * EP_MAX_PEERS * EP_NCAN)
static inline size_t canary_word(int dir, int slot, int src) { return ((size_t)(dir * EP_FLAG_SLOTS + slot) * EP_MAX_PEERS + src) * EP_NCAN; }

// ---- communicator (struct tutel_amd_ep_comm, ep_comm.h): RCCL comm + the side streams + the event table ------------------
static bool create_side_streams(tutel_amd_ep_comm *c) {
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return false;
  return hipStreamCreateWithPriority(&c->side_stream, hipStreamNonBlocking, greatest) == hipSuccess &&
         hipStreamCreateWithPriority(&c->side_stream_low, hipStreamNonBlocking, least) == hipSuccess &&
         hipStreamCreateWithPriority(&c->side_stream_mid, hipStreamNonBlocking, (least + greatest) / 2) == hipSuccess;
}

// the two side streams whose priority differs from the caller's (see struct tutel_amd_ep_comm); TUTEL_OPT_EP_STREAMS = 1: one
void side_streams_for(tutel_amd_ep_comm *c, hipStream_t caller, hipStream_t out[2]) {
  int least = 0, greatest = 0, pr = 0;
  out[0] = c->side_stream;
  out[1] = c->side_stream_low;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && hipStreamGetPriority(caller, &pr) == hipSuccess && least != greatest) {
    if (pr == greatest) out[0] = c->side_stream_mid;
    else if (pr == least) out[1] = c->side_stream_mid;
  }
  if (tutel_get_option(TUTEL_OPT_EP_STREAMS) == 1) out[1] = out[0];
}

extern "C" int tutel_amd_ep_unique_id(void *out, size_t bytes) {
  TUTEL_REQUIRE(out != nullptr && bytes >= sizeof(ncclUniqueId), "tutel_amd_ep_unique_id: need a %zu-byte buffer", sizeof(ncclUniqueId));
  if (tutel_amd_ep_load_rccl(nullptr) != 0) return -1;
  ncclUniqueId id;
  RCCL_CHECK(g_rccl.GetUniqueId(&id), "ncclGetUniqueId");
  memcpy(out, &id, sizeof(id));
  return 0;
}

extern "C" int tutel_amd_ep_comm_create(const void *id, size_t bytes, int world, int rank, tutel_amd_ep_comm_t **out) {
  TUTEL_REQUIRE(out != nullptr && world >= 1 && rank >= 0 && rank < world, "tutel_amd_ep_comm_create: bad world / rank %d / %d", world, rank);
  TUTEL_REQUIRE(id != nullptr && bytes >= sizeof(ncclUniqueId), "tutel_amd_ep_comm_create: need the %zu-byte id of tutel_amd_ep_unique_id", sizeof(ncclUniqueId));
  if (tutel_amd_ep_load_rccl(nullptr) != 0) return -1;
  tutel_amd_ep_comm *c = (tutel_amd_ep_comm *)calloc(1, sizeof(tutel_amd_ep_comm));
  TUTEL_REQUIRE(c != nullptr, "tutel_amd_ep_comm_create: out of memory");
  c->world = world;
  c->rank = rank;
  // every failure below releases what was created so far (tutel_amd_ep_comm_destroy tolerates the zeroed fields)
  auto fail = [&](int rc) {
    (void)tutel_amd_ep_comm_destroy(c);
    return rc;
  };
  if (hipGetDevice(&c->device) != hipSuccess) {
    tutel_set_error("tutel_amd_ep_comm_create: hipGetDevice failed");
    return fail(-1);
  }
  ncclUniqueId uid;
  memcpy(&uid, id, sizeof(uid));
  ncclResult_t nr = g_rccl.CommInitRank(&c->comm, world, uid, rank);
  if (nr != ncclSuccess) {
    c->comm = nullptr;
    tutel_set_error("ncclCommInitRank: RCCL error %d (%s)", (int)nr, g_rccl.GetErrorString(nr));
    return fail((int)nr);
  }
  bool ok = create_side_streams(c);
  for (int i = 0; ok && i < EP_MAX_SPLIT; ++i)
    ok = hipEventCreateWithFlags(&c->recv_ev[i], hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&c->done_ev[i], hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    tutel_set_error("tutel_amd_ep_comm_create: cannot create the side stream / event table: %s", hipGetErrorString(hipGetLastError()));
    return fail(-1);
  }
  *out = c;
  return 0;
}

extern "C" int tutel_amd_ep_comm_create_hosted(int world, int rank, tutel_amd_exchange_fn fn, void *user, tutel_amd_ep_comm_t **out) {
  TUTEL_REQUIRE(out != nullptr && fn != nullptr && world >= 1 && rank >= 0 && rank < world, "tutel_amd_ep_comm_create_hosted: bad arguments");
  tutel_amd_ep_comm *c = (tutel_amd_ep_comm *)calloc(1, sizeof(tutel_amd_ep_comm));
  TUTEL_REQUIRE(c != nullptr, "tutel_amd_ep_comm_create_hosted: out of memory");
  c->world = world;
  c->rank = rank;
  c->hosted = fn;
  c->hosted_user = user;
  bool ok = hipGetDevice(&c->device) == hipSuccess && create_side_streams(c);
  for (int i = 0; ok && i < EP_MAX_SPLIT; ++i)
    ok = hipEventCreateWithFlags(&c->recv_ev[i], hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&c->done_ev[i], hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    tutel_set_error("tutel_amd_ep_comm_create_hosted: cannot create the side stream / event table");
    (void)tutel_amd_ep_comm_destroy(c);
    return -1;
  }
  *out = c;
  return 0;
}

// A communicator with neither RCCL nor a host callback: the IPC transport (tutel_amd_ep_comm_attach_ipc) is its only
// exchange -- ranks that share one GPU (RCCL refuses those), or a node where RCCL is not wanted on the path at all.
extern "C" int tutel_amd_ep_comm_create_ipc(int world, int rank, tutel_amd_ep_comm_t **out) {
  TUTEL_REQUIRE(out != nullptr && world >= 1 && world <= EP_MAX_PEERS && rank >= 0 && rank < world,
                "tutel_amd_ep_comm_create_ipc: bad world / rank %d / %d (at most %d ranks: one node)", world, rank, EP_MAX_PEERS);
  tutel_amd_ep_comm *c = (tutel_amd_ep_comm *)calloc(1, sizeof(tutel_amd_ep_comm));
  TUTEL_REQUIRE(c != nullptr, "tutel_amd_ep_comm_create_ipc: out of memory");
  c->world = world;
  c->rank = rank;
  bool ok = hipGetDevice(&c->device) == hipSuccess && create_side_streams(c);
  for (int i = 0; ok && i < EP_MAX_SPLIT; ++i)
    ok = hipEventCreateWithFlags(&c->recv_ev[i], hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&c->done_ev[i], hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    tutel_set_error("tutel_amd_ep_comm_create_ipc: cannot create the side streams / event table");
    (void)tutel_amd_ep_comm_destroy(c);
    return -1;
  }
  *out = c;
  return 0;
}

extern "C" int tutel_amd_ep_comm_destroy(tutel_amd_ep_comm_t *c) {
  if (c == nullptr) return 0;
  if (c->side_stream != nullptr) (void)hipStreamSynchronize(c->side_stream);
  if (c->side_stream_low != nullptr) (void)hipStreamSynchronize(c->side_stream_low);
  if (c->side_stream_mid != nullptr) (void)hipStreamSynchronize(c->side_stream_mid);
  if (c->comm != nullptr && g_rccl.CommDestroy != nullptr) (void)g_rccl.CommDestroy(c->comm);
  if (c->side_stream != nullptr) (void)hipStreamDestroy(c->side_stream);
  if (c->side_stream_low != nullptr) (void)hipStreamDestroy(c->side_stream_low);
  if (c->side_stream_mid != nullptr) (void)hipStreamDestroy(c->side_stream_mid);
  for (int i = 0; i < EP_MAX_SPLIT; ++i) {
    if (c->recv_ev[i] != nullptr) (void)hipEventDestroy(c->recv_ev[i]);
    if (c->done_ev[i] != nullptr) (void)hipEventDestroy(c->done_ev[i]);
  }
  if (c->epochs != nullptr) (void)hipFree(c->epochs);
  if (c->err_host != nullptr) (void)hipHostFree(c->err_host);
  free(c);  // (the flag segment belongs to the caller: tutel_amd_ep_segment_free)
  return 0;
}

extern "C" int tutel_amd_ep_comm_info(const tutel_amd_ep_comm_t *c, int *world, int *rank) {
  TUTEL_REQUIRE(c != nullptr, "tutel_amd_ep_comm_info: null communicator");
  if (world) *world = c->world;
  if (rank) *rank = c->rank;
  return 0;
}

// equal-split all-to-all of `bytes_per_peer` bytes per rank pair on `stream` (all_to_all_single semantics,
// communicate.py:181-192): block r of `send` goes to rank r and lands as block (my rank) of its `recv`
int exchange(tutel_amd_ep_comm *c, const void *send, void *recv, size_t bytes_per_peer, int world, hipStream_t st, int stage) {
  if (bytes_per_peer == 0) return 0;
  // single rank without a communicator: the exchange is the identity -- nothing to do when the caller aliased the stage
  // buffers (impls/ep_native.py does), a copy otherwise
  if (c == nullptr && send == recv) return 0;
  StageScope scope(stage, st);
  if (c == nullptr) {
    HIP_CHECK(hipMemcpyAsync(recv, send, bytes_per_peer * (size_t)world, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync");
    return 0;
  }
  if (c->hosted != nullptr) {  // bring-up / test communicator
    const int rc = c->hosted(c->hosted_user, send, recv, bytes_per_peer, world);
    TUTEL_REQUIRE(rc == 0, "tutel_amd_ep_forward: the host exchange callback failed (%d)", rc);
    return 0;
  }
  TUTEL_REQUIRE(c->comm != nullptr, "tutel_amd_ep: this communicator has only the IPC transport (buffers must live in a segment: tutel_amd_ep_ipc_exchange)");
  if ((bytes_per_peer & 1) == 0)
    RCCL_CHECK(g_rccl.AllToAll(send, recv, bytes_per_peer / 2, ncclFloat16, c->comm, st), "ncclAllToAll");
  else
    RCCL_CHECK(g_rccl.AllToAll(send, recv, bytes_per_peer, ncclInt8, c->comm, st), "ncclAllToAll");
  return 0;
}

extern "C" int tutel_amd_ep_all_to_all(tutel_amd_ep_comm_t *c, const void *send, void *recv, size_t bytes_per_peer,
                                       tutel_stream_t stream) {
  TUTEL_REQUIRE(c != nullptr && send != nullptr && recv != nullptr && send != recv, "tutel_amd_ep_all_to_all: need a communicator and two distinct buffers");
  return exchange(c, send, recv, bytes_per_peer, c->world, (hipStream_t)stream);
}

// ---- variable-size exchanges (tutel.net.batch_all_to_all_v / batch_all_gather_v; custom_kernel.cpp:463-518) -----------
extern "C" int tutel_amd_ep_comm_set_hosted_v(tutel_amd_ep_comm_t *c, tutel_amd_exchange_v_fn fn) {
  TUTEL_REQUIRE(c != nullptr && c->hosted != nullptr, "tutel_amd_ep_comm_set_hosted_v: need a hosted communicator");
  c->hosted_v = fn;
  return 0;
}

// one grouped send / recv loop: to rank r `sb[r]` bytes from send + so[r], from rank r `rb[r]` bytes into the running offset
static int exchange_v(tutel_amd_ep_comm *c, const void *send, void *recv, const uint64_t *sb, const uint64_t *so, const uint64_t *rb,
                      hipStream_t st, const char *what) {
  StageScope scope(TUTEL_STAGE_OTHER, st);
  if (c->hosted != nullptr) {
    TUTEL_REQUIRE(c->hosted_v != nullptr, "%s: the hosted communicator has no variable-size callback (tutel_amd_ep_comm_set_hosted_v)", what);
    const int rc = c->hosted_v(c->hosted_user, send, recv, sb, so, rb, c->world);
    TUTEL_REQUIRE(rc == 0, "%s: the host exchange callback failed (%d)", what, rc);
    return 0;
  }
  TUTEL_REQUIRE(c->comm != nullptr, "%s: this communicator has only the IPC transport", what);
  RCCL_CHECK(g_rccl.GroupStart(), "ncclGroupStart");
  uint64_t ro = 0;
  ncclResult_t bad = ncclSuccess;
  for (int r = 0; r < c->world && bad == ncclSuccess; ++r) {
    if (sb[r]) bad = g_rccl.Send((const char *)send + so[r], (size_t)sb[r], ncclInt8, r, c->comm, st);
    if (rb[r] && bad == ncclSuccess) bad = g_rccl.Recv((char *)recv + ro, (size_t)rb[r], ncclInt8, r, c->comm, st);
    ro += rb[r];
  }
  const ncclResult_t end = g_rccl.GroupEnd();  // always closed, also after a failed send / recv
  RCCL_CHECK(bad, what);
  RCCL_CHECK(end, "ncclGroupEnd");
  return 0;
}

extern "C" int tutel_amd_ep_all_to_all_v(tutel_amd_ep_comm_t *c, const void *send, void *recv, const uint64_t *send_bytes,
                                         const uint64_t *recv_bytes, tutel_stream_t stream) {
  TUTEL_REQUIRE(c != nullptr && send_bytes != nullptr && recv_bytes != nullptr, "tutel_amd_ep_all_to_all_v: need a communicator and both size arrays");
  std::vector<uint64_t> so((size_t)c->world);
  uint64_t tot_s = 0, tot_r = 0;
  for (int r = 0; r < c->world; ++r) {
    so[r] = tot_s;
    tot_s += send_bytes[r];
    tot_r += recv_bytes[r];
  }
  TUTEL_REQUIRE((send != nullptr || tot_s == 0) && (recv != nullptr || tot_r == 0) && (send != recv || tot_s + tot_r == 0),
                "tutel_amd_ep_all_to_all_v: null or aliased buffers");
  return exchange_v(c, send, recv, send_bytes, so.data(), recv_bytes, (hipStream_t)stream, "tutel_amd_ep_all_to_all_v");
}

extern "C" int tutel_amd_ep_all_gather_v(tutel_amd_ep_comm_t *c, const void *send, void *recv, const uint64_t *recv_bytes,
                                         tutel_stream_t stream) {
  TUTEL_REQUIRE(c != nullptr && recv_bytes != nullptr, "tutel_amd_ep_all_gather_v: need a communicator and the size array");
  std::vector<uint64_t> sb((size_t)c->world), so((size_t)c->world);
  uint64_t tot_r = 0;
  for (int r = 0; r < c->world; ++r) {
    sb[r] = recv_bytes[c->rank];  // the same bytes to everybody
    so[r] = 0;
    tot_r += recv_bytes[r];
  }
  TUTEL_REQUIRE((send != nullptr || recv_bytes[c->rank] == 0) && (recv != nullptr || tot_r == 0) && (send != recv || tot_r == 0),
                "tutel_amd_ep_all_gather_v: null or aliased buffers");
  return exchange_v(c, send, recv, sb.data(), so.data(), recv_bytes, (hipStream_t)stream, "tutel_amd_ep_all_gather_v");
}

// ---- IPC transport ------------------------------------------------------------------------------------------------
// Replaces the exchange kernels of ncclAllToAll (custom_kernel.cpp:559-579, 627-648: one ncclSend / ncclRecv pair per peer and
// chunk) by stores of the producing kernels themselves.  Memory model: a producer's stores into a peer's segment become visible
// at its kernel boundary (end-of-kernel release to system scope); the flag is written by the NEXT kernel on the same stream, so
// it can never overtake the data; the consumer polls the flag with system-scope loads in a kernel of its own and the consuming
// kernel starts after that kernel's boundary (start-of-kernel acquire).  No fence inside a bandwidth kernel, no in-kernel spin
// in a kernel that holds more than one wave.
//
// Buffer reuse needs no credits: rank r overwrites rank w's receive array in forward n + 1 only after its own decode of forward
// n, which waited for w's stage flags of forward n, which w wrote after its GEMMs had read that array; and w overwrites r's
// return array in forward n + 1 only after its fc1 waited for r's dispatch flag of forward n + 1, which r wrote after its
// decode of forward n had read the return array.  Every rank calls the same forwards in the same order (SPMD), on one stream
// at a time per communicator.
extern "C" int tutel_amd_ep_segment_alloc(size_t bytes, int flag_memory, tutel_amd_ep_segment_t **out, void *handle_out, size_t handle_bytes) {
  TUTEL_REQUIRE(out != nullptr && bytes >= 1, "tutel_amd_ep_segment_alloc: bad arguments");
  TUTEL_REQUIRE(handle_out == nullptr || handle_bytes >= sizeof(hipIpcMemHandle_t), "tutel_amd_ep_segment_alloc: the handle needs %zu bytes", sizeof(hipIpcMemHandle_t));
  tutel_amd_ep_segment *sg = (tutel_amd_ep_segment *)calloc(1, sizeof(tutel_amd_ep_segment));
  TUTEL_REQUIRE(sg != nullptr, "tutel_amd_ep_segment_alloc: out of memory");
  sg->bytes = bytes;
  sg->world = 1;
  const char *what = "hipGetDevice";   // the call that failed, for the message (ranks sharing one device have shown transient failures here)
  hipError_t e = hipGetDevice(&sg->device);
  if (e == hipSuccess) {
    e = hipErrorInvalidValue;
    // flag words are polled while other agents write them: uncached device memory where the runtime has it (what RCCL uses for
    // its own peer flags), fine-grained next, plain device memory last (the polls are system-scope loads either way)
    what = "hipExtMallocWithFlags / hipMalloc";
    if (flag_memory) e = hipExtMallocWithFlags(&sg->local, bytes, hipDeviceMallocUncached);
    if (e != hipSuccess && flag_memory) e = hipExtMallocWithFlags(&sg->local, bytes, hipDeviceMallocFinegrained);
    if (e != hipSuccess && flag_memory) e = hipMalloc(&sg->local, bytes);
    if (!flag_memory) {
      // data segment: the epoch canaries live behind the user bytes, in the SAME allocation (same memory type, same mapping in
      // every peer) -- they are only meaningful if they travel the way the rows do
      sg->canary_off = (bytes + 255) / 256 * 256;
      what = "hipMalloc";
      e = hipMalloc(&sg->local, sg->canary_off + (size_t)EP_CANARY_WORDS * sizeof(uint32_t));
      if (e == hipSuccess) { what = "hipMemset"; e = hipMemset((char *)sg->local + sg->canary_off, 0, (size_t)EP_CANARY_WORDS * sizeof(uint32_t)); }
      if (e == hipSuccess) { what = "hipDeviceSynchronize"; e = hipDeviceSynchronize(); }
    }
  }
  if (e == hipSuccess && flag_memory) {
    what = "hipMemset";
    e = hipMemset(sg->local, 0, bytes);
    if (e == hipSuccess) { what = "hipDeviceSynchronize"; e = hipDeviceSynchronize(); }
  }
  if (e == hipSuccess && handle_out != nullptr) {
    hipIpcMemHandle_t h;
    what = "hipIpcGetMemHandle";
    e = hipIpcGetMemHandle(&h, sg->local);
    if (e == hipSuccess) memcpy(handle_out, &h, sizeof(h));
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    tutel_set_error("tutel_amd_ep_segment_alloc: %s: %s", what, hipGetErrorString(e));
    if (sg->local != nullptr) (void)hipFree(sg->local);
    free(sg);
    return (int)e;
  }
  sg->peer[0] = sg->local;
  *out = sg;
  return 0;
}

extern "C" int tutel_amd_ep_segment_open(tutel_amd_ep_segment_t *sg, int world, int rank, const void *handles, size_t handle_bytes) {
  TUTEL_REQUIRE(sg != nullptr && world >= 1 && world <= EP_MAX_PEERS && rank >= 0 && rank < world, "tutel_amd_ep_segment_open: bad world / rank %d / %d (at most %d ranks)", world, rank, EP_MAX_PEERS);
  TUTEL_REQUIRE(sg->tab_dev == nullptr, "tutel_amd_ep_segment_open: the segment is open already");
  TUTEL_REQUIRE(world == 1 || (handles != nullptr && handle_bytes >= sizeof(hipIpcMemHandle_t)), "tutel_amd_ep_segment_open: need %d handles", world);
  sg->world = world;
  sg->rank = rank;
  for (int w = 0; w < EP_MAX_PEERS; ++w) sg->peer[w] = nullptr;
  sg->peer[rank] = sg->local;
  for (int w = 0; w < world; ++w) {
    if (w == rank) continue;
    hipIpcMemHandle_t h;
    memcpy(&h, (const char *)handles + (size_t)w * handle_bytes, sizeof(h));
    const hipError_t e = hipIpcOpenMemHandle(&sg->peer[w], h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      sg->peer[w] = nullptr;
      tutel_set_error("tutel_amd_ep_segment_open: hipIpcOpenMemHandle of rank %d's segment failed: %s", w, hipGetErrorString(e));
      for (int v = 0; v < w; ++v)
        if (v != rank && sg->peer[v] != nullptr) {
          (void)hipIpcCloseMemHandle(sg->peer[v]);
          sg->peer[v] = nullptr;
        }
      return (int)e;
    }
  }
  uint64_t tab[EP_MAX_PEERS];
  for (int w = 0; w < EP_MAX_PEERS; ++w) tab[w] = (uint64_t)(uintptr_t)sg->peer[w < world ? w : rank];
  HIP_CHECK(hipMalloc((void **)&sg->tab_dev, sizeof(tab)), "hipMalloc");
  HIP_CHECK(hipMemcpy(sg->tab_dev, tab, sizeof(tab), hipMemcpyHostToDevice), "hipMemcpy");
  return 0;
}

extern "C" void *tutel_amd_ep_segment_ptr(const tutel_amd_ep_segment_t *sg, int peer) {
  if (sg == nullptr) return nullptr;
  if (peer < 0) return sg->local;
  return peer < EP_MAX_PEERS ? sg->peer[peer] : nullptr;
}

// bytes [off, off + bytes) of the LOCAL segment -> `dst` (device), enqueued on `stream`: how host code that owns no tensor over
// the segment (it is library memory) looks at what the peers stored
extern "C" int tutel_amd_ep_segment_read(const tutel_amd_ep_segment_t *sg, size_t off, void *dst, size_t bytes, tutel_stream_t stream) {
  TUTEL_REQUIRE(sg != nullptr && dst != nullptr && off + bytes <= sg->bytes, "tutel_amd_ep_segment_read: out of range");
  HIP_CHECK(hipMemcpyAsync(dst, (const char *)sg->local + off, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream), "hipMemcpyAsync");
  return 0;
}

extern "C" int tutel_amd_ep_segment_free(tutel_amd_ep_segment_t *sg) {
  if (sg == nullptr) return 0;
  for (int w = 0; w < sg->world && w < EP_MAX_PEERS; ++w)
    if (sg->peer[w] != nullptr && sg->peer[w] != sg->local) (void)hipIpcCloseMemHandle(sg->peer[w]);
  if (sg->tab_dev != nullptr) (void)hipFree(sg->tab_dev);
  if (sg->local != nullptr) (void)hipFree(sg->local);
  free(sg);
  return 0;
}

#define EP_FLAG_WORDS (2 * EP_FLAG_SLOTS * EP_MAX_PEERS)
extern "C" size_t tutel_amd_ep_flag_bytes(void) { return (size_t)EP_FLAG_WORDS * sizeof(uint32_t); }

extern "C" int tutel_amd_ep_comm_attach_ipc(tutel_amd_ep_comm_t *c, tutel_amd_ep_segment_t *flags, int timeout_ms) {
  TUTEL_REQUIRE(c != nullptr && flags != nullptr, "tutel_amd_ep_comm_attach_ipc: null communicator / segment");
  TUTEL_REQUIRE(c->flag_seg == nullptr, "tutel_amd_ep_comm_attach_ipc: the communicator has its flag segment already");
  TUTEL_REQUIRE(flags->tab_dev != nullptr && flags->world == c->world && flags->rank == c->rank && flags->bytes >= tutel_amd_ep_flag_bytes(),
                "tutel_amd_ep_comm_attach_ipc: the flag segment must be opened for this communicator's %d ranks and hold %zu bytes", c->world, tutel_amd_ep_flag_bytes());
  HIP_CHECK(hipMalloc((void **)&c->epochs, (4 * EP_FLAG_SLOTS + 1) * sizeof(uint32_t)), "hipMalloc");
  HIP_CHECK(hipMemset(c->epochs, 0, (4 * EP_FLAG_SLOTS + 1) * sizeof(uint32_t)), "hipMemset");
  HIP_CHECK(hipHostMalloc((void **)&c->err_host, sizeof(int), hipHostMallocMapped), "hipHostMalloc");
  *c->err_host = 0;
  HIP_CHECK(hipHostGetDevicePointer((void **)&c->err_dev, c->err_host, 0), "hipHostGetDevicePointer");
  HIP_CHECK(hipDeviceSynchronize(), "hipDeviceSynchronize");
  c->timeout_ticks = (long long)(timeout_ms > 0 ? timeout_ms : 120000) * 100000LL;  // wall_clock64: 100 MHz
  c->flag_seg = flags;
  return 0;
}

extern "C" int tutel_amd_ep_comm_has_ipc(const tutel_amd_ep_comm_t *c) { return c != nullptr && c->flag_seg != nullptr; }

extern "C" int tutel_amd_ep_ipc_set_timeout(tutel_amd_ep_comm_t *c, int timeout_ms) {
  TUTEL_REQUIRE(c != nullptr && c->flag_seg != nullptr && timeout_ms > 0, "tutel_amd_ep_ipc_set_timeout: need a communicator with the IPC transport and a positive time");
  c->timeout_ticks = (long long)timeout_ms * 100000LL;
  return 0;
}

// one workgroup, thread (i, w) = (stage, peer): flag[dir][stage0 + i][my rank] of rank w := this rank's next epoch for the slot
__global__ void ep_signal_kernel(const uint64_t *__restrict__ flag_tab, uint32_t *__restrict__ epochs, int dir, int stage0,
                                 int nstages, int W, int rank) {
  const int t = threadIdx.x, i = t / W, w = t % W;
  const bool on = i < nstages;
  uint32_t e = 0;
  if (on) e = epochs[dir * EP_FLAG_SLOTS + stage0 + i] + 1u;
  __syncthreads();  // every thread of a stage has read the old epoch before one of them writes the new one
  if (!on) return;
  __threadfence_system();
  uint32_t *f = reinterpret_cast<uint32_t *>(flag_tab[w]) + ((size_t)(dir * EP_FLAG_SLOTS + stage0 + i) * EP_MAX_PEERS + rank);
  __hip_atomic_store(f, e, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  if (w == 0) epochs[dir * EP_FLAG_SLOTS + stage0 + i] = e;
}

// one workgroup, thread (i, w): wait until peer w has signalled this rank's next expected epoch of slot (dir, stage0 + i).
// Every spin is bounded: after timeout_ticks the thread records which (dir, stage, peer) never arrived and gives up.
// error codes left in the communicator's error words: which wait gave up, and why
#define EP_ERR_STALE (1 << 24)  // the flag arrived, the epoch canaries of its producer had not: data behind the flag
__device__ __host__ static inline int ep_err_code(int dir, int stage, int peer, int stale) {
  return ((1 + dir) << 16) | (stage << 8) | peer | (stale ? EP_ERR_STALE : 0);
}
// Every spin is bounded: after timeout_ticks the thread records which (dir, stage, peer) never arrived and gives up.  `canary`
// (optional): this rank's canary words -- once the flag of (stage, peer) is here, the EP_NCAN words its producer stored behind
// its rows must carry the same epoch (system-scope loads: what is in memory, not what an L2 still holds).
__global__ void ep_wait_kernel(const uint32_t *__restrict__ flags, uint32_t *__restrict__ epochs, int dir, int stage0, int nstages,
                               int W, int *err, long long timeout_ticks, const uint32_t *__restrict__ canary) {
  const int t = threadIdx.x, i = t / W, w = t % W;
  const bool on = i < nstages;
  uint32_t *expect = epochs + 2 * EP_FLAG_SLOTS;
  int *err_word = reinterpret_cast<int *>(epochs + 4 * EP_FLAG_SLOTS);  // device copy of the error: what ep_poison_kernel reads
  uint32_t e = 0;
  if (on) e = expect[dir * EP_FLAG_SLOTS + stage0 + i] + 1u;
  __syncthreads();
  if (!on) return;
  const uint32_t *f = flags + ((size_t)(dir * EP_FLAG_SLOTS + stage0 + i) * EP_MAX_PEERS + w);
  const long long t0 = wall_clock64();
  int bad = 0;
  while ((int)(__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - e) < 0) {
    __builtin_amdgcn_s_sleep(20);
    if (wall_clock64() - t0 > timeout_ticks) {
      bad = ep_err_code(dir, stage0 + i, w, 0);
      break;
    }
  }
  if (bad == 0 && canary != nullptr) {
    const uint32_t *cw = canary + ((size_t)(dir * EP_FLAG_SLOTS + stage0 + i) * EP_MAX_PEERS + w) * EP_NCAN;
    uint32_t diff = 0;
#pragma unroll
    for (int j = 0; j < EP_NCAN; ++j) diff |= __hip_atomic_load(cw + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) ^ e;
    if (diff != 0) bad = ep_err_code(dir, stage0 + i, w, 1);
  }
  if (bad != 0) {
    __hip_atomic_store(err, bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(err_word, bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __threadfence_system();
  if (w == 0) expect[dir * EP_FLAG_SLOTS + stage0 + i] = e;
}

// The result of a forward whose exchange gave up (a peer never arrived, or its rows were behind its flag) is not a result: one
// workgroup after fast_decode turns it into NaNs, so that no caller can consume it as one (the call itself has long
// returned 0, and under HIP-graph replay there is no call).  Costs one load when nothing is wrong.
__global__ __launch_bounds__(1024) void ep_poison_kernel(const uint32_t *__restrict__ epochs, uint32_t *__restrict__ y, size_t n32) {
  const int err = *reinterpret_cast<const int *>(epochs + 4 * EP_FLAG_SLOTS);
  if (err == 0) return;
  for (size_t i = threadIdx.x; i < n32; i += 1024) y[i] = 0x7fc07fc0u;  // NaN as bf16 and as fp16 pairs
}
int ipc_poison(tutel_amd_ep_comm *c, void *y, size_t n32, hipStream_t st) {
  hipLaunchKernelGGL(ep_poison_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t *)c->epochs, (uint32_t *)y, n32);
  TUTEL_CHECK_LAUNCH("tutel_amd_ep_forward (poison)");
  return 0;
}

int ipc_check(tutel_amd_ep_comm *c, const char *what) {
  TUTEL_REQUIRE(c != nullptr && c->flag_seg != nullptr, "%s: the communicator has no IPC transport (tutel_amd_ep_comm_attach_ipc)", what);
  const int err = *(volatile int *)c->err_host;
  TUTEL_REQUIRE((err & EP_ERR_STALE) == 0,
                "%s: an earlier exchange saw rank %d's flag BEFORE the rows it announces (%s, stage %d: epoch canaries behind the flag) -- the peer-store "
                "transport is not safe on this system, its outputs since then are poisoned (NaN); use TUTEL_AMD_EP_TRANSPORT=rccl",
                what, err & 0xff, ((err >> 16) & 0xff) == 1 ? "dispatch" : "combine", (err >> 8) & 0xff);
  TUTEL_REQUIRE(err == 0, "%s: an earlier exchange timed out waiting for rank %d (%s, stage %d): a peer died or the ranks disagree about the call sequence; "
                "the outputs of the forwards since then are poisoned (NaN)",
                what, err & 0xff, (err >> 16) == 1 ? "dispatch" : "combine", (err >> 8) & 0xff);
  return 0;
}
PeerCanary producer_canary(const tutel_amd_ep_comm *c, const tutel_amd_ep_segment *seg, int dir, int slot) {
  PeerCanary pc = {nullptr, 0, 0, 0};
  if (c == nullptr || seg == nullptr || seg->canary_off == 0 || c->epochs == nullptr || tutel_get_option(TUTEL_OPT_EP_CANARY) == 0) return pc;
  pc.epoch = c->epochs + dir * EP_FLAG_SLOTS + slot;
  pc.off = (long long)(seg->canary_off + canary_word(dir, slot, c->rank) * sizeof(uint32_t));
  pc.world = c->world;
  pc.stale = tutel_get_option(TUTEL_OPT_EP_CANARY) == 2;  // test injection: every canary of this rank stays one epoch behind
  return pc;
}
int ipc_signal(tutel_amd_ep_comm *c, int dir, int stage0, int nstages, hipStream_t st) {
  hipLaunchKernelGGL(ep_signal_kernel, dim3(1), dim3(nstages * c->world), 0, st, c->flag_seg->tab_dev, c->epochs, dir, stage0, nstages, c->world, c->rank);
  TUTEL_CHECK_LAUNCH("tutel_amd_ep (signal)");
  return 0;
}
// `seg`: the data segment the awaited producers stored into (its canaries are checked once the flags are here); nullptr: flags only
int ipc_wait(tutel_amd_ep_comm *c, int dir, int stage0, int nstages, hipStream_t st, const tutel_amd_ep_segment *seg) {
  const uint32_t *canary = nullptr;
  if (seg != nullptr && seg->canary_off != 0 && tutel_get_option(TUTEL_OPT_EP_CANARY) != 0)
    canary = reinterpret_cast<const uint32_t *>((const char *)seg->local + seg->canary_off);
  hipLaunchKernelGGL(ep_wait_kernel, dim3(1), dim3(nstages * c->world), 0, st, (const uint32_t *)c->flag_seg->local, c->epochs, dir, stage0, nstages,
                     c->world, c->err_dev, c->timeout_ticks, canary);
  TUTEL_CHECK_LAUNCH("tutel_amd_ep (wait)");
  return 0;
}

// block r of `send` (bytes_per_peer bytes, 16-byte granules) -> rank r's segment at recv_off + <my rank> * bytes_per_peer
__global__ __launch_bounds__(256) void ep_peer_copy_kernel(const uint4 *__restrict__ send, const uint64_t *__restrict__ tab, long long recv_off,
                                                          size_t vec_per_peer, int W, int rank, PeerCanary can) {
  const size_t n = vec_per_peer * (size_t)W;
  for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (size_t)gridDim.x * 256) {
    const int w = (int)(v / vec_per_peer);
    const size_t o = v % vec_per_peer;
    reinterpret_cast<uint4 *>(tab[w] + recv_off)[(size_t)rank * vec_per_peer + o] = send[v];
  }
  peer_canary_store(tab, can);
}

// all_to_all_single with equal splits over the IPC transport: `send` is any device buffer of this rank, the result lands at
// byte offset recv_off of every rank's `seg` ([world][bytes_per_peer]); when the call's work completes on `stream` the
// received blocks may be read.  The caller keeps two such exchanges into the same offset apart (a barrier, or any exchange
// in the other direction): there are no credits.
extern "C" int tutel_amd_ep_ipc_exchange(tutel_amd_ep_comm_t *c, tutel_amd_ep_segment_t *seg, const void *send, size_t bytes_per_peer,
                                         size_t recv_off, tutel_stream_t stream) {
  if (ipc_check(c, "tutel_amd_ep_ipc_exchange") != 0) return -1;
  TUTEL_REQUIRE(seg != nullptr && seg->tab_dev != nullptr && seg->world == c->world && seg->rank == c->rank, "tutel_amd_ep_ipc_exchange: the segment is not open for this communicator");
  TUTEL_REQUIRE(bytes_per_peer % 16 == 0 && recv_off % 16 == 0 && ((uintptr_t)send % 16) == 0, "tutel_amd_ep_ipc_exchange: 16-byte granules");
  TUTEL_REQUIRE(recv_off + bytes_per_peer * (size_t)c->world <= seg->bytes, "tutel_amd_ep_ipc_exchange: the blocks do not fit the segment");
  hipStream_t st = (hipStream_t)stream;
  StageScope scope(TUTEL_STAGE_OTHER, st);
  if (bytes_per_peer > 0) {
    TUTEL_REQUIRE(send != nullptr, "tutel_amd_ep_ipc_exchange: null send buffer");
    const size_t vpp = bytes_per_peer / 16, n = vpp * (size_t)c->world;
    const int grid = (int)(n / 256 + 1 > 2048 ? 2048 : n / 256 + 1);
    hipLaunchKernelGGL(ep_peer_copy_kernel, dim3(grid), dim3(256), 0, st, (const uint4 *)send, seg->tab_dev, (long long)recv_off, vpp, c->world, c->rank,
                       producer_canary(c, seg, 0, EP_MAX_SPLIT));
    TUTEL_CHECK_LAUNCH("tutel_amd_ep_ipc_exchange");
  }
  int rc = ipc_signal(c, 0, EP_MAX_SPLIT, 1, st);
  if (rc) return rc;
  return ipc_wait(c, 0, EP_MAX_SPLIT, 1, st, bytes_per_peer > 0 ? seg : nullptr);
}

extern "C" int tutel_amd_ep_ipc_status(tutel_amd_ep_comm_t *c) { return ipc_check(c, "tutel_amd_ep_ipc_status"); }

// ---- payload-sized self-check of the transport (VERDICT r4 / ADVICE r4) --------------------------------------------------------
// What the 4 KB tagged exchange of round 4 could not show: ordering behind a kernel's worth of dirty lines.  Every pass a WRITER
// kernel (grid of 1024 workgroups, 16-byte stores, the store flavour under test) fills block <my rank> of every rank's segment with
// a pattern that names (call, pass, source, destination, position); the signal kernel follows it on the same stream; the wait kernel
// and a READER kernel (plain loads, every vector compared, mismatches counted on the device) follow on the consuming stream -- the
// caller's, or a side stream of the communicator as in the overlapped pipeline -- and an acknowledgement in the other direction
// keeps pass n + 1 from overwriting what a peer is still reading.  No host synchronisation between the passes: the reader of pass
// n has just pulled every line of the segment into its caches when pass n + 1 overwrites them from the other side.
// flavour: 0 plain stores (what the pipeline uses), 1 `sc1`, 2 `sc0 sc1` (system-scope write-through), 3 non-temporal.
template <int FLAVOUR> __device__ __forceinline__ void store16(uint4 *p, uint4 v) {
  typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
  const u32x4_t x = {v.x, v.y, v.z, v.w};
  // (s_nop: an inline-assembly VMEM store is invisible to the compiler's hazard recognizer -- the wait states the ISA demands before
  // a VALU write of the store's data registers are ours to provide; leaving them out is what produced round 4's "stale rows",
  // profiles/r05_two_process_visibility.txt)
  if (FLAVOUR == 1) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(x) : "memory");
  else if (FLAVOUR == 2) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(x) : "memory");
  else if (FLAVOUR == 3) __builtin_nontemporal_store(x, reinterpret_cast<u32x4_t *>(p));
  else *p = v;
}
__device__ __forceinline__ uint4 check_pattern(uint32_t tag, int src, int dst, size_t o) {
  const uint32_t lo = (uint32_t)o;
  return make_uint4(tag, ((uint32_t)src << 16) | (uint32_t)dst, lo, lo * 2654435761u + tag);
}
template <int FLAVOUR>
__global__ __launch_bounds__(256) void ep_check_write_kernel(const uint64_t *__restrict__ tab, long long off, size_t vec_per_peer, int W, int rank,
                                                            uint32_t tag, PeerCanary can) {
  const size_t n = vec_per_peer * (size_t)W;
  for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (size_t)gridDim.x * 256) {
    const int w = (int)(v / vec_per_peer);
    const size_t o = v % vec_per_peer;
    store16<FLAVOUR>(reinterpret_cast<uint4 *>(tab[w] + off) + (size_t)rank * vec_per_peer + o, check_pattern(tag, rank, w, o));
  }
  if (FLAVOUR != 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  peer_canary_store(tab, can);
}
// out[0] = vectors that differ, out[1] = (first) offending position: source rank << 40 | vector index
__global__ __launch_bounds__(256) void ep_check_read_kernel(const uint4 *__restrict__ local, size_t vec_per_peer, int W, int rank, uint32_t tag,
                                                           unsigned long long *__restrict__ out) {
  const size_t n = vec_per_peer * (size_t)W;
  unsigned long long bad = 0, first = ~0ull;
  for (size_t v = (size_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (size_t)gridDim.x * 256) {
    const int w = (int)(v / vec_per_peer);
    const size_t o = v % vec_per_peer;
    const uint4 got = local[v], want = check_pattern(tag, w, rank, o);
    if (got.x != want.x || got.y != want.y || got.z != want.z || got.w != want.w) {
      ++bad;
      if (first == ~0ull) first = ((unsigned long long)w << 40) | (unsigned long long)o;
    }
  }
  if (bad) {
    atomicAdd(out, bad);
    atomicMin(out + 1, first);
  }
}

extern "C" int tutel_amd_ep_ipc_selfcheck(tutel_amd_ep_comm_t *c, tutel_amd_ep_segment_t *seg, size_t bytes_per_peer, int passes, int flavour,
                                          int side_stream, unsigned long long *mismatch, tutel_stream_t stream) {
  if (ipc_check(c, "tutel_amd_ep_ipc_selfcheck") != 0) return -1;
  TUTEL_REQUIRE(seg != nullptr && seg->tab_dev != nullptr && seg->world == c->world && seg->rank == c->rank, "tutel_amd_ep_ipc_selfcheck: the segment is not open for this communicator");
  TUTEL_REQUIRE(bytes_per_peer >= 16 && bytes_per_peer % 16 == 0 && bytes_per_peer * (size_t)c->world <= seg->bytes, "tutel_amd_ep_ipc_selfcheck: %zu bytes per peer do not fit the segment", bytes_per_peer);
  TUTEL_REQUIRE(passes >= 1 && passes <= 255 && flavour >= 0 && flavour <= 3 && mismatch != nullptr, "tutel_amd_ep_ipc_selfcheck: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  hipStream_t kss[2] = {st, st};
  if (side_stream) side_streams_for(c, st, kss);
  hipStream_t rd = kss[0];  // the consuming stream
  const size_t vpp = bytes_per_peer / 16, n = vpp * (size_t)c->world;
  const int grid = (int)(n / 256 + 1 > 1024 ? 1024 : n / 256 + 1);
  const unsigned seq = ++c->selfcheck_seq;
  const int slot = EP_MAX_SPLIT;
  HIP_CHECK(hipMemsetAsync(mismatch, 0, sizeof(unsigned long long), st), "hipMemsetAsync");
  HIP_CHECK(hipMemsetAsync(mismatch + 1, 0xff, sizeof(unsigned long long), st), "hipMemsetAsync");
  int rc = 0;
  for (int p = 0; p < passes && rc == 0; ++p) {
    const uint32_t tag = (seq << 8) | (uint32_t)p;
    // pass p may overwrite the peers' blocks only when every peer has read pass p - 1 (their acknowledgements)
    if (p > 0 && (rc = ipc_wait(c, 1, slot, 1, st)) != 0) break;
    const PeerCanary can = producer_canary(c, seg, 0, slot);
    switch (flavour) {
      case 1: hipLaunchKernelGGL(ep_check_write_kernel<1>, dim3(grid), dim3(256), 0, st, seg->tab_dev, 0LL, vpp, c->world, c->rank, tag, can); break;
      case 2: hipLaunchKernelGGL(ep_check_write_kernel<2>, dim3(grid), dim3(256), 0, st, seg->tab_dev, 0LL, vpp, c->world, c->rank, tag, can); break;
      case 3: hipLaunchKernelGGL(ep_check_write_kernel<3>, dim3(grid), dim3(256), 0, st, seg->tab_dev, 0LL, vpp, c->world, c->rank, tag, can); break;
      default: hipLaunchKernelGGL(ep_check_write_kernel<0>, dim3(grid), dim3(256), 0, st, seg->tab_dev, 0LL, vpp, c->world, c->rank, tag, can);
    }
    TUTEL_CHECK_LAUNCH("tutel_amd_ep_ipc_selfcheck (write)");
    if ((rc = ipc_signal(c, 0, slot, 1, st)) != 0) break;
    if (rd != st) {
      HIP_CHECK(hipEventRecord(c->recv_ev[0], st), "hipEventRecord");
      HIP_CHECK(hipStreamWaitEvent(rd, c->recv_ev[0], 0), "hipStreamWaitEvent");
    }
    if ((rc = ipc_wait(c, 0, slot, 1, rd, seg)) != 0) break;
    hipLaunchKernelGGL(ep_check_read_kernel, dim3(grid), dim3(256), 0, rd, (const uint4 *)seg->local, vpp, c->world, c->rank, tag, mismatch);
    TUTEL_CHECK_LAUNCH("tutel_amd_ep_ipc_selfcheck (read)");
    if ((rc = ipc_signal(c, 1, slot, 1, rd)) != 0) break;
    if (rd != st) {
      HIP_CHECK(hipEventRecord(c->done_ev[0], rd), "hipEventRecord");
      HIP_CHECK(hipStreamWaitEvent(st, c->done_ev[0], 0), "hipStreamWaitEvent");
    }
  }
  if (rc == 0) rc = ipc_wait(c, 1, slot, 1, st);  // the acknowledgements of the last pass: every signal has its wait
  return rc;
}
