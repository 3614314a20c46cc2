"""HIP-graph capture of the MoE forward (inference).

With capacity_factor > 0 the forward path never synchronises with the host (the dropless mode's
one `int(capacity)` is the only sync the API implies), and every HIP kernel is enqueued on the
caller's current stream through the C ABI -- so the whole layer, routing to combine, can be captured
once and replayed with zero per-step host work:

    graphed = GraphedForward(layer, example_input)     # captures on a side stream
    y = graphed(x)                                     # copies x into the static input, replays

The static input/output buffers are owned by the wrapper; `y` is valid until the next call.

Dropless layers (capacity_factor <= 0) are captured on the packed layout only (csrc/dropless.hip: every buffer and grid sized by a
host bound, the capacity kept on the device), and only when asked for:

    graphed = GraphedForward(layer, example_input, capacity_factor=0.0, dropless_packed=True)

Replays then serve batches of any expert load, bit for bit what the eager padded dropless forward computes.  Both expert types
take it: `ffn`, and SwiGLU (`llama_ffn`, with the fused gate/up GEMM).  Experts with `fp8_weights` are captured reading FP8 when
`layer.dropless_packed_fp8` is on (impls/packed_w8.py; the warm-up forwards cache the quantised images), else on their 16-bit weights.

GraphedForward is forward-only.  A dropless TRAINING step of `ffn` experts (ReLU; bf16 / fp16 parameters, or fp32 masters under autocast) on the packed layout
(`layer.dropless_packed = True`, impls/packed_train.py) needs no host synchronisation in its forward or backward either, so
forward + backward are captured with plain torch.cuda.graph.  Warm up on a side stream BEFORE any eager step on the default
stream (the layer keeps `l_aux`, whose autograd graph would hold gradient-accumulation nodes of the default stream):

    s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()                                 # zero grads (set to None), y = layer(static_x), loss.backward()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    static_x.copy_(x); g.replay()                  # the parameters' .grad hold this batch's gradients

The same recipe captures the step of fp32 master weights under autocast (examples/helloworld_amp.py): put `with
torch.autocast("cuda", dtype=...)` around the forward and the loss INSIDE step().  The packed step casts its 16-bit compute copies
from the masters inside the captured forward, on every replay, and its weight / bias gradients are fp32 -- so an optimizer step
on the masters between replays (outside the graph, or captured after the backward) is seen by the next replay.

Gradient accumulation over micro-batches (`layer.dropless_packed_main_grad = True` after `packed_train.attach_main_grads(layer)`):
capture ONE micro-step -- step() above, forward + loss.backward(), with the switch on -- and replay it once per micro-batch; the
gradient kernels add into the expert parameters' fp32 `main_grad` on every replay.  Then run the optimizer on `main_grad`, eagerly:

    packed_train.zero_main_grads(layer)            # a plain memset: outside the graph, or captured in a graph of its own
    for x in micro_batches:
        static_x.copy_(x); g.replay()              # main_grad += this batch's dW1, db1, dW2, db2 (the expert .grad stay None)
    optimizer_step_on_main_grad()                  # eager; then zero_main_grads again

The `main_grad` tensors are allocated once and their addresses never change, so the captured kernels keep accumulating into
them: nothing else is needed -- no re-capture, no copies.  (Do not re-assign `p.main_grad` after the capture; zero it in place.
The warm-up steps and the capture itself accumulate too: zero before the first replay.)  The router's weight and x keep their
ordinary gradients, which hold the LAST replay's values as before."""
import torch


class GraphedForward:
    def __init__(self, layer, example, warmup=3, dropless_packed=False, **forward_kwargs):
        assert example.is_cuda, "HIP-graph capture needs a device tensor"
        if forward_kwargs.get("capacity_factor", getattr(layer.gates[0], "capacity_factor", 1.0)) <= 0 and not dropless_packed:
            raise ValueError("dropless routing (capacity_factor <= 0) reads the capacity back to the host and cannot be captured "
                             "(pass dropless_packed=True for the packed layout)")
        # what the forward will run (MOELayer.forward: capacity_factor or the gate's own)
        gate = layer.gates[forward_kwargs.get("gate_index", 0)]
        dropless = (forward_kwargs.get("capacity_factor") or getattr(gate, "capacity_factor", 1.0)) <= 0
        self.layer, self.kwargs = layer, forward_kwargs
        packed_before = getattr(layer, "dropless_packed", False)
        if dropless:
            layer.dropless_packed = True
        try:
            self._capture(layer, example, warmup, dropless, forward_kwargs)
        finally:
            if dropless:
                layer.dropless_packed = packed_before

    def _capture(self, layer, example, warmup, dropless, forward_kwargs):
        self._ep = getattr(layer, "world_size", 1) > 1
        self.static_in = example.clone()
        self.stream = torch.cuda.Stream(device=example.device)
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.no_grad(), torch.cuda.stream(self.stream):
            for i in range(max(warmup, 1) if dropless else warmup):
                layer(self.static_in, **forward_kwargs)
                ran = layer.__dict__.get("_dropless_packed_ran")
                if dropless and i == 0 and ran is not True:
                    torch.cuda.synchronize()
                    raise ValueError("GraphedForward: this dropless forward cannot take the packed layout: " +
                                     (ran or "it does not run through the one-call native path (autocast, training, batch-prioritised "
                                             "routing, a non-gshard loss, fp32 or custom experts ...)"))
            torch.cuda.synchronize()
            # W > 1: only the IPC transport (plain kernels + events, epochs counted on the device) replays safely.  Captured RCCL
            # collectives replay ~200-400 times and then never complete (RCCL 2.26.6 in torch 2.10, profiles/r03_ep_streams.txt):
            # refuse instead of handing out a graph that hangs (TUTEL_AMD_GRAPH_RCCL=1 overrides, for probing)
            if getattr(layer, "world_size", 1) > 1:
                import os
                from . import ep_native
                comm = ep_native.communicator(layer.group, example.device) if ep_native.group_ok(layer.group) else None
                if (comm is None or not comm.ipc) and os.environ.get("TUTEL_AMD_GRAPH_RCCL", "0") != "1":
                    raise RuntimeError("GraphedForward: an expert-parallel layer can only be captured with the IPC transport "
                                       "(peer stores; TUTEL_AMD_EP_TRANSPORT=auto|ipc): replaying captured RCCL collectives hangs")
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=self.stream):
                self.static_out = layer(self.static_in, **forward_kwargs)
        # the captured kernels hold raw pointers into the layer's cached pipeline workspaces (impls/ep_native.py keeps an LRU of
        # them): pin the ones alive now for as long as this graph lives, so that eviction cannot free memory a replay writes
        self._pinned = list(layer.__dict__.get("_ep_workspaces", {}).values())
        self.l_aux = getattr(self.static_out, "l_aux", None)
        torch.cuda.current_stream().wait_stream(self.stream)

    def __call__(self, x):
        # a replay makes no library call, so nothing would ever report an exchange of the IPC transport that gave up (a peer that
        # never arrived, rows behind their flag): ask before every replay -- one read of a pinned host word.  The
        # replay that gave up has poisoned its own output with NaN on the device (csrc/ep_comm.hip::ep_poison_kernel).
        if self._ep:
            from . import ep_native
            ep_native.ipc_status(self.layer.group, self.static_in.device)
        if x.data_ptr() != self.static_in.data_ptr():
            self.static_in.copy_(x)
        self.graph.replay()
        return self.static_out
