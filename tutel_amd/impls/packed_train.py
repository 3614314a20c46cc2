"""A dropless training step of ffn experts on the packed layout: forward AND backward without a host synchronisation.

The padded dropless step (MOELayer's generic path) reads the maximum expert load back to the host to shape [E, C, *] buckets
(extract_critical), and its weight gradients are library batched GEMMs over those buckets.  Here the experts' rows lie back to
back (csrc/dropless.hip), every buffer is sized by the host bound of tutel_amd_packed_plan, and every per-expert extent comes
from the device offsets -- so the whole step, loss.backward() included, can be captured with torch.cuda.graph.

    routing   : top-k + locations (the HIP kernels extract_critical runs) on logits.detach(); the differentiable gates and
                l_aux from the same ATen ops as extract_critical's training branch (fast_dispatch.gates_from_scores)
    layout    : ops.packed_layout -> offsets, tile table, packed slot map, device capacity
    forward   : hid = relu(x[slot] @ W1^T + b1)   (ops.expert_gemm_packed, k-major, rows gathered from the tokens)
                Y   = hid @ W2 + b2               (n-major: W2 [E, H, M_out] as stored)
                y   = sum_j g[j, t] * Y[off[e] + loc]
    backward  : dY   = g * dy scattered to the packed rows (ops.fast_encode through the packed slot map: pad rows are zeros)
                dg   = <dy[t], Y[off[e] + loc]>                       (ops.gate_grad_packed)
                dW2  = hid^T dY, db2 = sum dY                       (ops.expert_wgrad_packed / expert_bgrad_packed)
                dhid = (dY @ W2^T) * [hid > 0]                        (k-major, gated epilogue)
                dW1  = dhid^T x[slot], db1 = sum dhid
                dx   = sum_j (dhid @ W1)[off[e] + loc]                (n-major GEMM, then the packed decode without gates)

Under torch.autocast over fp32 master weights (examples/helloworld_amp.py) the same launches run on 16-bit compute copies that
the forward casts from the masters on EVERY call -- no cache: a captured graph re-casts on every replay, after the optimizer
has changed the masters -- and the weight / bias gradients leave their fp32 accumulators unrounded (out_dtype=torch.float32):
a loss-scaled fp16 sum past 65504 stays finite, and no 16-bit gradient is cast back up.

Gradient accumulation over micro-batches (layer.dropless_packed_main_grad, the Megatron-LM "gradient accumulation fusion"
convention): the weight / bias gradient kernels add their fp32 accumulators into p.main_grad of the expert parameter in their
epilogue (ops.expert_wgrad_packed(..., accumulate_into=p.main_grad)) instead of writing a gradient that AccumulateGrad reads back
and adds to p.grad.  The parameter's autograd gradient is then None (p.grad stays None) and p.grad_added_to_main_grad = True; the
optimizer reads main_grad.  For 16-bit parameters the sum over micro-batches stays in fp32 instead of being rounded per micro-batch.
The router weight and x keep their ordinary gradients.  MOELayer.forward raises instead of running the padded step when the switch
is on and the packed step is refused or a main_grad is missing (main_grad_problem): gradients never split between .grad and main_grad.
"""
import torch

from . import ep_native, losses
from .fast_dispatch import gates_from_scores
from .. import ops
from ..gates.top import LinearTopKGate


def _experts_kind(ex):
    from ..experts.ffn import FusedExpertsNetwork
    from ..experts.llama_ffn import LlamaFFNNetwork
    if isinstance(ex, LlamaFFNNetwork):
        return "swiglu"
    if isinstance(ex, FusedExpertsNetwork):
        return "ffn"
    return None


def autograd_live(layer, x):
    """grad enabled, and the input or an expert parameter requires grad"""
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in layer.experts.parameters()))


def unsupported(layer, gate, T, E, k, M, dtype, cf, alignment, reserve_dims=1, on_device=True):
    """why this layer's dropless training step cannot take the packed layout (None: it can): T tokens of M features in `dtype`
    (as MOELayer.forward hands them to the experts), E experts, top-k, capacity factor cf; host arithmetic only."""
    ex = layer.experts
    kind = _experts_kind(ex)
    if kind == "swiglu":
        return ep_native._swiglu_unsupported(ex, dtype) or "the packed training step covers ffn experts only (not SwiGLU)"
    if kind is None:
        return "the packed training step covers ffn experts (FusedExpertsNetwork) only"
    if cf > 0:
        return "the packed training step is dropless only (capacity_factor <= 0)"
    if layer.world_size != 1:
        return "the packed training step runs on a single rank only"
    if not layer.is_postscore:
        return "the packed training step needs is_postscore=True (gates applied in the decode)"
    if type(gate) is not LinearTopKGate or gate.gate_noise > 0:
        return "the packed training step needs a LinearTopKGate without gate noise"
    if layer.batch_prioritized_routing:
        return "the packed training step does not cover batch-prioritised routing"
    if not layer.is_gshard_loss:
        return "the packed training step needs the gshard loss"
    if ex.skip_expert or ex.sharded_count > 1 or layer.adaptive_degree != 1 or reserve_dims != 1:
        return "the packed training step needs unsharded local experts (sharded_count = 1, adaptive_r = 1, reserve_dims = 1)"
    w1 = ex.batched_fc1_w
    if torch.is_autocast_enabled() and w1.dtype == torch.float32:
        # fp32 master weights under (CUDA) autocast: 16-bit compute copies cast per call, fp32 gradients (_PackedFFNTrain)
        if any(p.dtype != torch.float32 for p in ex.parameters()):
            return "the packed training step under autocast needs every expert parameter in fp32 (master weights)"
        if dtype != torch.get_autocast_dtype("cuda") or dtype not in (torch.bfloat16, torch.float16):
            return "the packed training step under autocast needs tokens in the autocast dtype, bf16 / fp16"
    elif w1.dtype not in (torch.bfloat16, torch.float16) or dtype != w1.dtype:
        return "the packed training step needs bf16 / fp16 experts and tokens in their dtype"
    if ex.fused_activation() != "relu":
        return "the packed training step needs the ReLU activation"
    if not on_device or T == 0:
        return "the packed training step needs a non-empty batch on the HIP device"
    if ex.output_dim % 64 != 0:
        return "the packed training step needs M_out a multiple of 64 (the backward contracts over it)"
    limit = ep_native.dropless_row_limit(T, E, k, cf)
    return ep_native.packed_plan(T, E, k, M, w1.size(1), ex.output_dim, dtype, limit, alignment)[1]


def main_grad_problem(layer):
    """why this layer's expert gradients cannot be accumulated into main_grad (None: they can): every expert parameter that requires
    grad needs a contiguous fp32 main_grad of its shape on its device; host arithmetic only."""
    for name, p in layer.experts.named_parameters():
        if not p.requires_grad:
            continue
        mg = getattr(p, "main_grad", None)
        if not isinstance(mg, torch.Tensor):
            return f"expert parameter {name} has no main_grad (packed_train.attach_main_grads)"
        if mg.dtype != torch.float32:
            return f"main_grad of expert parameter {name} is {mg.dtype}, not torch.float32"
        if mg.shape != p.shape:
            return f"main_grad of expert parameter {name} has shape {tuple(mg.shape)}, the parameter {tuple(p.shape)}"
        if not mg.is_contiguous():
            return f"main_grad of expert parameter {name} is not contiguous"
        if mg.device != p.device:
            return f"main_grad of expert parameter {name} is on {mg.device}, the parameter on {p.device}"
    return None


def attach_main_grads(layer):
    """a zeroed fp32 main_grad of the parameter's shape, on its device, for every expert parameter that requires grad"""
    for p in layer.experts.parameters():
        if p.requires_grad:
            p.main_grad = torch.zeros(p.shape, dtype=torch.float32, device=p.device)
            p.grad_added_to_main_grad = False


def zero_main_grads(layer):
    """zero the expert parameters' main_grads in place (their addresses stay: a captured graph keeps accumulating into them)"""
    for p in layer.experts.parameters():
        if isinstance(getattr(p, "main_grad", None), torch.Tensor):
            p.main_grad.zero_()
            p.grad_added_to_main_grad = False


class _PackedFFNTrain(torch.autograd.Function):
    """y from (x, gates) over one packed layout; see the module docstring for the launches.  w1 / b1 / w2 / b2 are the parameters
    themselves: in x's dtype, or fp32 masters, cast to x's dtype here on every call (never cached: see the module docstring).
    main: None, or the parameters (w1, b1, w2, b2) whose gradients the backward adds into their main_grad instead of returning"""

    @staticmethod
    def forward(ctx, x, gates2d, w1, b1, w2, b2, lay, idx, loc, zero_row, main=None):
        ctx.master_dtype = w1.dtype
        ctx.main = main
        if w1.dtype != x.dtype:
            w1, w2 = w1.to(x.dtype), w2.to(x.dtype)
            b1 = b1.to(x.dtype) if b1 is not None else None
            b2 = b2.to(x.dtype) if b2 is not None else None
        hid = ops.expert_gemm_packed(x, w1, b1, True, lay, act="relu", gather=True, zero_row=zero_row)
        yp = ops.expert_gemm_packed(hid, w2, b2, False, lay)
        y = ops.fast_decode_packed(yp, idx, loc, gates2d, lay)
        ctx.save_for_backward(x, gates2d, w1, w2, hid, yp)
        ctx.lay, ctx.idx, ctx.loc, ctx.zero_row = lay, idx, loc, zero_row
        ctx.has_bias = (b1 is not None, b2 is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gates2d, w1, w2, hid, yp = ctx.saved_tensors   # w1, w2: the compute copies
        lay, idx, loc, gdt = ctx.lay, ctx.idx, ctx.loc, ctx.master_dtype
        gy = gy.contiguous()
        need_x, need_g, need_w1, need_b1, need_w2, need_b2 = ctx.needs_input_grad[:6]
        gx = gg = gw1 = gb1 = gw2 = gb2 = None

        def out(i):
            """where gradient i of (w1, b1, w2, b2) goes: a fresh tensor in the masters' dtype, or added into the parameter's main_grad"""
            if ctx.main is None:
                return {"out_dtype": gdt}
            ctx.main[i].grad_added_to_main_grad = True
            return {"accumulate_into": ctx.main[i].main_grad}

        def grad(g):
            return g if ctx.main is None else None   # accumulated in place: autograd gets no gradient for that parameter

        if need_g:
            gg = ops.gate_grad_packed(gy, yp, idx, loc, lay).to(gates2d.dtype)
        dyp = ops.fast_encode(gy, lay.slot_map, gates2d.detach(), lay.rows_bound)
        if need_w2:
            gw2 = grad(ops.expert_wgrad_packed(hid, dyp, lay, **out(2)))
        if need_b2 and ctx.has_bias[1]:
            gb2 = grad(ops.expert_bgrad_packed(dyp, lay, **out(3)))
        if need_x or need_w1 or (need_b1 and ctx.has_bias[0]):
            dhid = ops.expert_gemm_packed(dyp, w2, None, True, lay, mul=(hid > 0).to(hid.dtype))
            if need_w1:
                gw1 = grad(ops.expert_wgrad_packed(dhid, x, lay, gather="b", zero_row=ctx.zero_row, **out(0)))
            if need_b1 and ctx.has_bias[0]:
                gb1 = grad(ops.expert_bgrad_packed(dhid, lay, **out(1)))
            if need_x:
                gx = ops.fast_decode_packed(ops.expert_gemm_packed(dhid, w1, None, False, lay), idx, loc, None, lay)
        return gx, gg, gw1, gb1, gw2, gb2, None, None, None, None, None


def frozen_routing(logits, k, normalize_gate):
    """The routing prologue of a packed forward whose router takes no gradient: logits [T, E] -> (idx [k, T], gates [k, T],
    loc [k, T], dispatch_count [E], l_aux) -- the top-k launch and the location launch with the fused gshard loss, the kernel gates
    and loss as extract_critical takes them then.  Two launches, no host read.  Shared by the packed training step (a frozen
    router) and the packed FP8 forward (impls/packed_w8.py)."""
    E = logits.shape[1]
    work = logits if ops.routing_dtype(logits.dtype) else logits.float()
    l_dt = logits.dtype if ops.supported_dtype(logits.dtype) else torch.float32
    idx2d, gk, ws, _ = ops.gate_topk(work.detach(), k, apply_softmax=True, normalize_gate=normalize_gate)
    loc2d, cnt, _, lk, _ = ops.compute_location(idx2d, E, ws=ws, capacity=0, want_l_aux=True, l_aux_dtype=l_dt)
    gates2d = gk if gk.dtype == logits.dtype else gk.to(logits.dtype)
    l_aux = lk[0] if lk.dtype == logits.dtype else lk[0].to(logits.dtype)
    return idx2d, gates2d, loc2d, cnt, l_aux


def forward(layer, gate, x, logits, k, cf, alignment, main_grad=False):
    """One dropless training forward of `layer` on the packed layout: x [T, M], logits [T, E] (with autograd) -> (y [T, M_out], l_aux).
    main_grad: the backward accumulates the expert gradients into the parameters' main_grad (main_grad_problem(layer) is None).
    Sets dispatch_count, dropless_capacity (device int32 [1]), dropless_offsets and protected_shape as the packed forward does."""
    ex = layer.experts
    T, E = logits.shape
    M, H, Mo = x.shape[1], ex.batched_fc1_w.size(1), ex.output_dim
    limit = ep_native.dropless_row_limit(T, E, k, cf)
    plan, why = ep_native.packed_plan(T, E, k, M, H, Mo, x.dtype, limit, alignment)
    if plan is None:
        raise RuntimeError(why)
    # routing: the kernels extract_critical runs (same idx / loc / counts), on the detached logits
    work = logits if ops.routing_dtype(logits.dtype) else logits.float()
    l_dt = logits.dtype if ops.supported_dtype(logits.dtype) else torch.float32
    if torch.is_grad_enabled() and logits.requires_grad:
        idx2d, _, ws, _ = ops.gate_topk(work.detach(), k, apply_softmax=True, normalize_gate=layer.normalize_gate, want_scores=True)
        loc2d, cnt, _, _, _ = ops.compute_location(idx2d, E, ws=ws, capacity=0, want_l_aux=False, l_aux_dtype=l_dt)
        # the differentiable gates and the loss: extract_critical's training branch, op for op
        gates2d = torch.stack(gates_from_scores(torch.softmax(logits, dim=1), idx2d, layer.normalize_gate))
        l_aux = losses.gshard_loss(torch.softmax(logits, dim=1), idx2d.t().long())
    else:
        idx2d, gates2d, loc2d, cnt, l_aux = frozen_routing(logits, k, layer.normalize_gate)
    lay = ops.packed_layout(cnt, idx2d, loc2d, limit, alignment, plan["rows_bound"], plan["tiles_bound"], plan["row_limit"])
    # (its own tensor per call, not ops.zero_row: this step may run inside a captured graph, and the process-wide cache must not
    # hold memory that belongs to a graph's pool)
    zero_row = torch.zeros([max(M, 8)], dtype=x.dtype, device=x.device)
    xc = x if x.is_contiguous() else x.contiguous()
    params = (ex.batched_fc1_w, ex.batched_fc1_bias, ex.batched_fc2_w, ex.batched_fc2_bias)
    y = _PackedFFNTrain.apply(xc, gates2d, *params, lay, idx2d, loc2d, zero_row, params if main_grad else None)
    layer.dispatch_count = cnt
    layer.dropless_capacity = lay.capacity
    layer.dropless_offsets = lay.offsets
    layer.protected_shape = torch.Size([layer.num_local_experts, plan["rows_bound"], Mo])
    if getattr(layer, "_keep_routing", False):
        layer.last_routing = (idx2d.clone(), loc2d.clone())
    return y, l_aux
