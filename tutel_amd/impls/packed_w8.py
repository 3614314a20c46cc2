"""FP8 expert weights on the packed dropless forward: `ffn` and SwiGLU experts, inference, single rank, no host synchronisation.

The padded dropless forward of experts with `fp8_weights` reads the capacity back to the host to shape [E, C, *] buckets
(MOELayer's "routed" path), so it cannot be captured in a HIP graph; the one-call packed forwards (impls/ep_native.py) have no FP8
GEMM.  This forward composes the launches the library already has with the W8A16 grouped GEMMs over the packed tables
(csrc/expert_gemm_w8.hip, tutel_amd_expert_gemm_w8_packed / _glu_packed):

    routing : ops.gate_topk + ops.compute_location with the fused gshard loss      (packed_train.frozen_routing)
    layout  : ops.packed_layout -> offsets, tile table, packed slot map, device capacity
    fc1     : ffn     hid = act(x[slot] @ dq(W1)^T * s1 + b1)        ops.expert_gemm_w8_packed, rows gathered from the tokens
              SwiGLU  hid = act(x[slot] @ dq(Wg)^T * sg) * (x[slot] @ dq(Wu)^T * su)      ops.expert_gemm_w8_glu_packed
    fc2     : Y = hid @ dq(W2)^T * s2 + b2   (W_fc3 for SwiGLU, no bias)    ops.expert_gemm_w8_packed
    decode  : y[t] = sum_j g[j, t] * Y[off[e] + loc]                            ops.fast_decode_packed

Six launches, every extent per expert read from the device tables.  Each packed row is bit for bit the row the padded FP8 forward
computes (the W8 kernels' contract, include/tutel_amd.h), the routing and the decode are the padded path's own kernels, so the output,
the routing and l_aux equal the padded dropless FP8 forward's bits.  Opt-in: layer.dropless_packed_fp8 (TUTEL_AMD_DROPLESS_PACKED_FP8=1)
on top of layer.dropless_packed and experts.fp8_weights; MOELayer._packed_fp8_plan holds the admission.
"""
import torch

from . import ep_native, packed_train
from .. import _lib, ops
from ..experts import ffn as _ffn

ROUTING_REASON = ("the forward does not run through the one-call native path (autocast, training, batch-prioritised routing, "
                  "a non-gshard loss, gate noise, a router that takes a gradient, unequal token counts ...)")


def fp8_refusal(layer, x):
    """why this forward's experts cannot read FP8 weights on the packed layout (None: they can): the engine's own ladder.  The
    megablocks rung is walked with 0: on the packed layout megablocks_size only sets the alignment, as in the 16-bit packed forward"""
    ex = layer.experts
    if ep_native._swiglu(ex):
        return ex.w8_refusal(x, layer)   # (these experts' ladder has no megablocks rung)
    return ex.engine_refusal(_ffn.W8, x, layer, 0)


def forward(layer, x, logits, k, cf, alignment, plan):
    """x [T, M] contiguous, logits [T, E] -> (y [T, M_out], l_aux); plan: ep_native.packed_cover's for this call.  Sets dispatch_count,
    dropless_capacity (device int32 [1]), dropless_offsets, protected_shape and last_routing as ep_native.forward_packed does."""
    ex = layer.experts
    T, E = logits.shape
    M = x.shape[1]
    limit = ep_native.dropless_row_limit(T, E, k, cf)
    idx2d, gates2d, loc2d, cnt, l_aux = packed_train.frozen_routing(logits, k, layer.normalize_gate)
    lay = ops.packed_layout(cnt, idx2d, loc2d, limit, alignment, plan["rows_bound"], plan["tiles_bound"], plan["row_limit"])
    # (inside a capture its own tensor: the process-wide cache must not hold memory that belongs to a graph's pool)
    if torch.cuda.is_current_stream_capturing():
        zero_row = torch.zeros([max(M, 8)], dtype=x.dtype, device=x.device)
    else:
        zero_row = ops.zero_row(M, x.dtype, x.device)
    act = ex.fused_activation()
    if ep_native._swiglu(ex):
        (igu, sgu), (i3, s3) = ex.w8_params()
        H = ex.W_fc1_full_shape[2]
        hid = ops.expert_gemm_w8_glu_packed(x, igu, sgu, H, M, lay, act=act, gather=True, zero_row=zero_row)
        yp = ops.expert_gemm_w8_packed(hid, i3, s3, None, ex.output_dim, H, lay) if hid is not None else None
    else:
        (i1, s1), (i2, s2) = ex.w8_params()
        w1, b1, w2, b2 = _ffn._inference_params(ex)
        hid = ops.expert_gemm_w8_packed(x, i1, s1, b1, w1.size(1), M, lay, act=act, gather=True, zero_row=zero_row)
        yp = ops.expert_gemm_w8_packed(hid, i2, s2, b2, w2.size(2), w2.size(1), lay) if hid is not None else None
    if yp is None:   # the ladder asked the library's own coverage queries: a refusal here is a bug, never a quiet forward elsewhere
        raise _lib.TutelAmdError("the packed FP8 expert GEMMs refused a shape their own queries admit: " +
                                 _lib.lib().tutel_amd_last_error().decode("utf-8", "replace"))
    y = ops.fast_decode_packed(yp, idx2d, loc2d, gates2d, lay)
    layer.dispatch_count = cnt
    layer.dropless_capacity = lay.capacity
    layer.dropless_offsets = lay.offsets
    # (the middle entry is the host bound of the packed rows of ALL experts, as in ep_native.forward_packed)
    layer.protected_shape = torch.Size([layer.num_local_experts, plan["rows_bound"], ex.output_dim])
    if getattr(layer, "_keep_routing", False):
        layer.last_routing = (idx2d.clone(), loc2d.clone())
    return y, l_aux
