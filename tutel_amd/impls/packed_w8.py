"""FP8 and MXFP4 expert weights on the packed dropless forward: `ffn` and SwiGLU experts, inference, single rank, no host synchronisation.

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
on top of layer.dropless_packed and experts.fp8_weights; MOELayer._packed_plan holds the admission.

MXFP4 weights are the same forward under another Format (below): the W4A16 GEMMs over the packed tables (csrc/expert_gemm_w4.hip,
tutel_amd_expert_gemm_w4_packed / _glu_packed), the W4 ladders, the W4 images, no scale multiply
in the formulas above; the bits of the padded dropless FP4 forward.  Opt-in: layer.dropless_packed_fp4 (TUTEL_AMD_DROPLESS_PACKED_FP4=1)
on top of layer.dropless_packed and experts.fp4_weights.  With both formats switched on FP8 runs (the W4 ladder's own rung).

W4A8 is a third Format over the same MXFP4 images: the rows are quantised per row to e4m3 (ops.quantize_rows_a8 -- the TOKENS whole,
once, since fc1 gathers them; the packed hidden rows up to offsets[E], the bound read on the device) and the GEMMs are the block-scaled
fp4 x fp8 ones over the packed tables (csrc/expert_gemm_w4a8.hip, tutel_amd_expert_gemm_w4a8_packed / _glu_packed): eight launches, the
bits of the padded dropless W4A8 forward.  Opt-in: layer.dropless_packed_w4a8 (TUTEL_AMD_DROPLESS_PACKED_W4A8=1) on top of the FP4
format's switches and experts.w4a8; asked in front of FP4, which runs where the W4A8 ladder refuses.

W8A8 is the fourth: the FP8 Format's images and channel scales under rows quantised the same way, on the unscaled fp8 x fp8 matrix
instruction over the packed tables (csrc/expert_gemm_w8a8.hip, tutel_amd_expert_gemm_w8a8_packed / _glu_packed): eight launches, the
bits of the padded dropless W8A8 forward.  Opt-in: layer.dropless_packed_w8a8 (TUTEL_AMD_DROPLESS_PACKED_W8A8=1) on top of the FP8
format's switches and experts.fp8_activations; asked in front of FP8, which runs where the W8A8 ladder refuses (the reason stays in
layer._fp8_activations_ran).
"""
from typing import NamedTuple

import torch

from . import ep_native, packed_train
from .. import _lib, ops
from ..experts import ffn as _ffn
from ..experts import fp8_resident

ROUTING_REASON = ("the forward does not run through the one-call native path (autocast, training, batch-prioritised routing, "
                  "a non-gshard loss, gate noise, a router that takes a gradient, unequal token counts ...)")


class Format(NamedTuple):
    """one weight format of this forward, by what differs between them"""
    name: str          # "FP8" / "FP4", as the messages spell it
    switch: str        # the layer's switch
    weights: str       # the experts' engine switch
    frozen: str        # the experts' attribute that is True once they are resident in this format ("": a refusal never raises)
    refused: str       # what a resident module's refusal raises, in front of the reason
    engine: object     # the `ffn` experts' engine (experts/ffn.py: its ladder, and `ran`, the layer's report)
    glu_refusal: str   # the SwiGLU experts' method that walks their ladder
    params: str        # the experts' method that returns the two pairs of images
    gemm: object       # (a, image, scale, bias, N, K, layout, act=, gather=, zero_row=) -> [rows_bound, N] or None
    gemm_glu: object   # (a, image, scale, H, K, layout, act=, gather=, zero_row=) -> [rows_bound, H] or None


FP8 = Format("FP8", "dropless_packed_fp8", "fp8_weights", "fp8_frozen", fp8_resident.REFUSED, _ffn.W8, "w8_refusal", "w8_params",
             ops.expert_gemm_w8_packed, ops.expert_gemm_w8_glu_packed)
FP4 = Format("FP4", "dropless_packed_fp4", "fp4_weights", "fp4_frozen", fp8_resident.REFUSED_FP4, _ffn.W4, "w4_refusal", "w4_params",
             ops.expert_gemm_w4_packed, ops.expert_gemm_w4_glu_packed)


def _quantised(packed_gemm):
    """a W4A8 / W8A8 packed GEMM in a Format's shape: quantise the rows of `a`, then the GEMM over the codes and scales"""
    def gemm(a, codes, scales, *args, gather=None, **kw):
        lay = args[-1]
        q = ops.quantize_rows_a8(a, rows_dev=None if gather else lay.offsets[lay.E:])
        return None if q is None else packed_gemm(q[0], q[1], codes, scales, *args[:-1], a.dtype, lay, gather=gather, **kw)
    return gemm


# (frozen "": FP4 is asked behind it and raises for an FP4-resident module that no packed forward can run)
W4A8 = Format("W4A8", "dropless_packed_w4a8", "w4a8", "", fp8_resident.REFUSED_FP4, _ffn.W4A8, "w4a8_refusal", "w4_params",
              _quantised(ops.expert_gemm_w4a8_packed), _quantised(ops.expert_gemm_w4a8_glu_packed))
# (frozen "": FP8 is asked behind it and raises for an FP8-resident module that no packed forward can run)
W8A8 = Format("W8A8", "dropless_packed_w8a8", "fp8_activations", "", fp8_resident.REFUSED, _ffn.W8A8, "w8a8_refusal", "w8_params",
              _quantised(ops.expert_gemm_w8a8_packed), _quantised(ops.expert_gemm_w8a8_glu_packed))
# the order the layer asks them in: with both weight formats switched on FP8 runs; W8A8 in front of FP8 and W4A8 in front of FP4
FORMATS = (W8A8, FP8, W4A8, FP4)


def refusal(fmt, layer, x):
    """why this forward's experts cannot read `fmt` weights on the packed layout (None: they can): the engine's own ladder.  The
    megablocks rung is walked with 0: on the packed layout megablocks_size only sets the alignment, as in the 16-bit packed forward"""
    ex = layer.experts
    if ep_native._swiglu(ex):
        return getattr(ex, fmt.glu_refusal)(x, layer)   # (these experts' ladder has no megablocks rung)
    return ex.engine_refusal(fmt.engine, x, layer, 0)


def forward(fmt, layer, x, logits, k, cf, alignment, plan):
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
        (igu, sgu), (i3, s3) = getattr(ex, fmt.params)()
        H = ex.W_fc1_full_shape[2]
        hid = fmt.gemm_glu(x, igu, sgu, H, M, lay, act=act, gather=True, zero_row=zero_row)
        yp = fmt.gemm(hid, i3, s3, None, ex.output_dim, H, lay) if hid is not None else None
    else:
        (i1, s1), (i2, s2) = getattr(ex, fmt.params)()
        w1, b1, w2, b2 = _ffn._inference_params(ex)
        hid = fmt.gemm(x, i1, s1, b1, w1.size(1), M, lay, act=act, gather=True, zero_row=zero_row)
        yp = fmt.gemm(hid, i2, s2, b2, w2.size(2), w2.size(1), lay) if hid is not None else None
    if yp is None:   # the ladder asked the library's own coverage queries: a refusal here is a bug, never a quiet forward elsewhere
        raise _lib.TutelAmdError(f"the packed {fmt.name} expert GEMMs refused a shape their own queries admit: " +
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
