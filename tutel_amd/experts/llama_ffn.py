"""SwiGLU ("llama") per-expert FFN, `experts={'type': 'llama_ffn', 'hidden_size_per_expert': H, ..}`
(reference: tutel/experts/llama_ffn.py:7-44).

    y = (act(x @ W_fc1) * (x @ W_fc2)) @ W_fc3        per local expert, x [E_loc, R, M], no biases

Parameters keep the reference's names and its flat ZeRO-sharded storage (checkpoint compatible):
W_fc1 / W_fc2 hold ceil(E_loc*M*H / sharded_count) elements of the [E_loc, M, H] tensor, W_fc3 of
[E_loc, H, M]; all three are stored [K, N] row-major, i.e. the layout the grouped GEMM calls n-major.

Forward:
  * bf16 / fp16, no autograd, unsharded, recognised activation -> three launches of the MFMA
    grouped GEMM (tutel_amd_expert_gemm): the activation is fused into the W_fc1 launch and the
    gating product into the W_fc2 launch (its epilogue multiplies by the stored act(x @ W_fc1));
  * FP8 weights, opt-in (module.fp8_weights, default from TUTEL_AMD_FP8_WEIGHTS=1): the same experts in inference read e4m3 codes with
    one fp32 scale per (expert, output channel) -- TWO launches: the gate and up products in one (tutel_amd_expert_gemm_w8_glu, both
    weight matrices in one interleaved image, the gate never written to memory), then tutel_amd_expert_gemm_w8 on W_fc3; the images
    are derived copies in the KMajorCache (experts/w8.py).  w8_refusal names why a forward keeps its 16-bit weights.  module.fp8_freeze()
    makes the images the module's own buffers and frees the 16-bit weights (experts/fp8_resident.py): a forward that w8_refusal
    refuses then raises;
  * MXFP4 weights, opt-in (module.fp4_weights, default from TUTEL_AMD_FP4_WEIGHTS=1): the same two launches over e2m1 codes with one
    power-of-two scale byte per 32 values along K (tutel_amd_expert_gemm_w4_glu, then tutel_amd_expert_gemm_w4 on W_fc3; experts/w4.py).
    w4_refusal names why a forward does not take it; the packed dropless forward keeps its 16-bit path;
  * anything else -> ATen matmuls, op for op as the reference.
A dropless layer with `dropless_packed` runs these experts inside tutel_amd_moe_forward_packed_glu instead (impls/ep_native.py):
the gate and up products in ONE launch (tutel_amd_expert_gemm_gate_up's kernel), same bits as the two launches above.  With
`layer.dropless_packed_fp8` as well, FP8 weights run on that layout too (impls/packed_w8.py: tutel_amd_expert_gemm_w8_glu_packed, then
tutel_amd_expert_gemm_w8_packed on W_fc3), the bits of the padded FP8 forward.
"""
import types

import torch

from .. import net, ops
from . import ffn as _ffn
from . import fp8_resident, w4, w8
from .ffn import KMajorCache, classify_activation, _PREPACK


def _w8_params(net):
    return net.W_fc1, net.W_fc2, net.W_fc3


_W8_DTYPES = _ffn._dtypes(_ffn.W8_DTYPE_REASON, (torch.bfloat16, torch.float16), _w8_params)
_W8_GATHERED = _ffn._rung(_ffn.GATHERED_REASON,   # (these experts keep their own shard count: their parameters are stored flat and gathered)
                          lambda net, x, ctx, mb: net.sharded_count > 1 or _ffn._GATHERED(net, x, ctx, mb) is not None)
# fc3's K is H: stricter than the gate / up kernel's H % 16 == 0
_W8_SHAPE = _ffn._rung("the shape is not covered (M a multiple of 64, H a multiple of 64)",
                       lambda net, x, ctx, mb: not (ops.gemm_w8_glu_supported(x.dtype, net.W_fc1_full_shape[2], net.W_fc1_full_shape[1])
                                                    and ops.gemm_w8_supported(x.dtype, net.W_fc3_full_shape[2], net.W_fc3_full_shape[1])))
# why a forward of SwiGLU experts keeps its 16-bit weights: the shared rungs of experts/ffn.py, the switch first; the ORDER is behaviour
W8_LADDER = (
    _ffn._SWITCH_W8, _ffn._DEVICE, _ffn._AUTOGRAD_W8, _ffn._TRAINING_W8, _ffn._AUTOCAST, _W8_DTYPES, _W8_GATHERED, _ffn._ACTIVATION, _W8_SHAPE,
    _ffn._rung(_ffn.W8_CAPTURE_REASON, lambda net, x, ctx, mb: torch.cuda.is_current_stream_capturing() and not net.w8_cached()),
)
# the same for MXFP4 weights (W4A16): the FP4 switch's rungs, the W8 ladder's from the device rung on, its own shape and capture rungs
_W4_SHAPE = _ffn._rung("the shape is not covered (M a multiple of 64, H a multiple of 64)",
                       lambda net, x, ctx, mb: not (ops.gemm_w4_glu_supported(x.dtype, net.W_fc1_full_shape[2], net.W_fc1_full_shape[1])
                                                    and ops.gemm_w4_supported(x.dtype, net.W_fc3_full_shape[2], net.W_fc3_full_shape[1])))
W4_LADDER = (
    _ffn._SWITCH_W4, _ffn._W4_NOT_W8, _ffn._W4_NOT_FROZEN,
    _ffn._DEVICE, _ffn._AUTOGRAD_W8, _ffn._TRAINING_W8, _ffn._AUTOCAST, _W8_DTYPES, _W8_GATHERED, _ffn._ACTIVATION, _W4_SHAPE,
    _ffn._rung(_ffn.W8_CAPTURE_REASON, lambda net, x, ctx, mb: torch.cuda.is_current_stream_capturing() and not net.w4_cached()),
)
# the rungs a module answers without a forward, in the ladder's order: what fp8_freeze() requires
W8_STATIC = (_ffn._DEVICE, _ffn._TRAINING_W8, _W8_DTYPES, _W8_GATHERED, _ffn._ACTIVATION, _W8_SHAPE)


class LlamaFFNNetwork(torch.nn.Module):
    fp8_frozen = False   # True after fp8_freeze(): the FP8 images are the module's own buffers, the 16-bit weights are gone

    def _create_sharded_param(self, *full_shape, **kwargs):
        full_shape = torch.Size(full_shape)
        sharded = (full_shape.numel() + self.sharded_count - 1) // self.sharded_count
        return torch.nn.Parameter(torch.empty(sharded, **kwargs)), full_shape

    def _get_gathered_param(self, param, full_shape, parent_group):
        if self.sharded_count == 1:
            return param.view(full_shape)
        group = net.create_groups_from_world(group_count=-self.sharded_count, parent_group=parent_group).model_group
        return net.zero_gather(param, group=group).view(-1).narrow(0, 0, full_shape.numel()).view(full_shape)

    def __init__(self, model_dim, hidden_size_per_expert, num_experts_per_device, sharded_count,
                 activation_fn=torch.nn.functional.silu):
        super().__init__()
        self.sharded_count = sharded_count
        self.model_dim, self.output_dim = model_dim, model_dim
        self.W_fc1, self.W_fc1_full_shape = self._create_sharded_param(num_experts_per_device, model_dim, hidden_size_per_expert)
        self.W_fc2, self.W_fc2_full_shape = self._create_sharded_param(num_experts_per_device, model_dim, hidden_size_per_expert)
        self.W_fc3, self.W_fc3_full_shape = self._create_sharded_param(num_experts_per_device, hidden_size_per_expert, model_dim)
        self.activation_fn = activation_fn
        self._act_cache = {}
        self._kmajor = KMajorCache()
        # FP8 (e4m3) weights in inference, W8A16; the 16-bit parameters stay as they are
        self.fp8_weights = _ffn._FP8_WEIGHTS
        # MXFP4 weights in inference, W4A16; the 16-bit parameters stay as they are
        self.fp4_weights = _ffn._FP4_WEIGHTS
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            self.W_fc1.normal_(0, 0.01)
            self.W_fc2.normal_(0, 0.01)
            self.W_fc3.normal_(0, 0.01)

    def extra_repr(self):
        return "model_dim=%d, hidden_size=%d, num_experts_per_device=%d, sharded_count=%d." % (
            self.W_fc1_full_shape[1], self.W_fc1_full_shape[2], self.W_fc1_full_shape[0], self.sharded_count)

    # -- fused path -------------------------------------------------------------------------
    def fused_activation(self):
        key = self.training
        if key not in self._act_cache:
            self._act_cache[key] = classify_activation(self.activation_fn)
        return self._act_cache[key]

    def can_fuse(self, x, ctx):
        if self.fp8_frozen or not x.is_cuda or self.sharded_count > 1 or torch.is_autocast_enabled():
            return False
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        _, M, H = self.W_fc1_full_shape
        return (x.dim() == 3 and x.dtype == self.W_fc1.dtype and ops.gemm_supported(x.dtype, H, M)
                and ops.gemm_supported(x.dtype, M, H) and self.fused_activation() is not None)

    def kmajor_weights(self):
        """the eval-mode k-major copies (W_fc1 and W_fc2 [E, H, M], W_fc3 [E, M, H]) that forward_fused runs on: the operands of the
        packed dropless forward (impls/ep_native.py, tutel_amd_moe_forward_packed_glu)"""
        if self.fp8_frozen:
            raise RuntimeError(fp8_resident.REFUSED + "the 16-bit grouped GEMM was asked for")
        w1, w2, w3 = (self.W_fc1.view(self.W_fc1_full_shape), self.W_fc2.view(self.W_fc2_full_shape),
                      self.W_fc3.view(self.W_fc3_full_shape))
        return self._kmajor.get("fc1", w1), self._kmajor.get("fc2", w2), self._kmajor.get("fc3", w3)

    def forward_fused(self, x):
        w1, w2, w3 = (self.W_fc1.view(self.W_fc1_full_shape), self.W_fc2.view(self.W_fc2_full_shape),
                      self.W_fc3.view(self.W_fc3_full_shape))
        km = _PREPACK and not self.training  # eval: weights laid out k-major once (see KMajorCache)
        if km:
            w1, w2, w3 = self.kmajor_weights()
        g = ops.expert_gemm(x, w1, None, km, act=self.fused_activation())
        h = ops.expert_gemm(x, w2, None, km, mul=g)
        return ops.expert_gemm(h, w3, None, km)

    # -- FP8 weights (W8A16) --------------------------------------------------------------------
    def _no_autograd(self, x):
        return not (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())))

    def w8_refusal(self, x, ctx):
        """why this forward keeps its 16-bit weights (a string: the first failing check of W8_LADDER), or None when it reads FP8"""
        reasons = (check(self, x, ctx, None) for check in W8_LADDER)
        return next((why for why in reasons if why is not None), None)

    def _w8_views(self):
        return (self.W_fc1.view(self.W_fc1_full_shape), self.W_fc2.view(self.W_fc2_full_shape), self.W_fc3.view(self.W_fc3_full_shape))

    def _w8_gate_up_key(self, w2):
        """the gate / up entry is derived from BOTH parameters: W_fc2's key rides in the entry's `what`, W_fc1's is the entry's own"""
        return ("w8.glu", KMajorCache._key(w2))

    def w8_cached(self):
        if self.fp8_frozen:
            return True
        w1, w2, w3 = self._w8_views()
        return self._kmajor.holds("fc12.w8", w1, self._w8_gate_up_key(w2)) and self._kmajor.holds("fc3.w8", w3, "w8")

    def w8_params(self):
        """((image_gu, scale_gu), (image3, scale3)): the interleaved gate / up image of (W_fc1, W_fc2) and the image of W_fc3, all
        read from their [K, N] storage; derived copies re-quantised whenever a parameter they depend on changes (KMajorCache's rule);
        after fp8_freeze() the module's own buffers"""
        if self.fp8_frozen:
            return (self.fc12_w8, self.fc12_w8_scale), (self.fc3_w8, self.fc3_w8_scale)
        w1, w2, w3 = self._w8_views()
        gu = self._kmajor.derived("fc12.w8", w1, self._w8_gate_up_key(w2), lambda w: w8.prepare_gate_up(w, w2.detach(), False))
        p3 = self._kmajor.derived("fc3.w8", w3, "w8", lambda w: w8.prepare(w, False))
        return gu, p3

    def forward_fused_w8(self, x):
        """x [E_loc, R, M] contiguous -> [E_loc, R, M] in two launches: gate and up over one FP8 image, then W_fc3"""
        (igu, sgu), (i3, s3) = self.w8_params()
        _, M, H = self.W_fc1_full_shape
        h = ops.expert_gemm_w8_glu(x, igu, sgu, H, M, act=self.fused_activation())
        y = ops.expert_gemm_w8(h, i3, s3, None, M, H) if h is not None else None
        if y is None:   # the ladder asked the library's own coverage queries: a refusal here is a bug, never a quiet forward elsewhere
            from .. import _lib
            raise _lib.TutelAmdError("the FP8 expert GEMMs refused a shape their own queries admit: " +
                                     _lib.lib().tutel_amd_last_error().decode("utf-8", "replace"))
        return y

    def _forward_if_w8(self, x, ctx):
        """forward()'s FP8 step: the output, or None where the switch is off or a check refuses -- the reason is kept for the caller"""
        if not self.fp8_weights:
            return None
        why = self.w8_refusal(x, ctx)
        if why is None and not (x.dim() == 3 and x.size(0) == self.W_fc1_full_shape[0] and x.size(2) == self.W_fc1_full_shape[1]):
            why = "the input is not [E_loc, R, M]"
        try:
            setattr(ctx, "_fp8_weights_ran", True if why is None else why)
        except AttributeError:
            pass
        return self.forward_fused_w8(x.contiguous()) if why is None else None

    # -- MXFP4 weights (W4A16) ------------------------------------------------------------------
    def w4_refusal(self, x, ctx):
        """why this forward keeps its 16-bit weights (a string: the first failing check of W4_LADDER), or None when it reads MXFP4"""
        reasons = (check(self, x, ctx, None) for check in W4_LADDER)
        return next((why for why in reasons if why is not None), None)

    def _w4_gate_up_key(self, w2):
        return ("w4.glu", KMajorCache._key(w2))

    def w4_cached(self):
        w1, w2, w3 = self._w8_views()
        return self._kmajor.holds("fc12.w4", w1, self._w4_gate_up_key(w2)) and self._kmajor.holds("fc3.w4", w3, "w4")

    def w4_params(self):
        """((codes_gu, scales_gu), (codes3, scales3)): the interleaved gate / up MXFP4 image of (W_fc1, W_fc2) and the image of W_fc3,
        all read from their [K, N] storage; derived copies re-quantised whenever a parameter they depend on changes"""
        w1, w2, w3 = self._w8_views()
        gu = self._kmajor.derived("fc12.w4", w1, self._w4_gate_up_key(w2), lambda w: w4.prepare_gate_up(w, w2.detach(), False))
        p3 = self._kmajor.derived("fc3.w4", w3, "w4", lambda w: w4.prepare(w, False))
        return gu, p3

    def forward_fused_w4(self, x):
        """x [E_loc, R, M] contiguous -> [E_loc, R, M] in two launches: gate and up over one MXFP4 image, then W_fc3"""
        (cgu, sgu), (c3, s3) = self.w4_params()
        _, M, H = self.W_fc1_full_shape
        h = ops.expert_gemm_w4_glu(x, cgu, sgu, H, M, act=self.fused_activation())
        y = ops.expert_gemm_w4(h, c3, s3, None, M, H) if h is not None else None
        if y is None:   # the ladder asked the library's own coverage queries: a refusal here is a bug, never a quiet forward elsewhere
            from .. import _lib
            raise _lib.TutelAmdError("the FP4 expert GEMMs refused a shape their own queries admit: " +
                                     _lib.lib().tutel_amd_last_error().decode("utf-8", "replace"))
        return y

    def _forward_if_w4(self, x, ctx):
        """forward()'s FP4 step: the output, or None where the switch is off or a check refuses -- the reason is kept for the caller"""
        if not self.fp4_weights:
            return None
        why = self.w4_refusal(x, ctx)
        if why is None and not (x.dim() == 3 and x.size(0) == self.W_fc1_full_shape[0] and x.size(2) == self.W_fc1_full_shape[1]):
            why = "the input is not [E_loc, R, M]"
        try:
            setattr(ctx, "_fp4_weights_ran", True if why is None else why)
        except AttributeError:
            pass
        return self.forward_fused_w4(x.contiguous()) if why is None else None

    def invalidate_prepacked(self):
        self._kmajor.invalidate()

    def train(self, mode=True):
        if mode and self.fp8_frozen:
            raise RuntimeError(fp8_resident.REFUSED + _ffn._TRAINING_W8(types.SimpleNamespace(training=True), None, None, None))
        self._kmajor.invalidate()
        return super().train(mode)

    def _apply(self, fn, *args, **kwargs):
        fp8_resident.check_apply(self, fn)
        self._kmajor.invalidate()
        return super()._apply(fn, *args, **kwargs)

    def _load_from_state_dict(self, *args, **kwargs):
        return fp8_resident.load_from_state_dict(self, super()._load_from_state_dict, *args, **kwargs)

    # -- FP8-resident form (experts/fp8_resident.py) ----------------------------------------------------------------------
    def _fp8_steps(self):
        _, M, H = self.W_fc1_full_shape
        S = fp8_resident.Source
        return (fp8_resident.Step("fc12_w8", (S("W_fc1", tuple(self.W_fc1_full_shape), False, w8.glu_channel_map(H, False)),
                                              S("W_fc2", tuple(self.W_fc2_full_shape), False, w8.glu_channel_map(H, True))), 2 * H, M),
                fp8_resident.Step("fc3_w8", (S("W_fc3", tuple(self.W_fc3_full_shape), False, None),), M, H))

    def _fp8_dtype(self):
        return self.W_fc1.dtype

    def _fp8_static_refusal(self):
        """the first static rung of the W8 ladder this module fails (None: fp8_freeze() may run)"""
        x, ctx = fp8_resident.static_stand_ins(self.W_fc1)
        return fp8_resident.first_reason(self, W8_STATIC, x, ctx)

    def fp8_freeze(self):
        """Quantise gate and up into one image, then W_fc3, with the HIP quantiser; keep images and scales as buffers (fc12_w8,
        fc12_w8_scale, fc3_w8, fc3_w8_scale) and free the 16-bit weights, one parameter at a time.  Inference only from then on, and
        no way back (experts/fp8_resident.py).  ValueError, the module untouched, where a static rung of the FP8 ladder refuses"""
        return fp8_resident.freeze(self)

    # -- reference-equivalent ATen path -----------------------------------------------------
    def forward(self, x, ctx):
        y = self._forward_if_w8(x, ctx)
        if y is not None:
            return y
        if self.fp8_frozen:   # nothing below can run: every other forward reads the 16-bit weights
            raise RuntimeError(fp8_resident.REFUSED + (self.w8_refusal(x, ctx) or "the input is not [E_loc, R, M]"))
        y = self._forward_if_w4(x, ctx)
        if y is not None:
            return y
        if self.can_fuse(x, ctx):
            return self.forward_fused(x.contiguous())
        w1 = self._get_gathered_param(self.W_fc1, self.W_fc1_full_shape, ctx.group)
        w2 = self._get_gathered_param(self.W_fc2, self.W_fc2_full_shape, ctx.group)
        w3 = self._get_gathered_param(self.W_fc3, self.W_fc3_full_shape, ctx.group)
        y = self.activation_fn(torch.matmul(x, w1)) * torch.matmul(x, w2)
        return torch.matmul(y, w3)


ExpertModule = LlamaFFNNetwork
