"""Fused per-expert FFN (reference: tutel/experts/ffn.py, FusedExpertsNetwork).

Parameters keep the reference's names and shapes (checkpoint compatible):
    batched_fc1_w    [E_loc, H/s, M]        batched_fc1_bias [E_loc, H/s]
    batched_fc2_w    [E_loc, H/s, M_out]    batched_fc2_bias [E_loc, ceil(M_out/s)]

Forward, y = act(x @ W1^T + b1) @ W2 + b2 per local expert, x [E_loc, R, M]:
  * bf16 / fp16, no autograd, recognised activation -> the MFMA grouped GEMM kernels: two launches of
    tutel_amd_expert_gemm -- bias + activation fused into the first, bias into the second, dropless row counts honoured
    on device (or, opt-in with TUTEL_AMD_FFN_FUSED=1, ONE persistent launch for fc1 -> activation -> fc2,
    tutel_amd_expert_ffn: bit-identical, measured slower at the headline shape).  W2 is stored [H, M_out] (checkpoint format); the kernel takes that layout as is
    (training-mode modules) or, in eval mode, a k-major copy laid out once (KMajorCache below);
  * the gathered-weight modes -- adaptive_r = 0 (every rank's experts all-gathered, ffn.py:83-89) and sharded experts
    (num_local_experts < 0, ffn.py:91-109) -- run on the SAME MFMA grouped GEMM, fed the gathered [E, H', M] tensors
    (forward(), below the gathers);
  * fp32 experts, opt-in (TUTEL_AMD_NATIVE_FP32=1): two launches of tutel_amd_expert_gemm_f32 -- the exact-f32 MFMA, whose output is a
    k-ordered fmaf chain bit for bit (include/tutel_amd.h) -- with the same fusions: bias + activation in the epilogue, fc1's rows
    gathered from the tokens, fc2 read in its checkpoint layout.  No autograd, no megablocks row counts, local experts only;
  * FP8 weights, opt-in (module.fp8_weights, default from TUTEL_AMD_FP8_WEIGHTS=1): bf16 / fp16 experts in inference read e4m3 codes
    with one fp32 scale per (expert, output channel) instead of the 16-bit weights (W8A16: activations are not quantised) -- two
    launches of tutel_amd_expert_gemm_w8; the quantised images are derived copies in the KMajorCache (experts/w8.py).  A dropless
    layer with `dropless_packed` and `dropless_packed_fp8` runs them over the packed layout instead (impls/packed_w8.py).
    module.fp8_freeze() makes images and scales the module's own buffers, written by the HIP quantiser (csrc/quantize_w8.hip), and
    frees the 16-bit weights: the same launches on the same bits, inference only, FP8 state dicts (experts/fp8_resident.py);
  * MXFP4 weights, opt-in (module.fp4_weights, default from TUTEL_AMD_FP4_WEIGHTS=1): the same experts read e2m1 codes with one
    power-of-two scale byte per 32 values along K (W4A16; the widened weights are exact, activations are not quantised) -- two launches
    of tutel_amd_expert_gemm_w4; the images are derived copies in the KMajorCache (experts/w4.py), the 16-bit parameters stay;
  * otherwise fp32 / fp64 experts, weight gradients, and arbitrary python activations stay on ATen batched matmul (rocBLAS /
    hipBLASLt), op for op as the reference.
"""
import os
import types
from typing import NamedTuple

import torch
import torch.nn.functional as F

from .. import net, ops
from . import fp8_resident, w4, w8

# eval-mode weight pre-layout: keep a [E, N, K] (k-major) copy of weights stored [E, K, N]; 0 disables
_PREPACK = int(os.environ.get("TUTEL_AMD_PREPACK", "1")) != 0
# training: forward + data gradients of the bf16 / fp16 ReLU FFN on the MFMA grouped GEMM (weight gradients stay on ATen); 0 disables
_TRAIN_FUSED = int(os.environ.get("TUTEL_AMD_TRAIN_FUSED", "1")) != 0
# opt-in: fp32 experts on the native fp32 grouped GEMM (csrc/expert_gemm_f32.hip) instead of ATen's batched matmul.  Off: an fp32
# layer runs exactly as before
_NATIVE_FP32 = int(os.environ.get("TUTEL_AMD_NATIVE_FP32", "0")) != 0
# opt-in: bf16 / fp16 experts in inference stream their weights as FP8 (e4m3) codes (csrc/expert_gemm_w8.hip); the default of every
# module's `fp8_weights` switch.  Off: nothing changes
_FP8_WEIGHTS = int(os.environ.get("TUTEL_AMD_FP8_WEIGHTS", "0")) != 0
# opt-in: the same experts stream their weights as OCP MXFP4 (csrc/expert_gemm_w4.hip); the default of every module's `fp4_weights`
# switch.  Off: nothing changes
_FP4_WEIGHTS = int(os.environ.get("TUTEL_AMD_FP4_WEIGHTS", "0")) != 0


def _FFN_FUSED_ON():
    from .. import _lib
    return ops.get_option(_lib.OPT_FFN_FUSED) > 0


class _FFNTrain(torch.autograd.Function):
    """y = relu(x @ W1^T + b1) @ W2 + b2 per expert WITH autograd, on the grouped GEMM kernels (round 3).

    forward : two launches (bias + ReLU fused into the first, bias into the second); the hidden activation is kept for backward.
    backward: d hid = (gy @ W2^T) * [hid > 0] -- one launch, the ReLU mask rides in the GEMM's gating epilogue (W2 [E, H, M_out] is
              the k-major operand of that product as stored); d x = d hid @ W1 -- one launch (W1 [E, H, M] is its [K, N] operand as
              stored, consumed through the transposing LDS read).  The weight gradients contract over the ROW dimension
              (hid^T @ gy, d hid^T @ x): library batched GEMMs, as in the reference (ffn.py:114-120 under autograd)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        hid = ops.expert_gemm(x, w1, b1, True, act="relu")
        y = ops.expert_gemm(hid, w2, b2, False)
        ctx.save_for_backward(x, w1, w2, hid)
        ctx.has_bias = (b1 is not None, b2 is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w1, w2, hid = ctx.saved_tensors
        gy = gy.contiguous()
        need_x, need_w1, need_b1, need_w2, need_b2 = ctx.needs_input_grad
        gx = gw1 = gb1 = gw2 = gb2 = None
        if need_w2:
            gw2 = torch.matmul(hid.transpose(1, 2), gy)
        if need_b2 and ctx.has_bias[1]:
            gb2 = gy.sum(dim=1)
        if need_x or need_w1 or (need_b1 and ctx.has_bias[0]):
            ghid = ops.expert_gemm(gy, w2, None, True, mul=(hid > 0).to(hid.dtype))
            if need_x:
                gx = ops.expert_gemm(ghid, w1, None, False)
            if need_w1:
                gw1 = torch.matmul(ghid.transpose(1, 2), x)
            if need_b1 and ctx.has_bias[0]:
                gb1 = ghid.sum(dim=1)
        return gx, gw1, gb1, gw2, gb2


class KMajorCache:
    """k-major ([E, N, K] contiguous) copies of weights the checkpoint format stores [E, K, N].

    The MFMA operand layout wants 8 consecutive k per lane: a k-major tile is read from LDS with one
    ds_read_b128 per fragment, an n-major tile needs two transposing ds_read_b64_tr_b16 -- measured
    +3 us of 118 at the headline shape and +20 % at >= 256 rows per expert.  Inference weights are
    static, so the fused (no-autograd, eval) path lays them out once.  A copy is rebuilt whenever the
    parameter's storage pointer, autograd version counter (bumped by every in-place op on the
    parameter: optimizer steps, copy_, load_state_dict), dtype, device or shape changes.  Writes
    made through `param.data` bypass the version counter: call `invalidate()` (or
    `module.train()`; or set TUTEL_AMD_PREPACK=0) after such a write."""

    def __init__(self):
        self._store = {}

    @staticmethod
    def _key(w, *what):
        try:
            version = w._version
        except RuntimeError:  # inference tensors (module built under torch.inference_mode()) carry no version counter
            version = -1
        return (w.data_ptr(), version, w.dtype, w.device, tuple(w.shape)) + what

    def derived(self, name, w, what, make):
        """cached `make(w.detach())` -- any derived copy of parameter `w` (the FP8 image and scales of experts/w8.py), rebuilt under
        the same rule as the k-major copies; `what` names the derivation in the key"""
        key = self._key(w, what)
        hit = self._store.get(name)
        if hit is None or hit[0] != key:
            hit = (key, make(w.detach()))
            self._store[name] = hit
        return hit[1]

    def holds(self, name, w, what):
        hit = self._store.get(name)
        return hit is not None and hit[0] == self._key(w, what)

    def get(self, name, w, transpose=True, dtype=None):
        """cached derived copy of parameter `w`: transposed to k-major ([E, K, N] -> [E, N, K]) and / or cast to `dtype`
        (autocast: fp32 master weights, low-precision compute copies)"""
        key = self._key(w, bool(transpose), dtype)
        hit = self._store.get(name)
        if hit is None or hit[0] != key:
            t = w.detach()
            if dtype is not None and t.dtype != dtype:
                t = t.to(dtype)
            t = t.transpose(1, 2).contiguous() if transpose else t.contiguous()
            hit = (key, t)
            self._store[name] = hit
        return hit[1]

    def invalidate(self):
        self._store.clear()


def _probe_points():
    """fp32 probe: dense around the origin, then every magnitude a bf16 / fp16 / fp32 hidden activation can take."""
    lin = torch.linspace(-16.0, 16.0, 2049)
    mag = torch.logspace(-30, 38, 545)
    big = torch.tensor([60000.0, 65504.0, 1e5, 3.3e38])
    return torch.cat([lin, mag, -mag, big, -big, torch.zeros(1)])


_PROBE = _probe_points()
_REFS = (("relu", F.relu), ("gelu", F.gelu), ("silu", F.silu), ("none", lambda t: t))
# callables that ARE the fused epilogues (identity match, no evaluation needed)
_KNOWN_FNS = {F.relu: "relu", torch.relu: "relu", F.gelu: "gelu", F.silu: "silu"}


def classify_activation(fn, dtype=None):
    """Name of the fused GEMM epilogue that computes `fn`, or None (-> ATen path, the function is called).

    Recognised by identity: a string name, an explicit `_tutel_amd_act` tag, F.relu / F.gelu / F.silu
    themselves and default-argument nn.ReLU / nn.GELU / nn.SiLU modules.  Any other callable (typically
    the `lambda x: F.relu(x)` of the reference's examples, helloworld.py:86) is evaluated on a wide probe
    -- 2049 points on [-16, 16] plus every decade from 1e-30 to 3.3e38 in both signs, in fp32 AND in
    the experts' working dtype, twice (stochastic functions are rejected) -- and fused only when it
    matches an epilogue on every point: clipped variants (relu6, hardtanh, clamp) differ there."""
    if isinstance(fn, str):
        return fn if fn in ops.ACT_CODES else None
    tag = getattr(fn, "_tutel_amd_act", None)
    if tag in ops.ACT_CODES:
        return tag
    try:
        if fn in _KNOWN_FNS:
            return _KNOWN_FNS[fn]
    except TypeError:
        pass
    if isinstance(fn, torch.nn.Module):
        if type(fn) is torch.nn.ReLU:
            return "relu"
        if type(fn) is torch.nn.SiLU:
            return "silu"
        if type(fn) is torch.nn.GELU and getattr(fn, "approximate", "none") == "none":
            return "gelu"
        if type(fn) is torch.nn.Identity:
            return "none"
    try:
        with torch.no_grad():
            found = None
            for dt in ([torch.float32] + ([dtype] if dtype not in (None, torch.float32) else [])):
                lim = torch.finfo(dt).max
                probe = _PROBE.clamp(-lim, lim).to(dt)
                a, b = fn(probe.clone()), fn(probe.clone())
                if not (torch.is_tensor(a) and a.shape == probe.shape and a.dtype == dt and torch.equal(a, b)):
                    return None
                name = None
                for cand, ref in _REFS:
                    r = ref(probe)
                    if torch.allclose(a.float(), r.float(), rtol=0, atol=1e-7 if dt == torch.float32 else 0.0, equal_nan=True):
                        name = cand
                        break
                if name is None or (found is not None and name != found):
                    return None
                found = name
            return found
    except Exception:
        pass
    return None


# ---- the opt-in engines: replacements of the experts' default grouped GEMM -------------------------------------------------------
class Engine(NamedTuple):
    """One opt-in engine, by what differs between them.  Everything else is written once: FusedExpertsNetwork.engine_refusal walks
    the ladder, admitted_engine picks the engine a forward takes, forward_engine runs it (MOELayer._plan routes by the same answer)."""
    ran: str        # the attribute of the layer it reports into: True, or why this forward's experts did not take it
    ladder: tuple   # checks (net, x, ctx, megablocks_size) -> reason or None, the switch first; the ORDER is behaviour (users read the first)
    entry: str      # the library entry point `run` calls twice
    run: object     # (net, x, R, slot_map) -> y [E_loc, R, M_out], or None where the library refused

    def on(self, net):
        return self.ladder[0](net, None, None, None) is None


def _rung(reason, failed):
    """one check of a ladder: `reason` where failed(net, x, ctx, megablocks_size) holds"""
    return lambda net, x, ctx, mb: reason if failed(net, x, ctx, mb) else None


def _params(net):
    return net.batched_fc1_w, net.batched_fc2_w, net.batched_fc1_bias, net.batched_fc2_bias


def _dtypes(reason, allowed, params=_params):
    """the input in one of the `allowed` dtypes and every parameter in the input's"""
    return _rung(reason, lambda net, x, ctx, mb: x.dtype not in allowed or any(p is not None and p.dtype != x.dtype for p in params(net)))


def _shape(reason, covers):
    """both products covered by the library's own query: covers(x, N, K) for fc1 (N = H, K = M) and fc2 (N = M_out, K = H)"""
    return _rung(reason, lambda net, x, ctx, mb: not (covers(x, net.batched_fc1_w.size(1), net.batched_fc1_w.size(2))
                                                      and covers(x, net.batched_fc2_w.size(2), net.batched_fc2_w.size(1))))


_SKIP = _rung("SKIP_EXPERT is set", lambda net, x, ctx, mb: net.skip_expert)
_DEVICE = _rung("the input is not on the HIP device", lambda net, x, ctx, mb: not x.is_cuda)
_AUTOCAST = _rung("autocast is on", lambda net, x, ctx, mb: torch.is_autocast_enabled())
GATHERED_REASON = "gathered-weight modes (sharded experts, adaptive_r = 0) are not covered"
_GATHERED = _rung(GATHERED_REASON,
                  lambda net, x, ctx, mb: getattr(ctx, "sharded_count", 1) != 1 or getattr(ctx, "adaptive_degree", 1) == 0)
_MEGABLOCKS = _rung("megablocks row counts are not covered",   # mb: the value this forward will run with, where ctx does not hold it yet
                    lambda net, x, ctx, mb: (getattr(ctx, "megablocks_size", 0) if mb is None else mb) != 0)
_AUTOGRAD_F32 = _rung("autograd is live (training stays on ATen)", lambda net, x, ctx, mb: not net._no_autograd(x))
_AUTOGRAD_W8 = _rung("autograd is live (FP8 weights are inference only)", lambda net, x, ctx, mb: not net._no_autograd(x))
_ACTIVATION = _rung("the activation is not one of the fused epilogues", lambda net, x, ctx, mb: net.fused_activation() is None)
# the FP8 switch's own rungs, shared with SwiGLU experts (experts/llama_ffn.py walks a ladder of these)
_SWITCH_W8 = _rung("fp8_weights is off (TUTEL_AMD_FP8_WEIGHTS)", lambda net, x, ctx, mb: not net.fp8_weights)
_TRAINING_W8 = _rung("the module is in training mode (FP8 weights are inference only)", lambda net, x, ctx, mb: net.training)
W8_DTYPE_REASON = "the input is not bf16 / fp16 in the experts' own dtype"
# (quantising inside a capture would allocate the images in the graph's pool and redo the work at every replay)
W8_CAPTURE_REASON = "the quantised weights are not cached yet: run one eager forward before capturing a graph"


def _inference_params(net):
    """(w1, b1, w2, b2) detached, b2 cut to the output's width"""
    w1, w2, b1, b2 = (p.detach() if p is not None else None for p in _params(net))
    return w1, b1, w2, (b2[:, :net.output_dim] if b2 is not None else None)


def _run_f32(net, x, R, slot_map):
    """fc1 k-major with bias + activation, fc2 in its [H, M_out] layout"""
    w1, b1, w2, b2 = _inference_params(net)
    h = ops.expert_gemm_f32(x, w1, b1, True, act=net.fused_activation(), slot_map=slot_map, R=R)
    return ops.expert_gemm_f32(h, w2, b2, False) if h is not None else None


def _run_w8(net, x, R, slot_map):
    (i1, s1), (i2, s2) = net.w8_params()
    w1, b1, w2, b2 = _inference_params(net)
    h = ops.expert_gemm_w8(x, i1, s1, b1, w1.size(1), w1.size(2), act=net.fused_activation(), slot_map=slot_map, R=R)
    return ops.expert_gemm_w8(h, i2, s2, b2, w2.size(2), w2.size(1)) if h is not None else None


def _run_w4(net, x, R, slot_map):
    (c1, s1), (c2, s2) = net.w4_params()
    w1, b1, w2, b2 = _inference_params(net)
    h = ops.expert_gemm_w4(x, c1, s1, b1, w1.size(1), w1.size(2), act=net.fused_activation(), slot_map=slot_map, R=R)
    return ops.expert_gemm_w4(h, c2, s2, b2, w2.size(2), w2.size(1)) if h is not None else None


_W8_DTYPES = _dtypes(W8_DTYPE_REASON, (torch.bfloat16, torch.float16))
_W8_SHAPE = _shape("the shape is not covered (M and H multiples of 64, H and M_out multiples of 32)",
                   lambda x, N, K: ops.gemm_w8_supported(x.dtype, N, K))
# the rungs of the W8 ladder that a module answers without a forward, in the ladder's order: what fp8_freeze() requires
W8_STATIC = (_SKIP, _DEVICE, _TRAINING_W8, _W8_DTYPES, _GATHERED, _ACTIVATION, _W8_SHAPE)

# fp32 experts on the native fp32 grouped GEMM (the switch is read from the module at call time)
F32 = Engine(
    ran="_native_fp32_ran", entry="tutel_amd_expert_gemm_f32", run=_run_f32,
    ladder=(_rung("TUTEL_AMD_NATIVE_FP32 is off", lambda net, x, ctx, mb: not _NATIVE_FP32),
            _SKIP, _DEVICE, _AUTOCAST,
            _dtypes("the input and the experts' parameters are not all fp32", (torch.float32,)),
            _AUTOGRAD_F32, _GATHERED, _MEGABLOCKS, _ACTIVATION,
            _shape("the shape is not covered (M and H multiples of 32, H and M_out multiples of 4)",
                   lambda x, N, K: ops.gemm_f32_supported(N, K))))
# bf16 / fp16 experts in inference reading FP8 weights
W8 = Engine(
    ran="_fp8_weights_ran", entry="tutel_amd_expert_gemm_w8", run=_run_w8,
    ladder=(_SWITCH_W8, _SKIP, _DEVICE, _AUTOGRAD_W8, _TRAINING_W8,
            _AUTOCAST, _W8_DTYPES, _GATHERED, _MEGABLOCKS, _ACTIVATION, _W8_SHAPE,
            _rung(W8_CAPTURE_REASON,   # (FP8-resident experts hold their images for good)
                  lambda net, x, ctx, mb: torch.cuda.is_current_stream_capturing() and not net.fp8_frozen and not (
                      net._kmajor.holds("fc1.w8", net.batched_fc1_w, "w8") and net._kmajor.holds("fc2.w8", net.batched_fc2_w, "w8")))))
# the FP4 switch's own rungs, shared with SwiGLU experts
_SWITCH_W4 = _rung("fp4_weights is off (TUTEL_AMD_FP4_WEIGHTS)", lambda net, x, ctx, mb: not net.fp4_weights)
_W4_NOT_W8 = _rung("fp8_weights is on as well (one weight format per module)", lambda net, x, ctx, mb: net.fp8_weights)
_W4_NOT_FROZEN = _rung("the module is FP8-resident", lambda net, x, ctx, mb: net.fp8_frozen)
# bf16 / fp16 experts in inference reading MXFP4 weights: the W8 ladder's rungs from _SKIP on, then its own shape and capture rungs
W4 = Engine(
    ran="_fp4_weights_ran", entry="tutel_amd_expert_gemm_w4", run=_run_w4,
    ladder=(_SWITCH_W4, _W4_NOT_W8, _W4_NOT_FROZEN, _SKIP, _DEVICE, _AUTOGRAD_W8, _TRAINING_W8,
            _AUTOCAST, _W8_DTYPES, _GATHERED, _MEGABLOCKS, _ACTIVATION,
            _shape("the shape is not covered (M and H multiples of 64, H and M_out multiples of 32)",
                   lambda x, N, K: ops.gemm_w4_supported(x.dtype, N, K)),
            _rung(W8_CAPTURE_REASON,
                  lambda net, x, ctx, mb: torch.cuda.is_current_stream_capturing() and not (
                      net._kmajor.holds("fc1.w4", net.batched_fc1_w, "w4") and net._kmajor.holds("fc2.w4", net.batched_fc2_w, "w4")))))
# the order FusedExpertsNetwork.forward tries them in.  W8 and W4 exclude each other by W4's second rung (with both switches on FP8
# runs as it does alone), and either excludes F32 by dtype; an engine that is switched off is asked its first rung and nothing else
ENGINES = (W8, W4, F32)


class FusedExpertsNetwork(torch.nn.Module):
    fp8_frozen = False   # True after fp8_freeze(): the FP8 images are the module's own buffers, the 16-bit weights are gone

    def __init__(self, model_dim, hidden_size_per_expert, num_experts_per_device, sharded_count,
                 activation_fn=None, activation_fn_with_self=None, output_dim=None,
                 has_fc1_bias=True, has_fc2_bias=True):
        super().__init__()
        self.skip_expert = int(os.environ.get("SKIP_EXPERT", "0")) != 0
        assert hidden_size_per_expert % sharded_count == 0, \
            f"Can't evenly divide hidden_size_per_expert ({hidden_size_per_expert}) to {sharded_count} slices."
        self.model_dim = model_dim
        self.hidden_size_per_expert = hidden_size_per_expert
        self.local_experts = num_experts_per_device
        self.sharded_count = sharded_count
        self.hidden_size = hidden_size_per_expert // sharded_count
        self.output_dim = output_dim or model_dim

        self._act_opaque = False
        if activation_fn_with_self is not None:
            assert activation_fn is None, "Option `activation_fn_with_self` has been specified, please keep exactly one of them."
            tag = getattr(activation_fn_with_self, "_tutel_amd_act", None)
            activation_fn = lambda x: activation_fn_with_self(x, self)  # noqa: E731
            if tag is not None:
                activation_fn._tutel_amd_act = tag
            else:
                # a function of (x, module) may read module state or have side effects (fairseq passes
                # dropout + layernorm here): never evaluated on a probe, never replaced by an epilogue
                self._act_opaque = True
        if activation_fn is None:
            activation_fn = F.relu
        self.activation_fn = activation_fn
        self._act_cache = {}
        self._kmajor = KMajorCache()
        # FP8 (e4m3) weights in inference, W8A16 (the W8 engine); the 16-bit parameters stay as they are
        self.fp8_weights = _FP8_WEIGHTS
        # MXFP4 weights in inference, W4A16 (the W4 engine); the 16-bit parameters stay as they are
        self.fp4_weights = _FP4_WEIGHTS

        E, H = num_experts_per_device, self.hidden_size
        self.batched_fc1_w = torch.nn.Parameter(torch.empty(E, H, model_dim))
        self.batched_fc2_w = torch.nn.Parameter(torch.empty(E, H, self.output_dim))
        if has_fc1_bias:
            self.batched_fc1_bias = torch.nn.Parameter(torch.empty(E, H))
        else:
            self.register_parameter("batched_fc1_bias", None)
        if has_fc2_bias:
            self.batched_fc2_bias = torch.nn.Parameter(torch.empty(E, (self.output_dim + sharded_count - 1) // sharded_count))
        else:
            self.register_parameter("batched_fc2_bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        # per-expert nn.Linear initialisation, in the same RNG order as the reference
        # (ffn.py:39-49) so that seeded runs produce the same weights.
        with torch.no_grad():
            for i in range(self.batched_fc1_w.size(0)):
                fc1 = torch.nn.Linear(self.model_dim, self.hidden_size, bias=self.batched_fc1_bias is not None)
                fc2 = torch.nn.Linear(self.hidden_size, self.output_dim, bias=self.batched_fc2_bias is not None)
                self.batched_fc1_w[i] = fc1.weight
                self.batched_fc2_w[i] = fc2.weight.t()
                if self.batched_fc1_bias is not None:
                    self.batched_fc1_bias[i] = fc1.bias
                if self.batched_fc2_bias is not None:
                    self.batched_fc2_bias[i] = fc2.bias[:self.batched_fc2_bias.size(-1)]

    def extra_repr(self):
        return "model_dim=%d, hidden_size=%d, output_dim=%d, num_experts_per_device=%d. has_fc1_bias=%s, has_fc2_bias=%s." % (
            self.batched_fc1_w.size(2), self.batched_fc1_w.size(1), self.batched_fc2_w.size(2), self.batched_fc1_w.size(0),
            self.batched_fc1_bias is not None, self.batched_fc2_bias is not None)

    # -- fused path -------------------------------------------------------------------------
    def fused_activation(self):
        if self._act_opaque:
            return None
        key = (self.training, self.batched_fc1_w.dtype)
        if key not in self._act_cache:
            self._act_cache[key] = classify_activation(self.activation_fn, key[1])
        return self._act_cache[key]

    def _no_autograd(self, x):
        return not (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())))

    def compute_dtype(self, x):
        """dtype the MFMA GEMMs would run in for input x, or None.  Same dtype as the weights; or, under autocast,
        low-precision x against fp32 master weights -- ATen's matmul autocasts those (the reference relies on it,
        moe_layer.py:26-39,265-266, examples/helloworld_amp.py:76-79), the grouped GEMM uses cached casts instead."""
        w = self.batched_fc1_w
        if x.dtype not in (torch.bfloat16, torch.float16):
            return None
        if w.dtype == x.dtype:
            return x.dtype
        if torch.is_autocast_enabled() and w.dtype == torch.float32 and x.dtype == torch.get_autocast_dtype(x.device.type):
            return x.dtype
        return None

    def can_fuse(self, x, ctx):
        """the plain fused route: this rank's own local experts (no weight gathering), no autograd, MFMA-able shapes.  (False does NOT
        mean ATen: adaptive_r = 0 / sharded experts gather their weights in forward() and run the same MFMA kernel on the result.)"""
        if self.skip_expert or self.fp8_frozen or not x.is_cuda or not self._no_autograd(x):
            return False
        if getattr(ctx, "adaptive_degree", 1) == 0 or getattr(ctx, "sharded_count", 1) > 1:
            return False
        w1, w2 = self.batched_fc1_w, self.batched_fc2_w
        dt = self.compute_dtype(x)
        return (dt is not None and ops.gemm_supported(dt, w1.size(1), w1.size(2)) and
                ops.gemm_supported(dt, w2.size(2), w2.size(1)) and self.fused_activation() is not None)

    def can_fuse_training(self, x, ctx):
        """the same local experts WITH autograd: bf16 / fp16 (or autocast over fp32 master weights), ReLU, all four GEMM
        products MFMA-able (forward K = M, H; backward K = M_out, H)"""
        if (not _TRAIN_FUSED or self.skip_expert or self.fp8_frozen or not x.is_cuda or x.dim() != 3 or self._no_autograd(x)
                or getattr(ctx, "adaptive_degree", 1) == 0 or getattr(ctx, "sharded_count", 1) > 1):
            return False
        w1, w2 = self.batched_fc1_w, self.batched_fc2_w
        dt = self.compute_dtype(x)
        b2 = self.batched_fc2_bias
        return (dt is not None and self.fused_activation() == "relu" and x.size(0) == w1.size(0) and (b2 is None or b2.size(-1) == self.output_dim)
                and ops.gemm_supported(dt, w1.size(1), w1.size(2)) and ops.gemm_supported(dt, w2.size(2), w2.size(1))
                and ops.gemm_supported(dt, w2.size(1), w2.size(2)) and ops.gemm_supported(dt, w1.size(2), w1.size(1)))

    # -- the opt-in engines (Engine, above) ---------------------------------------------------------
    def engine_refusal(self, engine, x, ctx, megablocks_size=None):
        """why this forward does not take `engine` (a string: its first failing check), or None when it does.  megablocks_size: the
        value this forward will run with, where ctx does not hold it yet"""
        reasons = (check(self, x, ctx, megablocks_size) for check in engine.ladder)
        return next((why for why in reasons if why is not None), None)

    def admitted_engine(self, x, ctx, megablocks_size=None):
        """the opt-in engine this forward's experts run on, or None: the default GEMMs.  An engine that is switched off costs its
        switch and nothing else"""
        engines = (W8,) if self.fp8_frozen else ENGINES
        return next((e for e in engines if self.engine_refusal(e, x, ctx, megablocks_size) is None), None)

    def forward_engine(self, engine, x, R=None, slot_map=None):
        """x [E_loc, R, M] contiguous -> [E_loc, R, M_out] in two launches of engine.entry; slot_map given: x is the TOKEN array [T, M]
        and fc1 gathers its rows (R = capacity)"""
        y = engine.run(self, x, R, slot_map)
        if y is None:   # the ladder asked the library's own coverage query: a refusal here is a bug, never a quiet forward elsewhere
            from .. import _lib
            raise _lib.TutelAmdError(engine.entry + " refused a shape its own query admits: " +
                                     _lib.lib().tutel_amd_last_error().decode("utf-8", "replace"))
        return y

    def _forward_if_admitted(self, engine, x, ctx):
        """forward()'s step for one engine: its output, or None where it is off or refuses -- the reason is kept for the caller"""
        if not engine.on(self):
            return None
        why = self.engine_refusal(engine, x, ctx)
        if why is None and not (x.dim() == 3 and x.size(0) == self.batched_fc1_w.size(0) and x.size(2) == self.batched_fc1_w.size(2)):
            why = "the input is not [E_loc, R, M]"
        try:
            setattr(ctx, engine.ran, True if why is None else why)
        except AttributeError:
            pass
        return self.forward_engine(engine, x.contiguous()) if why is None else None

    def f32_refusal(self, x, ctx, megablocks_size=None):
        return self.engine_refusal(F32, x, ctx, megablocks_size)

    def can_fuse_f32(self, x, ctx):
        return self.engine_refusal(F32, x, ctx) is None

    def forward_fused_f32(self, x, ctx, R=None, slot_map=None):
        return self.forward_engine(F32, x, R, slot_map)

    def w8_refusal(self, x, ctx, megablocks_size=None):
        return self.engine_refusal(W8, x, ctx, megablocks_size)

    def forward_fused_w8(self, x, ctx, R=None, slot_map=None):
        return self.forward_engine(W8, x, R, slot_map)

    def w4_refusal(self, x, ctx, megablocks_size=None):
        return self.engine_refusal(W4, x, ctx, megablocks_size)

    def forward_fused_w4(self, x, ctx, R=None, slot_map=None):
        return self.forward_engine(W4, x, R, slot_map)

    def w4_params(self):
        """((codes1, scales1), (codes2, scales2)): the MXFP4 images of fc1 (read as stored, k-major) and fc2 (from its [E, H, M_out]
        storage), derived copies re-quantised whenever the KMajorCache would rebuild a k-major copy"""
        p1 = self._kmajor.derived("fc1.w4", self.batched_fc1_w, "w4", lambda w: w4.prepare(w, True))
        p2 = self._kmajor.derived("fc2.w4", self.batched_fc2_w, "w4", lambda w: w4.prepare(w, False))
        return p1, p2

    def w8_params(self):
        """((image1, scale1), (image2, scale2)): the FP8 images and scales of fc1 (read as stored, k-major) and fc2 (from its
        [E, H, M_out] storage), derived copies re-quantised whenever the KMajorCache would rebuild a k-major copy; after fp8_freeze()
        the module's own buffers"""
        if self.fp8_frozen:
            return (self.fc1_w8, self.fc1_w8_scale), (self.fc2_w8, self.fc2_w8_scale)
        p1 = self._kmajor.derived("fc1.w8", self.batched_fc1_w, "w8", lambda w: w8.prepare(w, True))
        p2 = self._kmajor.derived("fc2.w8", self.batched_fc2_w, "w8", lambda w: w8.prepare(w, False))
        return p1, p2

    def fused_params(self, dtype):
        """(w1, b1, w2, b2, w2_kmajor) of this rank's experts in the GEMM's compute dtype: the parameters themselves, or
        cached casts under autocast; fc2 as a k-major copy in eval mode."""
        if self.fp8_frozen:
            raise RuntimeError(fp8_resident.REFUSED + "the 16-bit grouped GEMM was asked for")
        w1, b1, w2, b2 = self.batched_fc1_w, self.batched_fc1_bias, self.batched_fc2_w, self.batched_fc2_bias
        cast = None if w1.dtype == dtype else dtype
        kmajor = self.w2_kmajor_now()
        if cast is not None:
            w1 = self._kmajor.get("fc1.cast", w1, transpose=False, dtype=cast)
            b1 = self._kmajor.get("b1.cast", b1, transpose=False, dtype=cast) if b1 is not None else None
        if kmajor or cast is not None:
            w2 = self._kmajor.get("fc2", w2, transpose=kmajor, dtype=cast)
        if b2 is not None:
            if b2.size(-1) != self.output_dim or cast is not None:
                b2 = self._kmajor.get("b2.cast", b2[:, :self.output_dim], transpose=False, dtype=cast)
        return w1, b1, w2, b2, kmajor

    def forward_fused(self, x, ctx, a_layout=None, R=None, out=None, d_layout=None, slot_map=None, expert_range=None):
        """x [E_loc,R,M] (or the raw all-to-all buffer described by a_layout) -> [E_loc,R,M_out]
        (or written into `out` in d_layout).  Two MFMA grouped-GEMM launches.
        slot_map given: x is the TOKEN array [T,M] and fc1 gathers its rows through the slot map
        (fast_encode fused into the GEMM; R = capacity).
        expert_range = (lo, hi): only local experts lo..hi-1 (x / out then hold hi-lo experts)."""
        counts, align = None, 1
        if getattr(ctx, "megablocks_size", 0) > 0:
            counts, align = ctx.dispatch_count, int(ctx.megablocks_size)
        w1, b1, w2, b2, w2_kmajor = self.fused_params(self.compute_dtype(x))
        if expert_range is not None:
            lo, hi = expert_range
            w1, w2 = w1[lo:hi], w2[lo:hi]
            b1 = b1[lo:hi] if b1 is not None else None
            b2 = b2[lo:hi] if b2 is not None else None
            assert counts is None, "megablocks row counts are not sliced"
        # TUTEL_OPT_FFN_FUSED = 1 (opt-in; the two launches below measured faster): one persistent launch for fc1 -> activation -> fc2
        # where the library takes the shape (<= 128 rows per expert, k-major fc2, plain [E_loc, R, *] operands) -- same tiles, same bits
        if _FFN_FUSED_ON() and w2_kmajor and counts is None and out is None and a_layout is None and d_layout is None and (slot_map is not None or x.dim() == 3):
            y = ops.expert_ffn(x, w1, b1, w2, b2, self.fused_activation(), R=R, smap=slot_map)
            if y is not None:
                return y
        if slot_map is not None:
            h = ops.expert_gemm_gather(x, slot_map, w1, b1, True, self.fused_activation(), R,
                                       row_counts=counts, row_align=align)
        else:
            h = ops.expert_gemm(x, w1, b1, True, act=self.fused_activation(), E_loc=w1.size(0), R=R,
                                a_layout=a_layout, row_counts=counts, row_align=align)
        return ops.expert_gemm(h, w2, b2, w2_kmajor, out=out, d_layout=d_layout, row_counts=counts, row_align=align)

    def w2_kmajor_now(self):
        """eval-mode modules run fc2 on a k-major copy of its weights (KMajorCache)"""
        return _PREPACK and not self.training

    def invalidate_prepacked(self):
        """Drop the eval-mode k-major weight copies (needed only after writes through `param.data`)."""
        self._kmajor.invalidate()

    def train(self, mode=True):
        if mode and self.fp8_frozen:
            raise RuntimeError(fp8_resident.REFUSED + _TRAINING_W8(types.SimpleNamespace(training=True), None, None, None))
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
        E, H, M = self.batched_fc1_w.shape
        Mo = self.batched_fc2_w.size(2)
        S = fp8_resident.Source
        return (fp8_resident.Step("fc1_w8", (S("batched_fc1_w", (E, H, M), True, None),), H, M),
                fp8_resident.Step("fc2_w8", (S("batched_fc2_w", (E, H, Mo), False, None),), Mo, H))

    def _fp8_dtype(self):
        return self.batched_fc1_w.dtype

    def _fp8_static_refusal(self):
        """the first static rung of the W8 ladder this module fails (None: fp8_freeze() may run)"""
        x, ctx = fp8_resident.static_stand_ins(self.batched_fc1_w, self.sharded_count)
        return fp8_resident.first_reason(self, W8_STATIC, x, ctx)

    def fp8_freeze(self):
        """Quantise fc1 and fc2 with the HIP quantiser, keep images and scales as buffers (fc1_w8, fc1_w8_scale, fc2_w8,
        fc2_w8_scale) and free the 16-bit weights, one parameter at a time; the biases stay.  Inference only from then on, and no
        way back (experts/fp8_resident.py).  ValueError, the module untouched, where a static rung of the FP8 ladder refuses"""
        return fp8_resident.freeze(self)

    # -- gathered-weight modes + the reference-equivalent ATen path ------------------------------
    def forward(self, x, ctx):
        if self.skip_expert:
            return x
        # the opt-in engines (W8 and W4 in front of the default GEMMs, F32 behind them); the reason one did not run is kept for the caller
        y = self._forward_if_admitted(W8, x, ctx)
        if y is not None:
            return y
        if self.fp8_frozen:   # nothing below can run: every other forward reads the 16-bit weights
            raise RuntimeError(fp8_resident.REFUSED + (self.engine_refusal(W8, x, ctx) or "the input is not [E_loc, R, M]"))
        y = self._forward_if_admitted(W4, x, ctx)
        if y is not None:
            return y

        if self.can_fuse(x, ctx):
            return self.forward_fused(x.contiguous(), ctx)

        y = self._forward_if_admitted(F32, x, ctx)
        if y is not None:
            return y

        if self.can_fuse_training(x, ctx):
            dt = self.compute_dtype(x)
            b1, b2 = self.batched_fc1_bias, self.batched_fc2_bias
            return _FFNTrain.apply(x.contiguous(), self.batched_fc1_w.to(dt), b1.to(dt) if b1 is not None else None,
                                   self.batched_fc2_w.to(dt), b2.to(dt) if b2 is not None else None)

        w1, w2 = self.batched_fc1_w, self.batched_fc2_w
        b1 = self.batched_fc1_bias.unsqueeze(1) if self.batched_fc1_bias is not None else None
        b2 = self.batched_fc2_bias.unsqueeze(1) if self.batched_fc2_bias is not None else None

        if ctx.adaptive_degree == 0:  # data-parallel experts: gather every rank's weights (ffn.py:83-89)
            E = ctx.num_global_experts
            w1 = net.zero_gather(w1, group=ctx.group).view(E, -1, w1.size(2))
            w2 = net.zero_gather(w2, group=ctx.group).view(E, -1, w2.size(2))
            if b1 is not None:
                b1 = net.zero_gather(b1, group=ctx.group).view(E, 1, -1)
            if b2 is not None:
                b2 = net.zero_gather(b2, group=ctx.group).view(E, 1, -1)
        elif ctx.sharded_count > 1:  # one expert's hidden dim sliced over ranks (ffn.py:91-109)
            mesh = net.get_world_size(ctx.group)
            if 1 < mesh < net.get_world_size():
                ctx.adaptive_degree = ctx.sharded_count
            group_size = ctx.sharded_count // ctx.adaptive_degree
            if group_size > 1:
                zg = net.create_groups_from_world(group_count=-group_size, parent_group=ctx.group).model_group
                w1 = net.zero_gather(w1, group=zg).view(1, -1, ctx.model_dim)
                w2 = net.zero_gather(w2, group=zg).view(1, -1, self.output_dim)
                if b1 is not None:
                    b1 = net.zero_gather(b1, group=zg).view(1, 1, -1)
            if b2 is not None:
                bg = net.create_groups_from_world(group_count=ctx.num_global_experts, parent_group=ctx.group).model_group
                b2 = net.zero_gather(b2, group=bg).view(1, 1, -1)
                if ctx.adaptive_degree > 1:
                    b2 = b2 * (1.0 / ctx.adaptive_degree)
        if b2 is not None and b2.size(-1) != self.output_dim:
            b2 = b2[:, :, :self.output_dim]

        # the gathered / sliced weights on the MFMA grouped GEMM as well (adaptive_r = 0 and sharded experts used to leave
        # the hand-written path): weights as they come out of the gather -- fc2 in its [E, H', M_out] checkpoint layout
        dt = self.compute_dtype(x)
        if (dt is not None and x.is_cuda and self._no_autograd(x) and self.fused_activation() is not None and x.dim() == 3
                and x.size(0) == w1.size(0) and ops.gemm_supported(dt, w1.size(1), w1.size(2))
                and ops.gemm_supported(dt, w2.size(2), w2.size(1))):
            def prep(t):
                return None if t is None else t.detach().to(dt).contiguous()
            b1f = prep(b1.squeeze(1)) if b1 is not None else None
            b2f = prep(b2.squeeze(1)) if b2 is not None else None
            h = ops.expert_gemm(x.contiguous(), prep(w1), b1f, True, act=self.fused_activation())
            return ops.expert_gemm(h, prep(w2), b2f, False)

        y = torch.matmul(x, w1.permute(0, 2, 1))
        if b1 is not None:
            y = y + b1
        y = self.activation_fn(y)
        y = torch.matmul(y, w2)
        if b2 is not None:
            y = y + b2
        return y


ExpertModule = FusedExpertsNetwork
