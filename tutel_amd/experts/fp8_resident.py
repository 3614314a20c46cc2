"""FP8-resident experts: `module.fp8_freeze()` of FusedExpertsNetwork and LlamaFFNNetwork (experts/ffn.py, experts/llama_ffn.py).

With `fp8_weights` alone the FP8 images are DERIVED copies beside the 16-bit parameters: memory grows by half.  fp8_freeze() makes
the images and scales the module's own state and frees the 16-bit weights:

  * one parameter at a time -- quantise with the HIP quantiser (ops.quantize_w8: no fp32 copy, nothing but image and scales is
    allocated), register image and scale as buffers, release that parameter's storage, then the next: the peak over the freeze is
    the memory before it plus the images;
  * where a parameter stood, a META tensor of its shape and dtype stays: the ladders, the planner and the packed plans keep asking
    the experts for their sizes and dtype, and nothing can compute with it (an operation that mixes it with device data raises);
  * the module is inference only from then on: `.train()` raises, and every forward that would otherwise read the 16-bit weights
    raises RuntimeError with the FP8 ladder's reason (REFUSED below);
  * state_dict() holds the buffers (`fc1_w8`, `fc1_w8_scale`, ...) and no 16-bit weight; load_state_dict() takes that form (an
    unfrozen module on the device is frozen by it) or the 16-bit form, which a frozen module quantises on arrival, straight from the
    checkpoint's tensors, one at a time.

The two expert classes describe themselves by `_fp8_steps()` (below) and `_fp8_static_refusal()`; everything else is written once here.
"""
import types
from typing import NamedTuple

import torch

from .. import ops

REFUSED = "FP8-resident experts (fp8_freeze) hold no 16-bit weights to fall back to: "


class Source(NamedTuple):
    """one 16-bit parameter of a step"""
    name: str           # the parameter's attribute name (and its key in a 16-bit state dict)
    shape: tuple        # [E, N, K] (w_kmajor) or [E, K, N]: the parameter itself, or the view of a flat one
    w_kmajor: bool
    channel_map: object  # ops.quantize_w8's, None: the plain map


class Step(NamedTuple):
    """one image: the buffers `buffer` [E, channels / 32, K / 32, 64, 16] uint8 and `buffer`_scale [E, channels] fp32"""
    buffer: str
    sources: tuple
    channels: int
    K: int


def static_stand_ins(w, sharded_count=1):
    """(x, ctx) for walking the static rungs of a W8 ladder without a forward: what the rungs look at, taken from the module"""
    x = types.SimpleNamespace(is_cuda=w.is_cuda, dtype=w.dtype, requires_grad=False)
    ctx = types.SimpleNamespace(sharded_count=sharded_count, adaptive_degree=1, megablocks_size=0)
    return x, ctx


def first_reason(mod, rungs, x, ctx):
    return next((why for why in (check(mod, x, ctx, 0) for check in rungs) if why is not None), None)


def _release(mod, name):
    """the parameter's storage goes; a meta tensor keeps its shape and dtype answerable"""
    p = mod._parameters.pop(name)
    p.grad = None
    setattr(mod, name, torch.empty(p.shape, dtype=p.dtype, device="meta"))


def _register(mod, step, image, scale):
    mod.register_buffer(step.buffer, image)
    mod.register_buffer(step.buffer + "_scale", scale)


def _quantise(w, src, image=None, scale=None, check_only=False):
    if w.data_ptr() % 16 or not w.is_contiguous():
        w = w.clone(memory_format=torch.contiguous_format)
    res = ops.quantize_w8(w, src.w_kmajor, image=image, scale=scale, channel_map=src.channel_map, check_only=check_only)
    if res is None:   # the static rungs asked the GEMMs' coverage, which implies the quantiser's: a refusal here is a bug
        from .. import _lib
        raise _lib.TutelAmdError("tutel_amd_quantize_w8 refused a shape the FP8 GEMMs admit: " +
                                 _lib.lib().tutel_amd_last_error().decode("utf-8", "replace"))
    return res


def freeze(mod):
    """module.fp8_freeze(): see the module docstring.  Raises ValueError, the module untouched, where a static rung of the FP8
    ladder fails or a weight is not finite"""
    if mod.fp8_frozen:
        return mod
    why = mod._fp8_static_refusal()
    if why is not None:
        raise ValueError("fp8_freeze: " + why)
    steps = mod._fp8_steps()
    with torch.no_grad():
        # a non-finite weight raises BEFORE anything is released: the quantiser's first pass alone, which writes nothing
        for step in steps:
            for src in step.sources:
                _quantise(getattr(mod, src.name).detach().view(src.shape), src, check_only=True)
        mod.invalidate_prepacked()   # the derived copies of the 16-bit weights go first
        for step in steps:
            image = scale = None
            for src in step.sources:
                image, scale = _quantise(getattr(mod, src.name).detach().view(src.shape), src, image, scale)
                _release(mod, src.name)
            _register(mod, step, image, scale)
    for p in mod.parameters():   # the biases: inference only, nothing here takes a gradient any more
        p.requires_grad_(False)
    mod.fp8_frozen = mod.fp8_weights = True
    return mod


def _freeze_empty(mod):
    """the frozen form with unwritten buffers, for a state dict to fill"""
    for step in mod._fp8_steps():
        dev = getattr(mod, step.sources[0].name).device
        E = step.sources[0].shape[0]
        for src in step.sources:
            _release(mod, src.name)
        _register(mod, step, torch.empty([E, step.channels // 32, step.K // 32, 64, 16], dtype=torch.uint8, device=dev),
                  torch.empty([E, step.channels], dtype=torch.float32, device=dev))
    mod.invalidate_prepacked()
    for p in mod.parameters():   # the biases: inference only, nothing here takes a gradient any more
        p.requires_grad_(False)
    mod.fp8_frozen = mod.fp8_weights = True


def load_from_state_dict(mod, super_load, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
    """_load_from_state_dict of both expert classes.  FP8 keys into an unfrozen module: it is frozen first (its own static rungs
    decide, a refusal is a loading error), then the default copy fills the buffers.  16-bit keys into a frozen module: each tensor
    is quantised into the module's buffers by the HIP quantiser, straight from the checkpoint (a CPU tensor is moved to the device
    one parameter at a time); mismatches are reported as load_state_dict reports them"""
    mod.invalidate_prepacked()
    steps = mod._fp8_steps()
    has8 = any(prefix + step.buffer in state_dict for step in steps)
    has16 = any(prefix + src.name in state_dict for step in steps for src in step.sources)
    if not mod.fp8_frozen and has8 and not has16:
        why = mod._fp8_static_refusal()
        if why is not None:
            error_msgs.append(f"{prefix or 'experts'}: the state dict holds FP8-resident experts, which this module cannot become: {why}")
            return
        _freeze_empty(mod)
    if mod.fp8_frozen:
        state_dict = {k: v for k, v in state_dict.items() if k.startswith(prefix)}
        for step in steps:
            image, scale = getattr(mod, step.buffer), getattr(mod, step.buffer + "_scale")
            seen = [prefix + src.name in state_dict for src in step.sources]
            for src in step.sources:
                key = prefix + src.name
                if key not in state_dict:
                    if any(seen):   # one half of a gate / up pair without the other
                        missing_keys.append(key)
                    continue
                t, here = state_dict.pop(key), getattr(mod, src.name)
                if t.shape != here.shape:
                    error_msgs.append(f"size mismatch for {key}: copying a param with shape {t.shape} from checkpoint, "
                                      f"the shape in current model is {here.shape}.")
                elif t.dtype != here.dtype:
                    error_msgs.append(f"dtype mismatch for {key}: the checkpoint holds {t.dtype}, the FP8-resident module was frozen "
                                      f"from {here.dtype} (quantising another dtype gives other codes).")
                else:
                    try:
                        with torch.no_grad():
                            _quantise(t.detach().to(image.device).view(src.shape), src, image, scale)
                    except ValueError as e:
                        error_msgs.append(f"While copying the parameter named \"{key}\": {e}")
            if any(seen):   # the buffers ARE this checkpoint's weights now (or an error says why not): their keys are not missing
                state_dict.setdefault(prefix + step.buffer, image)
                state_dict.setdefault(prefix + step.buffer + "_scale", scale)
            for name, buf in ((step.buffer, image), (step.buffer + "_scale", scale)):
                t = state_dict.get(prefix + name)
                if t is not None and t.dtype != buf.dtype:   # (the default copy would cast in silence)
                    error_msgs.append(f"dtype mismatch for {prefix + name}: the checkpoint holds {t.dtype}, the module {buf.dtype}.")
                    del state_dict[prefix + name]
    return super_load(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)


def check_apply(mod, fn):
    """Module._apply of a frozen module (.to(), .cuda(), .half() ...): the images are tied to their device and the scales to fp32 --
    a cast or a move is refused before it touches a buffer"""
    if not mod.fp8_frozen:
        return
    image = getattr(mod, mod._fp8_steps()[0].buffer)
    probes = [torch.empty(0, dtype=dt, device=image.device) for dt in (torch.float32, mod._fp8_dtype())]
    if any(out.dtype != p.dtype or out.device != p.device for p, out in ((p, fn(p)) for p in probes)):
        raise RuntimeError("FP8-resident experts (fp8_freeze) cannot be cast or moved: the images belong to their device, the scales are fp32")
