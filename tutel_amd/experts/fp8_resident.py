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

MXFP4-resident experts (`module.fp4_freeze()`) are the same machinery under another Format (below): the buffers are the W4A16 code
image and scale image (`fc1_w4`, `fc1_w4_scale`, ...), written by ops.quantize_w4, and the ladder that decides is the W4 one.  A
module is resident in one format at most: fp8_freeze() and fp4_freeze() refuse each other.
"""
import types
from typing import NamedTuple

import torch

from .. import ops

REFUSED = "FP8-resident experts (fp8_freeze) hold no 16-bit weights to fall back to: "
REFUSED_FP4 = "FP4-resident experts (fp4_freeze) hold no 16-bit weights to fall back to: "


class Format(NamedTuple):
    """one resident form, by what differs between them"""
    name: str            # "FP8" / "FP4", as the messages spell it
    method: str          # the module's freezing method
    flag: str            # the module's attribute that is True once frozen
    switch: str          # the module's engine switch, on with the flag
    steps: str           # the module's method that lists its Steps
    static_refusal: str  # the module's method that walks the static rungs of the format's ladder
    buffers: object      # (step, E) -> ((shape, dtype) of `buffer`, (shape, dtype) of `buffer`_scale)
    quantize: object     # (w, src, image, scale, check_only) -> (image, scale), or None where the library refuses
    entry: str           # the library entry point `quantize` calls
    refused: str         # what a forward that would read the 16-bit weights raises, in front of the ladder's reason
    no_apply: str        # what a cast or a move raises


FP8 = Format(
    name="FP8", method="fp8_freeze", flag="fp8_frozen", switch="fp8_weights", steps="_fp8_steps", static_refusal="_fp8_static_refusal",
    buffers=lambda step, E: (([E, step.channels // 32, step.K // 32, 64, 16], torch.uint8), ([E, step.channels], torch.float32)),
    quantize=lambda w, src, image, scale, check_only: ops.quantize_w8(w, src.w_kmajor, image=image, scale=scale,
                                                                      channel_map=src.channel_map, check_only=check_only),
    entry="tutel_amd_quantize_w8", refused=REFUSED,
    no_apply="FP8-resident experts (fp8_freeze) cannot be cast or moved: the images belong to their device, the scales are fp32")
FP4 = Format(
    name="FP4", method="fp4_freeze", flag="fp4_frozen", switch="fp4_weights", steps="_fp4_steps", static_refusal="_fp4_static_refusal",
    buffers=lambda step, E: (([E, step.channels // 32, step.K // 64, 64, 16], torch.uint8),
                             ([E, step.channels // 32, (step.K + 127) // 128, 32, 4], torch.uint8)),
    quantize=lambda w, src, image, scale, check_only: ops.quantize_w4(w, src.w_kmajor, codes=image, scales=scale,
                                                                      channel_map=src.channel_map, check_only=check_only),
    entry="tutel_amd_quantize_w4", refused=REFUSED_FP4,
    no_apply="FP4-resident experts (fp4_freeze) cannot be cast or moved: the images belong to their device and to the dtype they were "
             "quantised for")
FORMATS = (FP8, FP4)


def resident(mod):
    """the Format a module is frozen in, or None"""
    return next((fmt for fmt in FORMATS if getattr(mod, fmt.flag, False)), None)


class Source(NamedTuple):
    """one 16-bit parameter of a step"""
    name: str           # the parameter's attribute name (and its key in a 16-bit state dict)
    shape: tuple        # [E, N, K] (w_kmajor) or [E, K, N]: the parameter itself, or the view of a flat one
    w_kmajor: bool
    channel_map: object  # ops.quantize_w8's / ops.quantize_w4's, None: the plain map


class Step(NamedTuple):
    """one image: the buffers `buffer` and `buffer`_scale, in the shapes of the Format (FP8: [E, channels / 32, K / 32, 64, 16] uint8
    and [E, channels] fp32)"""
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


def _quantise(fmt, w, src, image=None, scale=None, check_only=False):
    if w.data_ptr() % 16 or not w.is_contiguous():
        w = w.clone(memory_format=torch.contiguous_format)
    res = fmt.quantize(w, src, image, scale, check_only)
    if res is None:   # the static rungs asked the GEMMs' coverage, which implies the quantiser's: a refusal here is a bug
        from .. import _lib
        raise _lib.TutelAmdError(f"{fmt.entry} refused a shape the {fmt.name} GEMMs admit: " +
                                 _lib.lib().tutel_amd_last_error().decode("utf-8", "replace"))
    return res


def freeze(mod, fmt=FP8):
    """module.fp8_freeze() (fmt FP4: module.fp4_freeze()): see the module docstring.  Raises ValueError, the module untouched, where
    a static rung of the format's ladder fails, the module is resident in the other format or a weight is not finite"""
    now = resident(mod)
    if now is fmt:
        return mod
    if now is not None:
        raise ValueError(f"{fmt.method}: the module is {now.name}-resident")
    why = getattr(mod, fmt.static_refusal)()
    if why is not None:
        raise ValueError(f"{fmt.method}: " + why)
    steps = getattr(mod, fmt.steps)()
    with torch.no_grad():
        # a non-finite weight raises BEFORE anything is released: the quantiser's first pass alone, which writes nothing
        for step in steps:
            for src in step.sources:
                _quantise(fmt, getattr(mod, src.name).detach().view(src.shape), src, check_only=True)
        mod.invalidate_prepacked()   # the derived copies of the 16-bit weights go first
        for step in steps:
            image = scale = None
            for src in step.sources:
                image, scale = _quantise(fmt, getattr(mod, src.name).detach().view(src.shape), src, image, scale)
                _release(mod, src.name)
            _register(mod, step, image, scale)
    for p in mod.parameters():   # the biases: inference only, nothing here takes a gradient any more
        p.requires_grad_(False)
    setattr(mod, fmt.flag, True)
    setattr(mod, fmt.switch, True)
    return mod


def _freeze_empty(mod, fmt):
    """the frozen form with unwritten buffers, for a state dict to fill"""
    for step in getattr(mod, fmt.steps)():
        dev = getattr(mod, step.sources[0].name).device
        E = step.sources[0].shape[0]
        for src in step.sources:
            _release(mod, src.name)
        (ishape, idtype), (sshape, sdtype) = fmt.buffers(step, E)
        _register(mod, step, torch.empty(ishape, dtype=idtype, device=dev), torch.empty(sshape, dtype=sdtype, device=dev))
    mod.invalidate_prepacked()
    for p in mod.parameters():   # the biases: inference only, nothing here takes a gradient any more
        p.requires_grad_(False)
    setattr(mod, fmt.flag, True)
    setattr(mod, fmt.switch, True)


def load_from_state_dict(mod, super_load, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
    """_load_from_state_dict of both expert classes.  FP8 (or FP4) keys into an unfrozen module: it is frozen first in that format
    (its own static rungs decide, a refusal is a loading error), then the default copy fills the buffers.  16-bit keys into a frozen
    module: each tensor is quantised into the module's buffers by the format's HIP quantiser, straight from the checkpoint (a CPU
    tensor is moved to the device one parameter at a time); mismatches are reported as load_state_dict reports them"""
    mod.invalidate_prepacked()
    fmt = resident(mod)
    for cand in FORMATS if fmt is None else ():
        steps = getattr(mod, cand.steps)()
        has8 = any(prefix + step.buffer in state_dict for step in steps)
        has16 = any(prefix + src.name in state_dict for step in steps for src in step.sources)
        if has8 and not has16:
            why = getattr(mod, cand.static_refusal)()
            if why is not None:
                error_msgs.append(f"{prefix or 'experts'}: the state dict holds {cand.name}-resident experts, which this module cannot become: {why}")
                return
            _freeze_empty(mod, cand)
            fmt = cand
            break
    if fmt is not None:
        steps = getattr(mod, fmt.steps)()
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
                    error_msgs.append(f"dtype mismatch for {key}: the checkpoint holds {t.dtype}, the {fmt.name}-resident module was frozen "
                                      f"from {here.dtype} (quantising another dtype gives other codes).")
                else:
                    try:
                        with torch.no_grad():
                            _quantise(fmt, t.detach().to(image.device).view(src.shape), src, image, scale)
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
    fmt = resident(mod)
    if fmt is None:
        return
    image = getattr(mod, getattr(mod, fmt.steps)()[0].buffer)
    probes = [torch.empty(0, dtype=dt, device=image.device) for dt in (torch.float32, mod._fp8_dtype())]
    if any(out.dtype != p.dtype or out.device != p.device for p, out in ((p, fn(p)) for p in probes)):
        raise RuntimeError(fmt.no_apply)
