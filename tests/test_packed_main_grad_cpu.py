"""Accumulating the packed weight / bias gradients into an fp32 main_grad, without a GPU: the two *_acc_f32 entry points on the
C-ABI boundary (declared, exported, bound; refusals and argument errors before anything is enqueued), the accumulate_into checks
of ops, and the host logic of impls/packed_train: main_grad_problem, attach_main_grads / zero_main_grads, and unsupported's
answers, which the new switch leaves as they were."""
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tutel_amd_expert_wgrad_packed_acc_f32", "tutel_amd_expert_bgrad_packed_acc_f32")


@pytest.fixture(scope="module")
def L():
    from tutel_amd import _lib
    _lib.build()
    return _lib.lib()


def test_acc_symbols_declared_exported_bound(L):
    from tutel_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tutel_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        m = re.search(r"\b" + n + r"\s*\(([^)]*)\)", hdr)
        assert m is not None, n
        assert hasattr(raw, n), n
        assert len(_lib.SIGNATURES[n][1]) == m.group(1).count(",") + 1, n
        # the argument list of the _f32 sibling
        sib = n.replace("_acc_f32", "_f32")
        ms = re.search(r"\b" + sib + r"\s*\(([^)]*)\)", hdr)
        assert re.sub(r"\s+", " ", m.group(1)) == re.sub(r"\s+", " ", ms.group(1)), n
        assert [a for a in _lib.SIGNATURES[n][1]] == [a for a in _lib.SIGNATURES[sib][1]], n


def test_acc_argument_errors_before_any_launch(L):
    from tutel_amd import _lib
    ENOTSUP = _lib.ENOTSUP
    wg, bg = L.tutel_amd_expert_wgrad_packed_acc_f32, L.tutel_amd_expert_bgrad_packed_acc_f32
    fake, odd = 1 << 20, (1 << 20) + 8      # never dereferenced: every call below returns before a launch
    # fp32 operands: not covered (16-bit operands only)
    assert wg(None, 128, None, 128, None, 0, 0, None, None, 8, 64, 128, 128, _lib.F32, None, None) == ENOTSUP
    assert b"16-bit" in L.tutel_amd_last_error() and b"_acc_f32" in L.tutel_amd_last_error()
    assert bg(None, 128, None, 8, 128, _lib.F32, None, None) == ENOTSUP
    assert b"16-bit" in L.tutel_amd_last_error() and b"_acc_f32" in L.tutel_amd_last_error()
    # N % 8, in either extent and in a leading dimension
    assert wg(None, 128, None, 128, None, 0, 0, None, None, 8, 64, 128, 100, _lib.BF16, None, None) == ENOTSUP
    assert b"multiples of 8" in L.tutel_amd_last_error()
    assert wg(None, 128, None, 128, None, 0, 0, None, None, 8, 64, 100, 128, _lib.F16, None, None) == ENOTSUP
    assert b"multiples of 8" in L.tutel_amd_last_error()
    assert wg(None, 132, None, 128, None, 0, 0, None, None, 8, 64, 128, 128, _lib.F16, None, None) == ENOTSUP
    assert b"multiples of 8" in L.tutel_amd_last_error()
    # a bad gather code, and a gather without its map, are argument errors
    assert wg(None, 128, None, 128, None, 3, 4, None, None, 8, 64, 128, 128, _lib.BF16, None, None) not in (0, ENOTSUP)
    assert b"bad sizes" in L.tutel_amd_last_error()
    assert wg(fake, 128, fake, 128, None, 2, 4, fake, fake, 8, 64, 128, 128, _lib.BF16, fake, None) not in (0, ENOTSUP)
    # null pointers: all, D alone, the zero row of a gathered operand
    assert wg(None, 128, None, 128, None, 0, 0, None, None, 8, 64, 128, 128, _lib.BF16, None, None) not in (0, ENOTSUP)
    assert b"null" in L.tutel_amd_last_error()
    assert wg(fake, 128, fake, 128, None, 0, 0, None, None, 8, 64, 128, 128, _lib.BF16, fake, None) not in (0, ENOTSUP)
    assert b"null" in L.tutel_amd_last_error()
    assert wg(fake, 128, fake, 128, fake, 1, 4, None, fake, 8, 64, 128, 128, _lib.BF16, fake, None) not in (0, ENOTSUP)
    assert b"null" in L.tutel_amd_last_error()
    assert bg(fake, 128, None, 8, 128, _lib.BF16, fake, None) not in (0, ENOTSUP)
    assert b"null" in L.tutel_amd_last_error()
    # D 8-byte but not 16-byte aligned: the epilogue moves 16 bytes
    assert wg(fake, 128, fake, 128, None, 0, 0, None, odd, 8, 64, 128, 128, _lib.BF16, fake, None) not in (0, ENOTSUP)
    assert b"16-byte" in L.tutel_amd_last_error()
    assert bg(fake, 128, odd, 8, 128, _lib.BF16, fake, None) not in (0, ENOTSUP)
    assert b"16-byte" in L.tutel_amd_last_error()


def test_ops_accumulate_into_is_checked_before_the_library(monkeypatch):
    from tutel_amd import _lib, ops

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", no_library)
    lay = types.SimpleNamespace(E=4)
    a, b = torch.zeros(16, 8, dtype=torch.bfloat16), torch.zeros(16, 24, dtype=torch.bfloat16)
    good = torch.zeros(4, 8, 24)
    for bad, word in [(good.to(torch.bfloat16), "float32"), (good.double(), "float32"), (torch.zeros(4, 8, 16), "elements"),
                      (torch.zeros(4, 8, 48)[:, :, ::2], "contiguous"), ([0.0], "float32")]:
        with pytest.raises(_lib.TutelAmdError, match=word):
            ops.expert_wgrad_packed(a, b, lay, accumulate_into=bad)
    with pytest.raises(_lib.TutelAmdError, match="out_dtype"):
        ops.expert_wgrad_packed(a, b, lay, out_dtype=torch.bfloat16, accumulate_into=good)
    for bad, word in [(torch.zeros(4, 24, dtype=torch.float16), "float32"), (torch.zeros(4, 16), "elements"),
                      (torch.zeros(4, 48)[:, ::2], "contiguous")]:
        with pytest.raises(_lib.TutelAmdError, match=word):
            ops.expert_bgrad_packed(b, lay, accumulate_into=bad)
    with pytest.raises(_lib.TutelAmdError, match="out_dtype"):
        ops.expert_bgrad_packed(b, lay, out_dtype=torch.bfloat16, accumulate_into=torch.zeros(4, 24))
    # a good target on the wrong device (the operands are not on the HIP device either: refused all the same, before the library)
    with pytest.raises(_lib.TutelAmdError):
        ops.expert_wgrad_packed(a, b, lay, accumulate_into=good)
    with pytest.raises(_lib.TutelAmdError, match="is on"):
        ops._grad_acc_target(good, good.numel(), None, torch.device("meta"), "expert_wgrad_packed")
    assert good.abs().sum() == 0


def _layer(M=256, H=256, E=8, k=2, dtype=torch.bfloat16, experts="ffn", **kw):
    from tutel import moe
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        spec = {"type": experts, "num_experts_per_device": E, "hidden_size_per_expert": H}
        if experts == "ffn":
            spec["activation_fn"] = kw.pop("act", torch.nn.functional.relu)
        layer = moe.moe_layer(gate_type=dict({"type": "top", "k": k, "capacity_factor": 0.0}, **kw.pop("gate", {})), experts=spec,
                              model_dim=M, **kw)
    finally:
        torch.set_default_dtype(old)
    return layer.train()


def test_switch_defaults_off_and_follows_the_environment(monkeypatch):
    assert _layer().dropless_packed_main_grad is False
    monkeypatch.setenv("TUTEL_AMD_PACKED_MAIN_GRAD", "1")
    assert _layer().dropless_packed_main_grad is True
    monkeypatch.setenv("TUTEL_AMD_PACKED_MAIN_GRAD", "0")
    assert _layer().dropless_packed_main_grad is False


def test_main_grad_problem_names_each_reason():
    from tutel_amd.impls import packed_train
    for dtype in (torch.bfloat16, torch.float32):
        layer = _layer(dtype=dtype)
        params = dict(layer.experts.named_parameters())
        assert set(params) == {"batched_fc1_w", "batched_fc2_w", "batched_fc1_bias", "batched_fc2_bias"}
        why = packed_train.main_grad_problem(layer)
        assert "no main_grad" in why and "batched_fc1_w" in why
        packed_train.attach_main_grads(layer)
        assert packed_train.main_grad_problem(layer) is None
        for name, p in params.items():
            assert p.main_grad.dtype == torch.float32 and p.main_grad.shape == p.shape and p.main_grad.is_contiguous()
            assert p.main_grad.device == p.device and not p.main_grad.requires_grad
            assert int((p.main_grad != 0).sum()) == 0 and p.grad is None and p.grad_added_to_main_grad is False
        w2 = params["batched_fc2_w"]
        good = w2.main_grad
        # one parameter without: named
        del w2.main_grad
        why = packed_train.main_grad_problem(layer)
        assert "no main_grad" in why and "batched_fc2_w" in why
        w2.main_grad = good.to(torch.bfloat16)
        assert "torch.bfloat16" in packed_train.main_grad_problem(layer) and "float32" in packed_train.main_grad_problem(layer)
        w2.main_grad = good[:, :, :-8].contiguous()
        assert "shape" in packed_train.main_grad_problem(layer)
        w2.main_grad = good.view(-1)
        assert "shape" in packed_train.main_grad_problem(layer)
        w2.main_grad = torch.zeros(good.shape[0], good.shape[2], good.shape[1]).transpose(1, 2)
        assert w2.main_grad.shape == w2.shape and "contiguous" in packed_train.main_grad_problem(layer)
        w2.main_grad = torch.zeros(good.shape, device="meta")
        assert "is on meta" in packed_train.main_grad_problem(layer)
        w2.main_grad = good
        assert packed_train.main_grad_problem(layer) is None
        # a frozen parameter needs none
        b1 = params["batched_fc1_bias"]
        del b1.main_grad
        assert "batched_fc1_bias" in packed_train.main_grad_problem(layer)
        b1.requires_grad_(False)
        assert packed_train.main_grad_problem(layer) is None


def test_attach_and_zero_main_grads():
    from tutel_amd.impls import packed_train
    layer = _layer(dtype=torch.float16)
    frozen = layer.experts.batched_fc2_bias.requires_grad_(False)
    packed_train.attach_main_grads(layer)
    assert not hasattr(frozen, "main_grad")
    assert not hasattr(layer.gates[0].wg.weight, "main_grad")        # the router keeps its ordinary gradient
    live = [p for p in layer.experts.parameters() if p.requires_grad]
    assert len(live) == 3
    ptrs = [p.main_grad.data_ptr() for p in live]
    for p in live:
        assert p.main_grad.dtype == torch.float32 and p.main_grad.shape == p.shape and int((p.main_grad != 0).sum()) == 0
        p.main_grad.add_(3.0)
        p.grad_added_to_main_grad = True
    packed_train.zero_main_grads(layer)
    for p, ptr in zip(live, ptrs):
        assert int((p.main_grad != 0).sum()) == 0 and p.main_grad.data_ptr() == ptr      # in place: a captured graph keeps its target
        assert p.grad_added_to_main_grad is False
    packed_train.zero_main_grads(_layer())                                                # nothing attached: nothing to do


def _why(layer, T=512, E=8, k=2, M=256, dtype=torch.bfloat16, cf=0.0, alignment=1, **kw):
    from tutel_amd.impls import packed_train
    return packed_train.unsupported(layer, layer.gates[0], T, E, k, M, dtype, cf, alignment, **kw)


def _set(layer, **kw):
    for n, v in kw.items():
        if n == "gate_noise":
            layer.gates[0].gate_noise = v
        else:
            setattr(layer, n, v)
    return layer


# the answers of packed_train.unsupported for the cases of tests/test_packed_train_cpu.py, as they were before the switch existed
UNSUPPORTED = [
    (lambda: (_layer(), {}), None),
    (lambda: (_layer(gate={"fp32_gate": True}), {}), None),
    (lambda: (_layer(), {"cf": -0.5}), None),
    (lambda: (_layer(dtype=torch.float16), {"dtype": torch.float16}), None),
    (lambda: (_layer(act=torch.nn.functional.gelu), {}), "the packed training step needs the ReLU activation"),
    (lambda: (_layer(act=lambda t: torch.clamp(t, -1.0, 1.0)), {}), "the packed training step needs the ReLU activation"),
    (lambda: (_layer(dtype=torch.float32), {"dtype": torch.float32}), "the packed training step needs bf16 / fp16 experts and tokens in their dtype"),
    (lambda: (_set(_layer(), is_postscore=False), {}), "the packed training step needs is_postscore=True (gates applied in the decode)"),
    (lambda: (_set(_layer(), gate_noise=0.5), {}), "the packed training step needs a LinearTopKGate without gate noise"),
    (lambda: (_set(_layer(), batch_prioritized_routing=True), {}), "the packed training step does not cover batch-prioritised routing"),
    (lambda: (_set(_layer(), is_gshard_loss=False), {}), "the packed training step needs the gshard loss"),
    (lambda: (_set(_layer(), world_size=2), {}), "the packed training step runs on a single rank only"),
    (lambda: (_layer(), {"cf": 1.0}), "the packed training step is dropless only (capacity_factor <= 0)"),
    (lambda: (_layer(), {"on_device": False}), "the packed training step needs a non-empty batch on the HIP device"),
    (lambda: (_layer(), {"T": 0}), "the packed training step needs a non-empty batch on the HIP device"),
]


def test_unsupported_answers_do_not_depend_on_the_switch(L):
    from tutel_amd.impls import packed_train
    for make, expect in UNSUPPORTED:
        layer, kw = make()
        assert layer.dropless_packed_main_grad is False
        off = _why(layer, **kw)
        assert off == expect, (off, expect)
        # neither the switch nor attached main_grads change the answer
        layer.dropless_packed_main_grad = True
        assert _why(layer, **kw) == off
        packed_train.attach_main_grads(layer)
        assert _why(layer, **kw) == off
    # the reasons that come from elsewhere keep their words (SwiGLU's own refusal, the plan's shape rules)
    for switch in (False, True):
        assert "inference" in _why(_set(_layer(experts="llama_ffn"), dropless_packed_main_grad=switch))
        assert "multiples of 64" in _why(_set(_layer(H=160), dropless_packed_main_grad=switch))
        assert "k * E" in _why(_set(_layer(E=4096, k=4), dropless_packed_main_grad=switch), E=4096, k=4)


def test_switch_on_raises_before_any_kernel():
    """with the switch on, a training forward that cannot take the packed step raises its reason before any kernel is reached (a CPU
    layer never can: this runs without a GPU)"""
    from tutel_amd.impls import packed_train
    layer = _layer(M=16, H=16, E=2)
    x = torch.randn(8, 16)
    packed_train.attach_main_grads(layer)
    layer.dropless_packed = True
    layer.dropless_packed_main_grad = True
    with pytest.raises(RuntimeError, match="main_grad.*HIP device"):
        layer(x)
    assert "HIP device" in layer._dropless_packed_ran
    layer.dropless_packed = False
    with pytest.raises(RuntimeError, match="main_grad.*dropless_packed is off"):
        layer(x)
    for p in layer.parameters():
        assert p.grad is None
    for p in layer.experts.parameters():
        assert int((p.main_grad != 0).sum()) == 0 and p.grad_added_to_main_grad is False
