"""The per-row activation quantiser (csrc/quantize_a8.hip, tutel_amd_quantize_rows_a8) on the MI355X: bit for bit
experts/w8.py::quantize_e4m3 on the CPU -- one, three and more rows than a workgroup holds, every register-count variant, strided
rows -- the rows the rounding can get wrong, and the non-finite row's contract."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _packed_fuzz import moat_intact, moated  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]


def _quantise(x, ldx):
    """x [rows, K] on the CPU -> (codes, scale) from the device, x inside a [rows, ldx] buffer and every operand inside guard bands"""
    from tutel_amd import ops
    rows, K = x.shape
    wide = torch.full([rows, ldx], float("nan"), dtype=x.dtype)
    wide[:, :K] = x
    xd = moated(wide, device=torch.device("cuda"))[:, :K]
    out = moated(torch.full([rows, K], 0xAB, dtype=torch.uint8), fill=0xAB, device=torch.device("cuda"))
    scale = moated(torch.full([rows], -7.0), fill=-7.0, device=torch.device("cuda"))
    assert ops.quantize_rows_a8_supported(x.dtype, K)
    got = ops.quantize_rows_a8(xd, out=out, scale=scale)
    assert got is not None and got[0] is out and got[1] is scale
    torch.cuda.synchronize()
    moat_intact(out, "the codes")
    moat_intact(scale, "the scales")
    return out.cpu(), scale.cpu()


def _reference(x):
    from tutel_amd.experts import w8
    q, scale = w8.quantize_e4m3(x.unsqueeze(0), True)
    return q[0].view(torch.uint8), scale[0]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("K", [64, 192, 2048, 4096])
@pytest.mark.parametrize("rows", [1, 3, 130])
def test_rows_are_quantised_bit_for_bit_as_on_the_cpu(rows, K, dtype):
    g = torch.Generator().manual_seed(131 * rows + K)
    # magnitudes over many binades, so that quotients land in the subnormal range of e4m3 as well
    x = (torch.randn([rows, K], generator=g) * torch.pow(2.0, torch.randint(-12, 3, [rows, K], generator=g).float())).to(dtype)
    codes, scale = _quantise(x, K + 8)
    want_codes, want_scale = _reference(x)
    assert torch.equal(scale.view(torch.int32), want_scale.view(torch.int32)), "scales"
    assert torch.equal(codes, want_codes), "codes"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_zero_row_ties_subnormals_and_a_non_finite_row(dtype):
    K = 64
    x = torch.zeros([4, K])
    # row 1: amax 448 -> scale 1: the quotients ARE the values.  Ties between neighbouring codes (17: 16 | 18, 22.0: 20 | 24 ...), ties
    # and values in the subnormal range (spacing 2^-9), the smallest normal, +-0
    ties = [448.0, 17.0, -17.0, 19.0, 22.0, 26.0, 416.0, 432.0, -432.0, 2.0 ** -10, -2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10,
            2.0 ** -9, 7 * 2.0 ** -9, 15 * 2.0 ** -10, 2.0 ** -6, 2.0 ** -6 + 2.0 ** -10, 2.0 ** -11, -0.0, 1.0625, 1.1875]
    x[1, :len(ties)] = torch.tensor(ties)
    x[2] = torch.randn([K], generator=torch.Generator().manual_seed(5))
    x[3] = x[2]
    x = x.to(dtype)
    assert torch.equal(x[1, :len(ties)].float(), torch.tensor(ties)), "the tie row is exact in the dtype"
    want_codes, want_scale = _reference(x)
    assert float(want_scale[0]) == 1.0 and float(want_scale[1]) == 1.0 and bool((want_codes[0] == 0).all())
    x[3, 17] = float("inf")
    codes, scale = _quantise(x, K + 24)
    assert torch.equal(scale[:3].view(torch.int32), want_scale[:3].view(torch.int32)), "scales"
    assert torch.equal(codes[:3], want_codes[:3]), "codes"
    assert bool(torch.isnan(scale[3])) and bool((codes[3] == 0x7F).all()), "a non-finite row: scale NaN, the NaN code throughout"


def test_refusals():
    from tutel_amd import ops
    dev = torch.device("cuda")
    assert not ops.quantize_rows_a8_supported(torch.float32, 64) and not ops.quantize_rows_a8_supported(torch.bfloat16, 96)
    assert not ops.quantize_rows_a8_supported(torch.bfloat16, 8192 + 64) and ops.quantize_rows_a8_supported(torch.float16, 8192)
    for x in (torch.ones([2, 96], dtype=torch.bfloat16, device=dev), torch.ones([2, 64], dtype=torch.float32, device=dev)):
        out = torch.full(list(x.shape), 0xAB, dtype=torch.uint8, device=dev)
        assert ops.quantize_rows_a8(x, out=out) is None and bool((out == 0xAB).all())
