"""OCP MXFP4 expert weights for the W4A16 grouped GEMM (csrc/expert_gemm_w4.hip): the format, the quantiser and the weight image.

Cold path, plain torch, runs on CPU and GPU alike.  A weight is an e2m1 code (sign, 2 exponent bits, 1 mantissa bit) under one e8m0
scale byte per block of 32 values along K:

    w[e, n, k] = val(code[e, n, k]) * 2^(s[e, n, k / 32] - 127)          val in +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}

The kernel multiplies the 16-bit activations with the EXACT value of every weight -- the scale is a power of two and, for the scale
bytes check_scales admits, every product is a normal number of the activations' dtype (the contract of include/tutel_amd.h) -- so
what is written here, which code and which scale byte a weight gets, is the whole of the quantisation's numerics.

The STANDARD layout (what quantize_mxfp4 returns and the public MXFP4 checkpoints ship): codes uint8 [E, N, K / 2], element 2 j in
the low nibble of byte j and element 2 j + 1 in the high nibble; scales uint8 [E, N, K / 32].

The IMAGE is the kernel's own layout (include/tutel_amd.h), per expert
    codes  [N / 32][K / 64][64 lanes][16 bytes]: lane l of block (g, t) holds channel 32 g + (l & 31); dword q of its 16 bytes holds
           the eight codes k = 64 t + 16 q + 8 (l >> 5) + j, j the nibble index (low nibble of the lowest byte first);
    scales [N / 32][ceil(K / 128)][32 channels][4 bytes]: byte i is the scale of k-block 4 t128 + i; padded with 127.
pack / unpack are pure index operations.  pack takes the standard layout: importing a ready-made MXFP4 checkpoint is
check_scales(scales, dtype) followed by pack(codes, scales).

A SwiGLU expert's gate and up matrices share ONE image of 2 H channels (tutel_amd_expert_gemm_w4_glu): each is quantised on its own,
codes and scale bytes are interleaved by 16 channels (w8.interleave_gate_up) and the result goes through the same pack.
"""
import torch

from .w8 import interleave_gate_up

BLOCK = 32
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
SCALE_ONE = 127
# the scale bytes for which every val * 2^(s - 127) is a NORMAL number of the dtype: 0.5 * 2^e at least the smallest normal and
# 6 * 2^e = 1.5 * 2^(e + 2) at most the largest finite -- bf16 e in [-125, 125], fp16 e in [-13, 13]
SCALE_RANGE = {torch.bfloat16: (2, 252), torch.float16: (114, 140)}


def _lut(device):
    v = torch.tensor(E2M1_VALUES, dtype=torch.float32, device=device)
    return torch.cat([v, -v])


def quantize_mxfp4(w, w_kmajor, dtype=None):
    """w [E, N, K] (w_kmajor) or [E, K, N], bf16 / fp16 / fp32 -> (codes uint8 [E, N, K / 2], scales uint8 [E, N, K / 32]) in the
    standard MX layout, for activations of `dtype` (bf16 / fp16; default: w's own when it is one of them).  Per block of 32 along K,
    in fp32: amax == 0 -> s = 127 and codes 0; else e = floor(log2(amax)) - 2 (from the fp32 exponent field) clamped to the dtype's
    admitted range, the code is w / 2^e rounded to nearest-even on the e2m1 grid (a tie goes to the neighbour with mantissa bit 0)
    and saturated at +-6.  A value that rounds to zero gets code 0x0 whatever its sign (-0 included): the image holds no negative zero."""
    assert w.dim() == 3 and w.dtype in (torch.float32, torch.bfloat16, torch.float16)
    dtype = w.dtype if dtype is None else dtype
    assert dtype in SCALE_RANGE, "quantize_mxfp4: the activations' dtype must be bf16 or fp16"
    w = w.detach()
    if not w_kmajor:
        w = w.transpose(1, 2)
    E, N, K = w.shape
    assert K % BLOCK == 0, "quantize_mxfp4: K must be a multiple of 32"
    wf = w.float().contiguous().view(E, N, K // BLOCK, BLOCK)
    amax = wf.abs().amax(dim=3)
    if not bool(torch.isfinite(amax).all()):   # amax is NaN / inf exactly when its block holds a non-finite weight
        bad = (~torch.isfinite(amax)).nonzero()[0].tolist()
        raise ValueError(f"quantize_mxfp4: channel (expert {bad[0]}, output {bad[1]}) holds a non-finite weight")
    lo, hi = SCALE_RANGE[dtype]
    s = ((amax.view(torch.int32) >> 23) & 0xff) - 2           # floor(log2(amax)) - 2 + 127 (an fp32 subnormal: below every range)
    s = torch.where(amax == 0, torch.full_like(s, SCALE_ONE), s.clamp(lo, hi))
    x = wf / (s << 23).view(torch.float32).unsqueeze(3)       # a division by a power of two
    a = x.abs()
    # the grid's midpoints; a tie belongs to the even neighbour: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4
    idx = ((a > 0.25).to(torch.uint8) + (a >= 0.75).to(torch.uint8) + (a > 1.25).to(torch.uint8) + (a >= 1.75).to(torch.uint8) +
           (a > 2.5).to(torch.uint8) + (a >= 3.5).to(torch.uint8) + (a > 5.0).to(torch.uint8))
    code = idx | (((x < 0) & (idx > 0)).to(torch.uint8) << 3)
    code = code.view(E, N, K // 2, 2)
    return (code[..., 0] | (code[..., 1] << 4)).contiguous(), s.to(torch.uint8).contiguous()


def unpack_nibbles(codes):
    """codes uint8 [..., K / 2] -> uint8 [..., K], one code per element"""
    return torch.stack([codes & 0xf, codes >> 4], dim=-1).view(*codes.shape[:-1], 2 * codes.shape[-1])


def dequantize(codes, scales, dtype=torch.float32):
    """the weights the kernel multiplies with, as [E, N, K] in `dtype`: val(code) times the fp32 with bits s << 23 -- 2^(s - 127) for
    1 <= s <= 254, the operand the kernel hands to the convert.  Exact in fp32, and in bf16 / fp16 for the scale bytes check_scales
    admits for them."""
    assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8 and codes.dim() == 3
    E, N, K2 = codes.shape
    assert scales.shape == (E, N, 2 * K2 // BLOCK)
    val = _lut(codes.device)[unpack_nibbles(codes).long()].view(E, N, -1, BLOCK)
    two = (scales.to(torch.int32) << 23).view(torch.float32)
    return (val * two.unsqueeze(3)).view(E, N, 2 * K2).to(dtype)


def check_scales(scales, dtype):
    """refuse a scale byte outside the dtype's admitted range (0xFF, the e8m0 NaN, included): ValueError naming expert, channel, block"""
    assert scales.dtype == torch.uint8 and scales.dim() == 3 and dtype in SCALE_RANGE
    lo, hi = SCALE_RANGE[dtype]
    bad = (scales < lo) | (scales > hi)
    if bool(bad.any()):
        e, n, b = bad.nonzero()[0].tolist()
        raise ValueError(f"check_scales: scale byte {int(scales[e, n, b])} of (expert {e}, channel {n}, block {b}) is outside "
                         f"[{lo}, {hi}], the range in which every MXFP4 value is a normal {str(dtype).split('.')[-1]} number")


def scale_dwords(K):
    return (K + 127) // 128


def pack(codes, scales):
    """the standard layout -> the kernel's image: (codes uint8 [E, N / 32, K / 64, 64, 16], scales uint8 [E, N / 32, ceil(K / 128), 32, 4]);
    N % 32 == 0 and K % 64 == 0 (the shapes the kernel covers).  A ready-made MXFP4 checkpoint in the standard layout is imported by
    check_scales(scales, dtype) followed by this function."""
    assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8 and codes.dim() == 3
    E, N, K2 = codes.shape
    K = 2 * K2
    assert N % 32 == 0 and K % 64 == 0, "the W4A16 image needs N % 32 == 0 and K % 64 == 0"
    assert scales.shape == (E, N, K // BLOCK)
    # codes [E, g, l31, t, q, kg, b] -> [E, g, t, kg, l31, q, b]: lane = 32 kg + l31, byte = 4 q + b (k = 64 t + 16 q + 8 kg + 2 b + nibble)
    ci = codes.contiguous().view(E, N // 32, 32, K // 64, 4, 2, 4).permute(0, 1, 3, 5, 2, 4, 6).contiguous().view(E, N // 32, K // 64, 64, 16)
    T = scale_dwords(K)
    sc = scales
    if 4 * T != K // BLOCK:
        sc = torch.nn.functional.pad(sc, (0, 4 * T - K // BLOCK), value=SCALE_ONE)
    si = sc.contiguous().view(E, N // 32, 32, T, 4).permute(0, 1, 3, 2, 4).contiguous()
    return ci, si


def unpack(image_codes, image_scales, N, K):
    """the inverse of pack: the image -> (codes [E, N, K / 2], scales [E, N, K / 32]), the pad bytes dropped"""
    E = image_codes.size(0)
    T = scale_dwords(K)
    assert image_codes.dtype == torch.uint8 and image_codes.numel() == E * N * K // 2
    assert image_scales.dtype == torch.uint8 and image_scales.numel() == E * N * T * 4
    codes = image_codes.view(E, N // 32, K // 64, 2, 32, 4, 4).permute(0, 1, 4, 2, 5, 3, 6).contiguous().view(E, N, K // 2)
    scales = image_scales.view(E, N // 32, T, 32, 4).permute(0, 1, 3, 2, 4).contiguous().view(E, N, 4 * T)
    return codes, scales[:, :, :K // BLOCK].contiguous()


def prepare(w, w_kmajor, dtype=None):
    """quantise and lay out one parameter: (image codes, image scales) as the kernel reads them"""
    return pack(*quantize_mxfp4(w, w_kmajor, dtype))


def prepare_gate_up(w_gate, w_up, w_kmajor, dtype=None):
    """quantise a SwiGLU expert's gate and up parameters, each on its own, and lay them out as ONE image of 2 H channels:
    pack(interleave(codes_gate, codes_up), interleave(scales_gate, scales_up))"""
    cg, sg = quantize_mxfp4(w_gate, w_kmajor, dtype)
    cu, su = quantize_mxfp4(w_up, w_kmajor, dtype)
    return pack(interleave_gate_up(cg, cu), interleave_gate_up(sg, su))
