"""FP8 (OCP e4m3fn) expert weights for the W8A16 grouped GEMM (csrc/expert_gemm_w8.hip): the quantiser and the weight image.

Cold path, plain torch, runs on CPU and GPU (the reference of the HIP quantiser at the end of this file, which writes the same bits
on the device without the intermediate copies).  The kernel multiplies the 16-bit activations with the EXACT value of every e4m3 code
(widened to bf16 / fp16) and applies the per-channel scale once per output in fp32 (the contract of include/tutel_amd.h), so what
is written here -- which code and which scale a weight gets -- is the whole of the quantisation's numerics.

    scale[e, n] = fp32(amax_k |w[e, n, k]|) / 448.0f           (an all-zero channel: 1)
    q[e, n, k]  = e4m3_rne(clamp(fp32(w[e, n, k]) / scale[e, n], -448, 448))

The clamp is needed: the division can round a quotient a little above 448, and torch's cast turns anything above 464 into the NaN
code.  Everything is elementwise or a max-reduction in fp32: deterministic.

The image is the kernel's own layout (include/tutel_amd.h): per expert [N / 32][K / 32][64 lanes][16 bytes], byte b of lane l of
block (g, t) = the code of channel 32 g + (l & 31) at k = 32 t + 16 (b >> 3) + 8 (l >> 5) + (b & 7); N and K padded up to multiples of
32 with code 0x00.  pack / unpack are pure index operations.

A SwiGLU expert's gate and up matrices share ONE image of 2 H channels (tutel_amd_expert_gemm_w8_glu): each is quantised on its own,
the channels are interleaved by 16 (interleave_gate_up) and the result goes through the same pack.
"""
import torch

E4M3_MAX = 448.0
TILE_N = 32
TILE_K = 32


def quantize_e4m3(w, w_kmajor):
    """w [E, N, K] (w_kmajor) or [E, K, N], 16-bit or fp32 -> (q_nk [E, N, K] float8_e4m3fn, scale [E, N] fp32)"""
    assert w.dim() == 3 and w.dtype in (torch.float32, torch.bfloat16, torch.float16)
    w = w.detach()
    if not w_kmajor:
        w = w.transpose(1, 2)
    wf = w.float().contiguous()
    amax = wf.abs().amax(dim=2)
    if not bool(torch.isfinite(amax).all()):   # amax is NaN / inf exactly when its channel holds a non-finite weight
        bad = (~torch.isfinite(amax)).nonzero()[0].tolist()
        raise ValueError(f"quantize_e4m3: channel (expert {bad[0]}, output {bad[1]}) holds a non-finite weight")
    # tensor / tensor: a true fp32 division on every device (a Python-scalar divisor is turned into a multiplication by its rounded
    # reciprocal on the GPU, which moves some scales by an ulp and with them the codes that sit on a rounding tie)
    scale = amax / torch.full_like(amax, E4M3_MAX)
    scale = torch.where(amax == 0, torch.ones_like(scale), scale)
    q = (wf / scale.unsqueeze(2)).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return q, scale


def dequantize(q_nk, scale, dtype=torch.float32):
    """the weights the kernel multiplies with, q * scale, as [E, N, K] in `dtype` (exact in fp32 up to the one product's rounding)"""
    return (q_nk.float() * scale.unsqueeze(2)).to(dtype)


def padded(n, tile):
    return (n + tile - 1) // tile * tile


def pack(q_nk):
    """q_nk [E, N, K] float8_e4m3fn -> the kernel's image, uint8 [E, Np / 32, Kp / 32, 64, 16] contiguous (Np, Kp: N, K padded to 32)"""
    assert q_nk.dim() == 3 and q_nk.dtype == torch.float8_e4m3fn
    E, N, K = q_nk.shape
    Np, Kp = padded(N, TILE_N), padded(K, TILE_K)
    b = q_nk.contiguous().view(torch.uint8)
    if (Np, Kp) != (N, K):
        b = torch.nn.functional.pad(b, (0, Kp - K, 0, Np - N), value=0)
    # [E, g, l31, t, s, kg, j] -> [E, g, t, kg, l31, s, j]: lane = 32 kg + l31, byte = 8 s + j
    b = b.view(E, Np // 32, 32, Kp // 32, 2, 2, 8).permute(0, 1, 3, 5, 2, 4, 6)
    return b.contiguous().view(E, Np // 32, Kp // 32, 64, 16)


def unpack(image, N, K):
    """the inverse of pack: image -> q_nk [E, N, K] float8_e4m3fn (the pad bytes dropped)"""
    E = image.size(0)
    Np, Kp = padded(N, TILE_N), padded(K, TILE_K)
    assert image.dtype == torch.uint8 and image.numel() == E * Np * Kp
    b = image.view(E, Np // 32, Kp // 32, 2, 32, 2, 8).permute(0, 1, 4, 2, 5, 3, 6).contiguous().view(E, Np, Kp)
    return b[:, :N, :K].contiguous().view(torch.float8_e4m3fn)


def prepare(w, w_kmajor):
    """quantise and lay out one parameter: (image, scale) as the kernel reads them"""
    q, scale = quantize_e4m3(w, w_kmajor)
    return pack(q), scale.contiguous()


# ---- SwiGLU experts: gate and up in one image (tutel_amd_expert_gemm_w8_glu) ------------------------------------------------------------
# Register 4 rg + r of a lane's 32 x 32 accumulator is image channel 32 nt + 8 rg + 4 kg + r (kg = lane >> 5).  With the two matrices
# interleaved by GLU_GROUP channels -- in every 32-channel group, position p < 16 gate channel 16 g + p, position 16 + p up channel
# 16 g + p -- registers rg = 0, 1 of a lane are gate channels 16 g + 8 rg + 4 kg + r and registers rg + 2 the up channels of the same
# indices: the gating product is register against register.  Only the channel order changes; the bytes below it are pack's.
GLU_GROUP = 16


def interleave_gate_up(gate, up):
    """gate, up [E, H, ...] (codes [E, H, K] or scales [E, H]) -> [E, 2 H, ...]: blocks of 16 channels, gate then up; H % 16 == 0"""
    assert gate.shape == up.shape and gate.dtype == up.dtype and gate.dim() >= 2
    if gate.dtype == torch.float8_e4m3fn:   # codes move as bytes
        return interleave_gate_up(gate.view(torch.uint8), up.view(torch.uint8)).view(torch.float8_e4m3fn)
    E, H = gate.shape[:2]
    assert H % GLU_GROUP == 0, "the gate / up image needs H % 16 == 0"
    rest = tuple(gate.shape[2:])
    both = torch.stack([gate.reshape(E, H // GLU_GROUP, GLU_GROUP, *rest), up.reshape(E, H // GLU_GROUP, GLU_GROUP, *rest)], dim=2)
    return both.reshape(E, 2 * H, *rest)


def deinterleave_gate_up(both):
    """the inverse of interleave_gate_up: [E, 2 H, ...] -> (gate, up) [E, H, ...]"""
    if both.dtype == torch.float8_e4m3fn:
        return tuple(t.view(torch.float8_e4m3fn) for t in deinterleave_gate_up(both.view(torch.uint8)))
    E, N = both.shape[:2]
    assert N % (2 * GLU_GROUP) == 0
    rest = tuple(both.shape[2:])
    b = both.reshape(E, N // (2 * GLU_GROUP), 2, GLU_GROUP, *rest)
    return b[:, :, 0].reshape(E, N // 2, *rest), b[:, :, 1].reshape(E, N // 2, *rest)


def prepare_gate_up(w_gate, w_up, w_kmajor):
    """quantise a SwiGLU expert's gate and up parameters, each on its own (its own per-channel scales), and lay them out as ONE image:
    (pack(interleave(q_gate, q_up)), interleave(scale_gate, scale_up) [E, 2 H] fp32)"""
    qg, sg = quantize_e4m3(w_gate, w_kmajor)
    qu, su = quantize_e4m3(w_up, w_kmajor)
    return pack(interleave_gate_up(qg, qu)), interleave_gate_up(sg, su).contiguous()


# ---- the HIP quantiser (csrc/quantize_w8.hip, tutel_amd_quantize_w8) ------------------------------------------------------------------------
# The functions above hold an fp32 copy of the parameter, its codes and two permuted copies at once: several times the parameter's
# size.  The kernel reads the parameter as stored and writes image and scales directly, the same bits.  Where the library does not
# cover the call (a CPU tensor, K or the channel count no multiple of 32) the torch functions answer, with the same return types.
def glu_channel_map(H, up):
    """the channel map of one half of a gate / up image of 2 H channels: (image_channels, group, group_stride, group_offset) --
    interleave_gate_up's order, c(n) = (n / 16) * 32 + 16 * up + n % 16"""
    return (2 * H, GLU_GROUP, 2 * GLU_GROUP, GLU_GROUP if up else 0)


def prepare_native(w, w_kmajor):
    """prepare(w, w_kmajor) by the HIP quantiser where it covers the call"""
    if w.is_cuda:
        from .. import ops
        res = ops.quantize_w8(w.detach(), w_kmajor)
        if res is not None:
            return res
    return prepare(w, w_kmajor)


def prepare_gate_up_native(w_gate, w_up, w_kmajor):
    """prepare_gate_up(w_gate, w_up, w_kmajor) by the HIP quantiser where it covers the call: two launches into one image"""
    if w_gate.is_cuda and w_up.is_cuda and w_gate.shape == w_up.shape and w_gate.dtype == w_up.dtype:
        from .. import ops
        H = w_gate.shape[1] if w_kmajor else w_gate.shape[2]
        res = ops.quantize_w8(w_gate.detach(), w_kmajor, channel_map=glu_channel_map(H, False))
        if res is not None:
            res = ops.quantize_w8(w_up.detach(), w_kmajor, image=res[0], scale=res[1], channel_map=glu_channel_map(H, True))
            if res is not None:
                return res
    return prepare_gate_up(w_gate, w_up, w_kmajor)
