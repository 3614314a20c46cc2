// w4_image.h -- the MXFP4 weight image (include/tutel_amd.h; tutel_amd/experts/w4.py::pack) as the kernels that stream it share it:
// the kernel arguments, a lane's ring of K-tiles through exact-size buffer descriptors and the host-side checks of the weight operands.
// Included by expert_gemm_w4.hip (W4A16: the ring's tiles are widened to 16 bit) and expert_gemm_w4a8.hip (W4A8: they go into the
// block-scaled matrix instruction as stored).
#pragma once
#include "gemm_wstream.h"

struct W4Args {
  const unsigned char *A; long long a_stride_e; int lda;     // in the format's own unit: 16-bit elements (W4A16), bytes (W4A8)
  const unsigned char *Wq; long long w_stride_e;             // bytes
  const unsigned char *Ws; long long s_stride_e;             // bytes
  const uint16_t *bias; long long bias_stride_e;             // elements
  uint16_t *D; long long d_stride_e; int ldd;                // elements
  int R, N, K, ntm, ntn;
  const int32_t *slot_map; int T; const unsigned char *zero_row;
};

// streamed loads through the channel group's descriptors (each byte is read once by one workgroup per row tile)
__device__ __forceinline__ u32x4 w4_wload(__amdgpu_buffer_rsrc_t rs, int voff) {
  return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 2));
}
__device__ __forceinline__ uint32_t w4_sload(__amdgpu_buffer_rsrc_t rs, int voff) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_raw_buffer_load_b32(rs, voff, 0, 0));
}

// The group's codes are one run of 16 K bytes (K / 64 blocks of 1 KB) and its scales one run of 128 T128 bytes, one descriptor each.
// The K-tile's offset is part of the VECTOR offset: the hardware's range check covers the vector and the immediate offset, not the
// scalar one.  w[d]: dword q holds the lane's codes k = 64 t + 16 q + 8 kg .. + 7; s[d]: the scale bytes of the four 32-blocks of
// k-range [128 (t >> 1), + 128)
struct W4Ring {
  __amdgpu_buffer_rsrc_t rs_w, rs_s;
  int wl, sl;
  u32x4 w[WS_DEPTH];
  uint32_t s[WS_DEPTH];
  __device__ __forceinline__ void open(const W4Args &p, int e, int nt, int lane) {
    const int nk = p.K / WS_BK;
    const int T128 = (p.K + 127) >> 7;   // scale dwords per channel
    rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char *>(p.Wq + (long long)e * p.w_stride_e + (long long)nt * nk * 1024), 0,
                                             nk * 1024, 0x00020000);
    rs_s = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char *>(p.Ws + (long long)e * p.s_stride_e + (long long)nt * T128 * 128), 0,
                                             T128 * 128, 0x00020000);
    wl = lane * 16;
    sl = (lane & 31) * 4;
  }
  __device__ __forceinline__ void load(int d, int t) {
    w[d] = w4_wload(rs_w, wl + t * 1024);
    s[d] = w4_sload(rs_s, sl + (t >> 1) * 128);
  }
};

// the weight operands as an entry point got them (gemm_wstream.h: Fmt::Weights)
struct W4Weights {
  const void *Wq; int64_t w_stride_e; const void *Ws; int64_t s_stride_e;
  bool strides_ok() const { return w_stride_e % 16 == 0 && s_stride_e % 4 == 0; }
  bool image_ok(long long NI, int K) const { return w_stride_e >= NI * K / 2 && s_stride_e >= NI * (((long long)K + 127) / 128) * 4; }
  static bool run_ok(int K) { return (long long)K * 16 <= 0x7fffffffLL; }
  bool present() const { return Wq && Ws; }
  bool aligned() const { return ((uintptr_t)Wq % 16) == 0 && ((uintptr_t)Ws % 4) == 0; }
  void fill(W4Args &a) const {
    a.Wq = (const unsigned char *)Wq; a.w_stride_e = w_stride_e;
    a.Ws = (const unsigned char *)Ws; a.s_stride_e = s_stride_e;
  }
};

#define W4_SMALL "w_stride_e / s_stride_e is smaller than one expert's image (N * K / 2 code bytes, N * ceil(K / 128) * 4 scale bytes)"
#define W4_SMALL_GU "w_stride_e / s_stride_e is smaller than one expert's image (H * K code bytes, 2 * H * ceil(K / 128) * 4 scale bytes)"
