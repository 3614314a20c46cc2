// quantize_w4.hip -- the OCP MXFP4 weight quantiser of the W4A16 grouped GEMMs (expert_gemm_w4.hip): reads a parameter as it is stored
// and writes the GEMM's code image and scale image directly.  The contract -- which scale byte and which e2m1 code a weight gets, bit
// for bit those of tutel_amd/experts/w4.py::quantize_mxfp4 on a CPU, and the images' byte layout -- is in include/tutel_amd.h.
//
// ONE pass: an MX scale covers 32 values along K, so nothing has to be known about the rest of a channel.  One workgroup of 256
// threads owns 32 consecutive source channels x one K chunk of 256 (QW4_KC: four 64-k code tiles, two 128-k scale dwords):
//   load    the 32 x 256 tile, every element once, 16 bytes per lane in the source's own order (k-major source: a wave reads two
//           channel rows of 512 B, fp32 one row of 1 KB; n-major source: a lane holds 8 (fp32: 4) neighbouring channels of one k, a
//           wave covers 16 (8) k rows of 64 (128) B), widened to fp32 bit patterns and written into an LDS tile;
//   turn    every thread is ONE 16-byte lane chunk of the image -- wave t = the chunk's 64-k code tile, lane = channel + 32 x k-half --
//           and reads its 32 values from LDS once: k = 64 t + 16 q + 8 half + j.  Dwords q = 0, 1 lie in MX block 2 t, q = 2, 3 in
//           block 2 t + 1, and the other half of either block is held by lane ^ 32 of the same wave: a block's amax is 16 integer
//           maxima and one cross-lane exchange.  As in quantize_w8.hip the maximum is taken on the BIT PATTERN of |w|, so inf and
//           every NaN come out on top and one comparison against 0x7f800000 finds a non-finite block (one atomicMin of e * N + n);
//   codes   from the same registers; a wave stores 1 KB contiguous of the code image (two runs of 256 B per k-half where a gate /
//           up pair shares a 32-channel group);
//   scales  the eight scale bytes of a channel meet in 256 B of LDS and leave as two whole dwords, pad bytes (127) included.
// The grid is E x ceil(N / 32) x ceil(K / 256) workgroups (N is a multiple of 16: a gate / up matrix of H = 48 ends in half a
// workgroup).  Wq == nullptr: load, amax and the status word, nothing is written.
//
// The rounding is INTEGER arithmetic on bit patterns, not a division followed by float comparisons: with s = 2 the quotient of a
// small weight (and a scaled threshold such as 0.25 * 2^-125) is an fp32 subnormal, and what is compared bit for bit against the CPU
// must not depend on the kernel's denormal mode.  |w| = mant * 2^(e - 150) (mant with the hidden bit, e >= 1; a subnormal: e = 1
// without it), so |w| / 2^(s - 127) * 2^25 = mant << (e - s + 2), an exact integer below 2^29 for every shift that matters (a shift
// below 0 is a quotient below 0.25: code 0; a shift above 4 is a quotient of at least 8: saturated), compared against the grid's
// midpoints times 2^25.  No floating-point instruction touches a weight after the widen, which is exact.
//
// Byte model: the parameter read once, the images written once -- E * N * K * (sizeof(T) + 1 / 2) + E * N * ceil(K / 128) * 4 bytes.
// LDS: 33 KB (k-major) / 36 KB (n-major) per workgroup, four workgroups per CU.  No scratch.
#include "common.h"

#define QW4_THREADS 256
#define QW4_CH 32           // source channels per workgroup
#define QW4_KC 256          // k per workgroup: four code tiles of 64 k, two scale dwords of 128 k
// LDS bank arithmetic (64 banks of 4 bytes; a 16-byte access is served 16 lanes at a time, a 4-byte access 64 lanes at a time; in units
// of 16-byte slots a 16-lane access is free of conflicts when its 16 slots differ mod 16):
//   tile[channel][k], QW4_LD_K = 260 words = 65 slots (k-major source).  Reads: 16 lanes are 16 channels at one k, slots 65 c + const =
//     c + const mod 16: all differ.  Writes, fp32 source: 16 lanes write 16 consecutive slots of one row.  Writes, 16-bit source: a lane
//     holds 8 k = two slots, 16 lanes span 32 slots of one row; lanes 0..7 of every 16 write their even slot first and lanes 8..15 their
//     odd slot first (2 i for i < 8, 2 i + 1 = 1, 3, .. mod 16 for i >= 8), then the other: all differ in both instructions.
//   tile[k][channel], QW4_LD_N = 36 words = 9 slots (n-major source).  Reads (4 bytes): lanes 0..31 are consecutive channels of one k,
//     lanes 32..63 the same channels 8 k further, 8 * 36 = 288 = 32 mod 64 words on: 64 banks, all differ.  Writes, 16-bit source: a row
//     is four lanes of two slots, 16 lanes are four rows; rows k, k + 1, k + 8, k + 9 start at slots 0, 9, 72 = 8, 81 = 1 mod 16, and
//     with the lanes' 0, 2, 4, 6 that is every slot once per instruction -- so the loader walks the rows with bits 1 and 3 of the row
//     index exchanged.  Writes, fp32 source: a row is eight lanes of one slot, 16 lanes are rows k and k + 8 (bits 0 and 3 exchanged):
//     slots 0..7 and 72.. = 8..15.
#define QW4_LD_K (QW4_KC + 4)
#define QW4_LD_N (QW4_CH + 4)
#define QW4_SCALE_ONE 127u

struct Qw4Args {
  const unsigned char *W; int64_t w_stride_e, ldw;    // elements
  unsigned char *Wq; int64_t wq_stride_e;             // bytes; Wq == nullptr: the finiteness check alone
  unsigned char *Ws; int64_t s_stride_e;              // bytes
  int N, K, ngroups, nchunks;                         // ceil(N / 32) and ceil(K / 256): the grid is E * ngroups * nchunks
  int group, group_stride, group_offset;
  int s_lo, s_hi;                                     // the admitted scale bytes of the activations' dtype
  int32_t *status;
};

__device__ __forceinline__ uint32_t qw4_umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

// the scale byte of a block whose amax has the bit pattern `bits` (finite): exponent field - 2, clamped; an all-zero block: 127
__device__ __forceinline__ uint32_t qw4_scale(uint32_t bits, int lo, int hi) {
  const int s = (int)(bits >> 23) - 2;
  return bits == 0u ? QW4_SCALE_ONE : (uint32_t)(s < lo ? lo : (s > hi ? hi : s));
}

// the e2m1 code of the fp32 with bit pattern u under scale byte s (>= 2): round to nearest even on the grid, saturated at 6; a value
// that rounds to zero gets 0x0 whatever its sign.  x = |w| / 2^(s - 127) * 2^25 as an integer (see the header comment)
__device__ __forceinline__ uint32_t qw4_code(uint32_t u, int s) {
  const int ef = (int)((u >> 23) & 0xffu);
  const uint32_t mant = (u & 0x7fffffu) | (ef != 0 ? 0x800000u : 0u);
  const int sh = (ef != 0 ? ef : 1) - s + 2;
  const uint32_t x = sh < 0 ? 0u : mant << (sh > 5 ? 5 : sh);   // (a normal weight shifted by 5 is at least 2^28: above every midpoint)
  const uint32_t idx = (uint32_t)(x > 0x0800000u) + (uint32_t)(x >= 0x1800000u) + (uint32_t)(x > 0x2800000u) + (uint32_t)(x >= 0x3800000u) +
                       (uint32_t)(x > 0x5000000u) + (uint32_t)(x >= 0x7000000u) + (uint32_t)(x > 0xa000000u);
  return idx | (idx != 0u ? (u >> 28) & 8u : 0u);
}

// source channel n -> image channel
__device__ __forceinline__ int qw4_image_channel(const Qw4Args &p, int n) {
  return (n / p.group) * p.group_stride + p.group_offset + n % p.group;
}

template <typename T, bool KMAJOR>
__global__ __launch_bounds__(QW4_THREADS) void quantize_w4_kernel(const Qw4Args p) {
  constexpr int VEC = Vec<T>::N;                         // elements per 16-byte load
  constexpr int NV = QW4_CH * QW4_KC / VEC / QW4_THREADS;   // loads per thread: 4 (16 bits) or 8 (fp32)
  __shared__ __attribute__((aligned(16))) float s_tile[KMAJOR ? QW4_CH * QW4_LD_K : QW4_KC * QW4_LD_N];
  __shared__ __attribute__((aligned(4))) unsigned char s_scale[QW4_CH][8];

  const int tid = (int)threadIdx.x;
  const unsigned per_e = (unsigned)p.ngroups * (unsigned)p.nchunks;
  const int e = (int)(blockIdx.x / per_e);
  const unsigned rem = blockIdx.x % per_e;
  const int n0 = (int)(rem / (unsigned)p.nchunks) * QW4_CH, k0 = (int)(rem % (unsigned)p.nchunks) * QW4_KC;
  const int K = p.K, klen = K - k0 < QW4_KC ? K - k0 : QW4_KC;   // a multiple of 64
  const T *W = reinterpret_cast<const T *>(p.W) + (int64_t)e * p.w_stride_e;

  // ---- load: the tile, once, in the source's order ------------------------------------------------------------------------------------
  vec16 x[NV];
#pragma unroll
  for (int it = 0; it < NV; ++it) {
    const int v = it * QW4_THREADS + tid;
    x[it] = vec16{{0u, 0u, 0u, 0u}};
    if constexpr (KMAJOR) {
      constexpr int RV = QW4_KC / VEC;   // loads per channel row
      const int row = v / RV, kk = (v % RV) * VEC;
      if (kk < klen && n0 + row < p.N) x[it] = *reinterpret_cast<const vec16 *>(W + (int64_t)(n0 + row) * p.ldw + k0 + kk);
    } else {
      constexpr int CV = QW4_CH / VEC;   // loads across the 32 channels
      constexpr int B = VEC == 8 ? 1 : 0;
      const int rr = v / CV, c = (v % CV) * VEC;
      const int sw = ((rr >> B) ^ (rr >> 3)) & 1, kk = rr ^ ((sw << B) | (sw << 3));   // bits B and 3 exchanged
      if (kk < klen && n0 + c < p.N) x[it] = *reinterpret_cast<const vec16 *>(W + (int64_t)(k0 + kk) * p.ldw + n0 + c);
    }
  }
#pragma unroll
  for (int it = 0; it < NV; ++it) {
    const int v = it * QW4_THREADS + tid;
    float f[VEC];
    Vec<T>::unpack(x[it], f);
    int at;
    if constexpr (KMAJOR) {
      constexpr int RV = QW4_KC / VEC;
      at = (v / RV) * QW4_LD_K + (v % RV) * VEC;
    } else {
      constexpr int CV = QW4_CH / VEC;
      constexpr int B = VEC == 8 ? 1 : 0;
      const int rr = v / CV;
      const int sw = ((rr >> B) ^ (rr >> 3)) & 1;
      at = (rr ^ ((sw << B) | (sw << 3))) * QW4_LD_N + (v % CV) * VEC;
    }
    if constexpr (VEC == 4) {
      *reinterpret_cast<float4 *>(&s_tile[at]) = make_float4(f[0], f[1], f[2], f[3]);
    } else {
      const bool odd_first = KMAJOR && ((tid >> 3) & 1) != 0;   // (selects on values, not on an index: the halves stay in registers)
      const int first = odd_first ? 4 : 0;
      *reinterpret_cast<float4 *>(&s_tile[at + first]) =
          make_float4(odd_first ? f[4] : f[0], odd_first ? f[5] : f[1], odd_first ? f[6] : f[2], odd_first ? f[7] : f[3]);
      *reinterpret_cast<float4 *>(&s_tile[at + 4 - first]) =
          make_float4(odd_first ? f[0] : f[4], odd_first ? f[1] : f[5], odd_first ? f[2] : f[6], odd_first ? f[3] : f[7]);
    }
  }
  __syncthreads();

  // ---- turn: this thread's lane chunk of the image: channel, k half, code tile of the chunk -------------------------------------------------
  const int ch = tid & 31, half = (tid >> 5) & 1, t = tid >> 6;
  const int n = n0 + ch;
  const bool live = 64 * t < klen && n < p.N;   // (N is a multiple of 16: an expert's last workgroup may hold 16 channels)
  uint32_t u[32];   // bit patterns of k = 64 t + 16 q + 8 half + j at u[8 q + j]
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int kk = 64 * t + 16 * q + 8 * half;
    if constexpr (KMAJOR) {
      const float4 a = *reinterpret_cast<const float4 *>(&s_tile[ch * QW4_LD_K + kk]);
      const float4 b = *reinterpret_cast<const float4 *>(&s_tile[ch * QW4_LD_K + kk + 4]);
      u[8 * q + 0] = __float_as_uint(a.x); u[8 * q + 1] = __float_as_uint(a.y); u[8 * q + 2] = __float_as_uint(a.z); u[8 * q + 3] = __float_as_uint(a.w);
      u[8 * q + 4] = __float_as_uint(b.x); u[8 * q + 5] = __float_as_uint(b.y); u[8 * q + 6] = __float_as_uint(b.z); u[8 * q + 7] = __float_as_uint(b.w);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) u[8 * q + j] = __float_as_uint(s_tile[(kk + j) * QW4_LD_N + ch]);
    }
  }
  // (a tile past K and a channel past N were loaded as zeros: their threads run along, their blocks get the pad byte and nothing of
  // theirs is stored)
  uint32_t m[2] = {0u, 0u};
#pragma unroll
  for (int i = 0; i < 32; ++i) m[i >> 4] = qw4_umax(m[i >> 4], u[i] & 0x7fffffffu);
  int s[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    m[b] = qw4_umax(m[b], (uint32_t)__shfl_xor((int)m[b], 32, 64));
    s[b] = (int)qw4_scale(m[b] >= 0x7f800000u ? 0x7f7fffffu : m[b], p.s_lo, p.s_hi);
  }
  if (half == 0 && qw4_umax(m[0], m[1]) >= 0x7f800000u) atomicMin(p.status, e * p.N + n);
  if (p.Wq == nullptr) return;   // (uniform over the grid)

  const int c_out = qw4_image_channel(p, n < p.N ? n : 0);
  if (half == 0) {
    s_scale[ch][2 * t] = (unsigned char)s[0];
    s_scale[ch][2 * t + 1] = (unsigned char)s[1];
  }
  if (live) {
    vec16 out;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      uint32_t w = 0u;
#pragma unroll
      for (int j = 0; j < 8; ++j) w |= qw4_code(u[8 * q + j], s[q >> 1]) << (4 * j);
      out.w[q] = w;
    }
    unsigned char *const dst = p.Wq + (int64_t)e * p.wq_stride_e +
                               (((int64_t)(c_out >> 5) * (K / 64) + (k0 / 64 + t)) * 64 + 32 * half + (c_out & 31)) * 16;
    *reinterpret_cast<vec16 *>(dst) = out;
  }
  __syncthreads();
  // ---- scales: one whole dword per channel and 128 k, the bytes past K / 32 blocks are the all-zero blocks' 127 ---------------------------
  if (tid < 2 * QW4_CH && 128 * (tid >> 5) < klen && n < p.N) {
    const int d = tid >> 5;
    const int64_t T128 = (K + 127) / 128;
    unsigned char *const dst = p.Ws + (int64_t)e * p.s_stride_e + (((int64_t)(c_out >> 5) * T128 + (k0 / 128 + d)) * 32 + (c_out & 31)) * 4;
    *reinterpret_cast<uint32_t *>(dst) = *reinterpret_cast<const uint32_t *>(&s_scale[ch][4 * d]);
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static const char *const QW4_NAME = "tutel_amd_quantize_w4";

// the shape's part of the coverage, with its reason (nullptr: covered)
static const char *qw4_shape_refusal(int dtype, int act_dtype, int N, int K, int image_channels, int group, int group_stride, int group_offset) {
  if (!dtype_ok(dtype)) return "the weights must be bf16, fp16 or fp32";
  if (act_dtype != TUTEL_BF16 && act_dtype != TUTEL_F16) return "the activations' dtype must be bf16 or fp16";
  if (K < 64 || K % 64 != 0) return "K must be a multiple of 64";
  if (image_channels < 32 || image_channels % 32 != 0) return "image_channels must be a multiple of 32";
  if (group < 16 || group % 16 != 0) return "group must be a multiple of 16";
  if (N < group || N % group != 0) return "N must be a multiple of group";
  if (group_offset < 0 || (long long)group_offset + group > group_stride) return "a group must fit its stride (group_offset + group <= group_stride)";
  if ((long long)(N / group) * group_stride > image_channels) return "the channel map leaves the image ((N / group) * group_stride <= image_channels)";
  return nullptr;
}

extern "C" int tutel_amd_quantize_w4_supported(int dtype, int act_dtype, int N, int K, int image_channels, int group, int group_stride,
                                               int group_offset) {
  return qw4_shape_refusal(dtype, act_dtype, N, K, image_channels, group, group_stride, group_offset) == nullptr ? 1 : 0;
}

template <typename T> static void qw4_launch(const Qw4Args &a, int w_kmajor, unsigned grid, hipStream_t st) {
  if (w_kmajor) hipLaunchKernelGGL((quantize_w4_kernel<T, true>), dim3(grid), dim3(QW4_THREADS), 0, st, a);
  else hipLaunchKernelGGL((quantize_w4_kernel<T, false>), dim3(grid), dim3(QW4_THREADS), 0, st, a);
}

// Every check stands in front of the first HIP call
extern "C" int tutel_amd_quantize_w4(const void *W, int dtype, int act_dtype, int w_kmajor, int64_t w_stride_e, int ldw, int E, int N, int K,
                                     void *Wq, int64_t wq_stride_e, void *Ws, int64_t s_stride_e, int image_channels, int group,
                                     int group_stride, int group_offset, int32_t *status, tutel_stream_t stream) {
  TUTEL_REQUIRE(E >= 0 && N >= 1 && K >= 1, "%s: bad sizes E=%d N=%d K=%d", QW4_NAME, E, N, K);
  const char *why = qw4_shape_refusal(dtype, act_dtype, N, K, image_channels, group, group_stride, group_offset);
  if (why != nullptr) return tutel_notsup(QW4_NAME, why);
  const long long rows = w_kmajor ? N : K, cols = w_kmajor ? K : N, vec = 16 / dtype_size(dtype);
  const long long t128 = ((long long)K + 127) / 128;
  if (ldw < cols) return tutel_notsup(QW4_NAME, "ldw is smaller than a row of the layout (K for a k-major source, N for an n-major one)");
  if (w_stride_e < (rows - 1) * ldw + cols) return tutel_notsup(QW4_NAME, "w_stride_e is smaller than one expert's matrix");
  if (ldw % vec != 0 || w_stride_e % vec != 0)
    return tutel_notsup(QW4_NAME, "rows of W must stay 16-byte aligned (ldw and w_stride_e multiples of 16 bytes)");
  if (wq_stride_e % 16 != 0) return tutel_notsup(QW4_NAME, "the code images must stay 16-byte aligned (wq_stride_e % 16)");
  if (wq_stride_e < (long long)image_channels * K / 2)
    return tutel_notsup(QW4_NAME, "wq_stride_e is smaller than one expert's code image (image_channels * K / 2 bytes)");
  if (s_stride_e % 4 != 0) return tutel_notsup(QW4_NAME, "the scale images must stay 4-byte aligned (s_stride_e % 4)");
  if (s_stride_e < (long long)image_channels * t128 * 4)
    return tutel_notsup(QW4_NAME, "s_stride_e is smaller than one expert's scale image (image_channels * ceil(K / 128) * 4 bytes)");
  const long long ngroups = (N + QW4_CH - 1) / QW4_CH, nchunks = ((long long)K + QW4_KC - 1) / QW4_KC;
  if ((long long)E * N > 0x7fffffffLL || (long long)E * ngroups * nchunks > 0x7fffffffLL)
    return tutel_notsup(QW4_NAME, "E * N and the workgroup count E * ceil(N / 32) * ceil(K / 256) must stay below 2^31");
  if (E == 0) return 0;
  TUTEL_REQUIRE(W != nullptr && status != nullptr && (Wq == nullptr) == (Ws == nullptr),
                "%s: null pointer (W and status always; Wq and Ws both, or neither for the finiteness check alone)", QW4_NAME);
  if (((uintptr_t)W % 16) != 0 || ((uintptr_t)Wq % 16) != 0) return tutel_notsup(QW4_NAME, "W and Wq must be 16-byte aligned");
  TUTEL_REQUIRE(((uintptr_t)Ws % 4) == 0 && ((uintptr_t)status % 4) == 0, "%s: Ws and status must be 4-byte aligned", QW4_NAME);

  Qw4Args a;
  a.W = (const unsigned char *)W; a.w_stride_e = w_stride_e; a.ldw = ldw;
  a.Wq = (unsigned char *)Wq; a.wq_stride_e = wq_stride_e;
  a.Ws = (unsigned char *)Ws; a.s_stride_e = s_stride_e;
  a.N = N; a.K = K; a.ngroups = (int)ngroups; a.nchunks = (int)nchunks;
  a.group = group; a.group_stride = group_stride; a.group_offset = group_offset;
  a.s_lo = act_dtype == TUTEL_BF16 ? 2 : 114; a.s_hi = act_dtype == TUTEL_BF16 ? 252 : 140;
  a.status = status;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)((long long)E * ngroups * nchunks);
  if (dtype == TUTEL_BF16) qw4_launch<bf16_t>(a, w_kmajor, grid, st);
  else if (dtype == TUTEL_F16) qw4_launch<f16_t>(a, w_kmajor, grid, st);
  else qw4_launch<float>(a, w_kmajor, grid, st);
  TUTEL_CHECK_LAUNCH(QW4_NAME);
  return 0;
}
