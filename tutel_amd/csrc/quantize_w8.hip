// quantize_w8.hip -- the FP8 (OCP e4m3fn) weight quantiser of the W8A16 grouped GEMMs (expert_gemm_w8.hip): reads a parameter as it is
// stored and writes the GEMM's weight image and the per-channel scales directly.  The contract -- which scale and which code a weight
// gets, bit for bit those of tutel_amd/experts/w8.py::quantize_e4m3 on a CPU, and the image's byte layout -- is in include/tutel_amd.h.
//
// One workgroup of 256 threads owns 32 consecutive source channels of one expert over all of K:
//   pass 1  amax: every element read once, 16 bytes per lane.  k-major source: a wave walks 8 channel rows, 1 KB contiguous per load;
//           n-major source: a lane holds 8 (fp32: 4) neighbouring channels of one k, a wave covers 16 (8) k rows of 64 (128) bytes.  The maximum is
//           taken on the BIT PATTERN of |w| as an unsigned integer: it orders the finite values as their magnitudes do, inf and every
//           NaN come out on top (a float maximum would drop the NaN), so one comparison against 0x7f800000 finds a non-finite channel.
//   scale   amax / 448 by a correctly rounded division (an all-zero channel: 1), kept in LDS; a non-finite channel reports
//           e * N + n through one atomicMin on the status word.
//   pass 2  the same elements again (32 x K of them: they hit L2), 128 k at a time through an LDS tile that turns the source's order
//           into the image's: thread (t, kg, channel) divides, clamps and converts 16 values and stores ONE 16-byte lane chunk, so a
//           wave writes 1 KB contiguous of the image (two runs of 256 bytes where a gate / up pair shares a 32-channel group).
// The e4m3 conversion is integer arithmetic (round to nearest even on the bit pattern), not the hardware convert: what is compared
// bit for bit against the CPU must not depend on an instruction's treatment of denormal quotients or of -0.
// Byte model: the parameter read twice (the second time from L2 where a workgroup's 32 x K tile stays resident: 128 KB at K = 2048
// in 16 bits), the image written once.
#include "common.h"

#define QW_THREADS 256
#define QW_CH 32          // source channels per workgroup
#define QW_KC 128         // k per LDS tile: four 32-k groups of the image
#define QW_LD_K (QW_KC + 4)   // tile[channel][k] (k-major source): rows stay 16-byte aligned, 16 lanes of a b128 read hit 16 slots
#define QW_LD_N (QW_CH + 4)   // tile[k][channel] (n-major source)

struct QwArgs {
  const unsigned char *W; int64_t w_stride_e, ldw;    // elements
  unsigned char *Wq; int64_t wq_stride_e;             // bytes; Wq == nullptr: the finiteness check alone
  float *scale; int64_t scale_stride_e;
  int N, K, ngroups;                                  // ngroups = ceil(N / 32) workgroups per expert
  int group, group_stride, group_offset;
  int32_t *status;
};

// fp32 -> e4m3fn code, round to nearest even; |x| >= 480 and NaN give the NaN code (never reached behind the clamp for finite input).
// Below 2^-6 the codes are subnormal, spacing 2^-9: adding 2^14 (whose ulp is 2^-9) rounds to that spacing in one fp32 addition and
// leaves the code in the low mantissa bits.  Above, the rounding is done on the bit pattern: rebias the exponent by 7 - 127, add half
// of the dropped 20 bits minus one, plus the kept part's last bit (ties to even), and drop them.
__device__ __forceinline__ uint32_t qw_e4m3fn(float x) {
  uint32_t u = __float_as_uint(x);
  const uint32_t sign = u & 0x80000000u;
  u ^= sign;
  uint32_t r;
  if (u >= 0x43f00000u) {
    r = 0x7fu;
  } else if (u < 0x3c800000u) {
    r = __float_as_uint(__fadd_rn(__uint_as_float(u), 16384.0f)) - 0x46800000u;
  } else {
    u += 0xc4000000u + 0x7ffffu + ((u >> 20) & 1u);
    r = u >> 20;
  }
  return r | (sign >> 24);
}

// clamp(w / scale, -448, 448) as the reference's: a true division, NaN passes through, -0 keeps its sign
__device__ __forceinline__ uint32_t qw_code(float w, float scale) {
  float q = __fdiv_rn(w, scale);
  q = q < -448.0f ? -448.0f : (q > 448.0f ? 448.0f : q);
  return qw_e4m3fn(q);
}

__device__ __forceinline__ uint32_t qw_umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

// source channel n -> image channel
__device__ __forceinline__ int qw_image_channel(const QwArgs &p, int n) {
  return (n / p.group) * p.group_stride + p.group_offset + n % p.group;
}

template <typename T, bool KMAJOR>
__global__ __launch_bounds__(QW_THREADS) void quantize_w8_kernel(const QwArgs p) {
  constexpr int VEC = Vec<T>::N;          // elements per 16-byte load
  constexpr int CV = QW_CH / VEC;         // loads across the workgroup's 32 channels (n-major source)
  __shared__ uint32_t s_amax[QW_CH];
  __shared__ float s_scale[QW_CH];
  __shared__ __attribute__((aligned(16))) float s_tile[KMAJOR ? QW_CH * QW_LD_K : QW_KC * QW_LD_N];

  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int e = (int)(blockIdx.x / (unsigned)p.ngroups), n0 = (int)(blockIdx.x % (unsigned)p.ngroups) * QW_CH;
  const int N = p.N, K = p.K;
  const T *W = reinterpret_cast<const T *>(p.W) + (int64_t)e * p.w_stride_e;

  // ---- pass 1: amax per channel -----------------------------------------------------------------------------------------------------
  if (tid < QW_CH) s_amax[tid] = 0u;
  __syncthreads();
  if constexpr (KMAJOR) {
    uint32_t m[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) m[r] = 0u;
    for (int kv = lane; kv < K / VEC; kv += 64) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int n = n0 + wave * 8 + r;
        if (n < N) {
          const vec16 v = *reinterpret_cast<const vec16 *>(W + (int64_t)n * p.ldw + (int64_t)kv * VEC);
          float f[VEC];
          Vec<T>::unpack(v, f);
#pragma unroll
          for (int i = 0; i < VEC; ++i) m[r] = qw_umax(m[r], __float_as_uint(f[i]) & 0x7fffffffu);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m[r] = qw_umax(m[r], (uint32_t)__shfl_xor((int)m[r], o, 64));
      if (lane == 0) s_amax[wave * 8 + r] = m[r];
    }
  } else {
    uint32_t m[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) m[i] = 0u;
    const int cv = tid % CV;
    if (n0 + cv * VEC < N) {
      for (int k = tid / CV; k < K; k += QW_THREADS / CV) {
        const vec16 v = *reinterpret_cast<const vec16 *>(W + (int64_t)k * p.ldw + n0 + cv * VEC);
        float f[VEC];
        Vec<T>::unpack(v, f);
#pragma unroll
        for (int i = 0; i < VEC; ++i) m[i] = qw_umax(m[i], __float_as_uint(f[i]) & 0x7fffffffu);
      }
    }
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
#pragma unroll
      for (int o = 32; o >= CV; o >>= 1) m[i] = qw_umax(m[i], (uint32_t)__shfl_xor((int)m[i], o, 64));
      if (lane < CV) atomicMax(&s_amax[cv * VEC + i], m[i]);
    }
  }
  __syncthreads();

  // ---- the scales, and the report of a non-finite channel -----------------------------------------------------------------------------
  if (tid < QW_CH && n0 + tid < N) {
    const int n = n0 + tid;
    const uint32_t bits = s_amax[tid];
    if (bits >= 0x7f800000u) atomicMin(p.status, e * N + n);
    const float s = bits == 0u ? 1.0f : __fdiv_rn(__uint_as_float(bits), 448.0f);
    s_scale[tid] = s;
    if (p.scale != nullptr) p.scale[(int64_t)e * p.scale_stride_e + qw_image_channel(p, n)] = s;
  }
  if (p.Wq == nullptr) return;   // (uniform over the grid)

  // ---- pass 2: the codes, 128 k at a time -----------------------------------------------------------------------------------------------
  const int l31 = tid & 31, kg = (tid >> 5) & 1, tl = tid >> 6;   // this thread's lane chunk of the image: channel, k half, 32-k group of the tile
  const int n_out = n0 + l31;
  const int c_out = n_out < N ? qw_image_channel(p, n_out) : 0;
  unsigned char *const dst = p.Wq + (int64_t)e * p.wq_stride_e + ((int64_t)(c_out >> 5) * (K / 32) * 64 + 32 * kg + (c_out & 31)) * 16;
  for (int k0 = 0; k0 < K; k0 += QW_KC) {
    __syncthreads();   // the tile's readers of the round before (first round: s_scale)
    if constexpr (KMAJOR) {
      constexpr int RV = QW_KC / VEC;   // loads per channel row of the tile
      for (int v = tid; v < QW_CH * RV; v += QW_THREADS) {
        const int row = v / RV, kk = (v % RV) * VEC;
        if (n0 + row < N && k0 + kk < K) {
          const vec16 x = *reinterpret_cast<const vec16 *>(W + (int64_t)(n0 + row) * p.ldw + k0 + kk);
          float f[VEC];
          Vec<T>::unpack(x, f);
#pragma unroll
          for (int i = 0; i < VEC; i += 4)
            *reinterpret_cast<float4 *>(&s_tile[row * QW_LD_K + kk + i]) = make_float4(f[i], f[i + 1], f[i + 2], f[i + 3]);
        }
      }
    } else {
      for (int v = tid; v < QW_KC * CV; v += QW_THREADS) {
        const int kk = v / CV, c = (v % CV) * VEC;
        if (n0 + c < N && k0 + kk < K) {
          const vec16 x = *reinterpret_cast<const vec16 *>(W + (int64_t)(k0 + kk) * p.ldw + n0 + c);
          float f[VEC];
          Vec<T>::unpack(x, f);
#pragma unroll
          for (int i = 0; i < VEC; i += 4)
            *reinterpret_cast<float4 *>(&s_tile[kk * QW_LD_N + c + i]) = make_float4(f[i], f[i + 1], f[i + 2], f[i + 3]);
        }
      }
    }
    __syncthreads();
    if (n_out < N && k0 + 32 * tl < K) {
      const float s = s_scale[l31];
      vec16 out;
#pragma unroll
      for (int h = 0; h < 2; ++h) {   // bytes 8 h + j: k = 32 t + 16 h + 8 kg + j
        const int kk = 32 * tl + 16 * h + 8 * kg;
        float f[8];
        if constexpr (KMAJOR) {
          const float4 a = *reinterpret_cast<const float4 *>(&s_tile[l31 * QW_LD_K + kk]);
          const float4 b = *reinterpret_cast<const float4 *>(&s_tile[l31 * QW_LD_K + kk + 4]);
          f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] = s_tile[(kk + j) * QW_LD_N + l31];
        }
        out.w[2 * h] = qw_code(f[0], s) | (qw_code(f[1], s) << 8) | (qw_code(f[2], s) << 16) | (qw_code(f[3], s) << 24);
        out.w[2 * h + 1] = qw_code(f[4], s) | (qw_code(f[5], s) << 8) | (qw_code(f[6], s) << 16) | (qw_code(f[7], s) << 24);
      }
      *reinterpret_cast<vec16 *>(dst + (int64_t)(k0 / 32 + tl) * 64 * 16) = out;
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
static const char *const QW_NAME = "tutel_amd_quantize_w8";

// the shape's part of the coverage, with its reason (nullptr: covered)
static const char *qw_shape_refusal(int dtype, int N, int K, int image_channels, int group, int group_stride, int group_offset) {
  if (!dtype_ok(dtype)) return "the weights must be bf16, fp16 or fp32";
  if (K < 32 || K % 32 != 0) return "K must be a multiple of 32";
  if (image_channels < 32 || image_channels % 32 != 0) return "image_channels must be a multiple of 32";
  if (group < 16 || group % 16 != 0) return "group must be a multiple of 16";
  if (N < group || N % group != 0) return "N must be a multiple of group";
  if (group_offset < 0 || (long long)group_offset + group > group_stride) return "a group must fit its stride (group_offset + group <= group_stride)";
  if ((long long)(N / group) * group_stride > image_channels) return "the channel map leaves the image ((N / group) * group_stride <= image_channels)";
  return nullptr;
}

extern "C" int tutel_amd_quantize_w8_supported(int dtype, int N, int K, int image_channels, int group, int group_stride, int group_offset) {
  return qw_shape_refusal(dtype, N, K, image_channels, group, group_stride, group_offset) == nullptr ? 1 : 0;
}

template <typename T> static void qw_launch(const QwArgs &a, int w_kmajor, unsigned grid, hipStream_t st) {
  if (w_kmajor) hipLaunchKernelGGL((quantize_w8_kernel<T, true>), dim3(grid), dim3(QW_THREADS), 0, st, a);
  else hipLaunchKernelGGL((quantize_w8_kernel<T, false>), dim3(grid), dim3(QW_THREADS), 0, st, a);
}

// Every check stands in front of the first HIP call
extern "C" int tutel_amd_quantize_w8(const void *W, int dtype, int w_kmajor, int64_t w_stride_e, int ldw, int E, int N, int K, void *Wq,
                                     int64_t wq_stride_e, float *scale, int64_t scale_stride_e, int image_channels, int group,
                                     int group_stride, int group_offset, int32_t *status, tutel_stream_t stream) {
  TUTEL_REQUIRE(E >= 0 && N >= 1 && K >= 1, "%s: bad sizes E=%d N=%d K=%d", QW_NAME, E, N, K);
  const char *why = qw_shape_refusal(dtype, N, K, image_channels, group, group_stride, group_offset);
  if (why != nullptr) return tutel_notsup(QW_NAME, why);
  const long long rows = w_kmajor ? N : K, cols = w_kmajor ? K : N, vec = 16 / dtype_size(dtype);
  if (ldw < cols) return tutel_notsup(QW_NAME, "ldw is smaller than a row of the layout (K for a k-major source, N for an n-major one)");
  if (w_stride_e < (rows - 1) * ldw + cols) return tutel_notsup(QW_NAME, "w_stride_e is smaller than one expert's matrix");
  if (ldw % vec != 0 || w_stride_e % vec != 0)
    return tutel_notsup(QW_NAME, "rows of W must stay 16-byte aligned (ldw and w_stride_e multiples of 16 bytes)");
  if (wq_stride_e % 16 != 0) return tutel_notsup(QW_NAME, "the images must stay 16-byte aligned (wq_stride_e % 16)");
  if (wq_stride_e < (long long)image_channels * K) return tutel_notsup(QW_NAME, "wq_stride_e is smaller than one expert's image (image_channels * K bytes)");
  if (scale_stride_e < image_channels) return tutel_notsup(QW_NAME, "scale_stride_e is smaller than the image's channels");
  const long long ngroups = (N + QW_CH - 1) / QW_CH;
  if ((long long)E * N > 0x7fffffffLL || (long long)E * ngroups > 0x7fffffffLL)
    return tutel_notsup(QW_NAME, "E * N must stay below 2^31");
  if (E == 0) return 0;
  TUTEL_REQUIRE(W != nullptr && status != nullptr && (Wq == nullptr) == (scale == nullptr),
                "%s: null pointer (W and status always; Wq and scale both, or neither for the finiteness check alone)", QW_NAME);
  if (((uintptr_t)W % 16) != 0 || ((uintptr_t)Wq % 16) != 0) return tutel_notsup(QW_NAME, "W and Wq must be 16-byte aligned");
  TUTEL_REQUIRE(((uintptr_t)scale % 4) == 0 && ((uintptr_t)status % 4) == 0, "%s: scale and status must be 4-byte aligned", QW_NAME);

  QwArgs a;
  a.W = (const unsigned char *)W; a.w_stride_e = w_stride_e; a.ldw = ldw;
  a.Wq = (unsigned char *)Wq; a.wq_stride_e = wq_stride_e;
  a.scale = scale; a.scale_stride_e = scale_stride_e;
  a.N = N; a.K = K; a.ngroups = (int)ngroups;
  a.group = group; a.group_stride = group_stride; a.group_offset = group_offset;
  a.status = status;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)((long long)E * ngroups);
  if (dtype == TUTEL_BF16) qw_launch<bf16_t>(a, w_kmajor, grid, st);
  else if (dtype == TUTEL_F16) qw_launch<f16_t>(a, w_kmajor, grid, st);
  else qw_launch<float>(a, w_kmajor, grid, st);
  TUTEL_CHECK_LAUNCH(QW_NAME);
  return 0;
}
