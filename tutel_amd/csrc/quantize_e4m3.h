// quantize_e4m3.h -- the e4m3fn rounding of the quantisers (quantize_w8.hip: weights per channel, quantize_a8.hip: activations per row):
// integer arithmetic on the fp32 bit pattern, so that what is compared bit for bit against experts/w8.py::quantize_e4m3 on a CPU does
// not depend on an instruction's treatment of denormal quotients or of -0.
#pragma once
#include "common.h"

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
