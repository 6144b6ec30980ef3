// MXFP4 (OCP MX, e2m1 elements, one E8M0 scale per 32 K elements): the
// arithmetic of the format, shared by the device quantiser
// (gemm_mxfp4.hip) and the host sweep (tests/mxfp4_format_sweep.cc).
//
//   code       0    1    2    3    4    5    6    7      bit 3: sign
//   magnitude  0   0.5   1   1.5   2    3    4    6
//
// Per block of 32: e = clamp(floor(log2(amax)) - 2, -127, 127) (2 is the emax
// of e2m1), scale byte e + 127 (127 for a zero block), element
// RNE_to_e2m1(clamp(x 2^-e, -6, 6)), ties to the even code.
//
// The stochastic rounding of the gradient quantisers (quantize_mxfp4_sr.hip,
// host sweep tests/mxfp4_sr_sweep.cc) has its own block exponent and element
// conversion below, block_exp_noclip and f32_to_e2m1_sr.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MXFP4_HD __host__ __device__
#else
#define MXFP4_HD
#endif

namespace mxfp4 {

constexpr int kBlock = 32;
constexpr float kMax = 6.0f;

// floor(log2(amax)) - 2 clamped to [-127, 127]; 0 for amax == 0.  amax is a
// finite non-negative fp32, so the result is at most 254 - 127 - 2 = 125 and
// only the lower clamp can bind (an fp32 subnormal has exponent field 0).
MXFP4_HD inline int block_exp(float amax) {
  uint32_t u;
  __builtin_memcpy(&u, &amax, 4);
  if (u == 0) return 0;
  const int e = static_cast<int>(u >> 23) - 127 - 2;
  return e < -127 ? -127 : (e > 127 ? 127 : e);
}

// 2^-e for e in [-127, 125]: always a normal fp32.
MXFP4_HD inline float block_inv_scale(int e) {
  const uint32_t u = static_cast<uint32_t>(127 - e) << 23;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

// RNE of a finite fp32 to an e2m1 nibble, saturating at +-6.  The seven
// thresholds are the midpoints of neighbouring magnitudes; a midpoint goes to
// the even code, so it counts (>=) only where the upper neighbour is even.
// What rounds to zero gives code 0 whatever its sign: -0 (code 8) is never
// produced.
MXFP4_HD inline uint32_t f32_to_e2m1(float v) {
  uint32_t u;
  __builtin_memcpy(&u, &v, 4);
  const uint32_t sign = (u >> 28) & 0x8u;
  u &= 0x7FFFFFFFu;
  float a;
  __builtin_memcpy(&a, &u, 4);
  const uint32_t code = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) +
                        (a >= 3.5f) + (a > 5.0f);
  return code ? code | sign : 0u;
}

// ---- stochastic rounding (the gradient quantisers, quantize_mxfp4_sr.hip) ----
// block_exp leaves scaled block maxima in [4, 8) and what lies above 6 is
// clamped, which shrinks every block whatever the rounding.  The exponent that
// does not clip: one more where amax 2^-e > 6 (exact: a bf16 times a power of
// two), so scaled maxima land in (3, 6] unless the lower clamp binds.
// block_exp is at most 125, so the result stays in [-127, 126], where
// block_inv_scale still gives a normal fp32.
MXFP4_HD inline int block_exp_noclip(float amax) {
  const int e = block_exp(amax);
  return amax * block_inv_scale(e) > kMax ? e + 1 : e;
}

// A finite fp32 with |v| <= 6 to an e2m1 nibble, rounded to one of its two
// neighbours at random: with lo the largest magnitude <= |v| (code c), gap the
// distance to the next one and t = (|v| - lo) / gap 2^16, the upper neighbour
// where u < t for the 16-bit random u.  Every step is exact in fp32 (|v| - lo
// by Sterbenz, the rest powers of two), so exactly ceil(t) of the 65536 values
// of u round up, a value on the grid keeps its code, and FMA contraction
// cannot change a bit.  Sign and zero as f32_to_e2m1.
MXFP4_HD inline uint32_t f32_to_e2m1_sr(float v, uint32_t u16) {
  uint32_t u;
  __builtin_memcpy(&u, &v, 4);
  const uint32_t sign = (u >> 28) & 0x8u;
  u &= 0x7FFFFFFFu;
  float a;
  __builtin_memcpy(&a, &u, 4);
  const uint32_t c = (a >= 0.5f) + (a >= 1.0f) + (a >= 1.5f) + (a >= 2.0f) + (a >= 3.0f) + (a >= 4.0f) +
                     (a >= 6.0f);
  uint32_t code = 7u;
  if (c < 7u) {
    // lo = 0, 0.5, 1, 1.5 | 2, 3 | 4 and 2^16 / gap
    const float lo = c < 4u ? 0.5f * static_cast<float>(c) : (c < 6u ? static_cast<float>(c) - 2.0f : 4.0f);
    const float per_gap = c < 4u ? 131072.0f : (c < 6u ? 65536.0f : 32768.0f);
    const float t = (a - lo) * per_gap;
    code = c + (static_cast<float>(u16 & 0xFFFFu) < t ? 1u : 0u);
  }
  return code ? code | sign : 0u;
}

MXFP4_HD inline float e2m1_to_f32(uint32_t code) {
  const uint32_t m = code & 7u;
  // 0, 0.5 (the subnormal), then (1 + 0.5 man) 2^(exp - 1)
  const uint32_t bits = m < 2 ? (m ? 0x3F000000u : 0u) : (((m >> 1) + 126u) << 23) | ((m & 1u) << 22);
  const uint32_t u = bits | ((code & 8u) << 28);
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

}  // namespace mxfp4
