// The element formats of the block-scaled quantiser kernels (mx_quantize.h,
// mx_swiglu_quantize.h): E4m3 (MXFP8), E2m1 (MXFP4, round to nearest even) and
// E2m1Sr (MXFP4, stochastic rounding; quantize_mxfp4_sr.hip has the
// definition).  They stay in an unnamed namespace, as they were in
// gemm_mxfp8.hip, gemm_mxfp4.hip and quantize_mxfp4_sr.hip, so every kernel
// instantiated on them keeps its symbol and its instruction stream
// (profiles/mx_swiglu/isa_diff.txt).
#pragma once
#include "mx_quantize.h"
#include "mx_philox.h"
#include "mxfp4_format.h"

namespace {

struct E4m3 {
  static constexpr int kBits = 8;
  static constexpr float kMax = 448.f;

  // floor(log2(amax)) - 8 clamped to [-127, 127]; 0 for amax == 0
  __device__ static int block_exp(float amax) {
    uint32_t u;
    __builtin_memcpy(&u, &amax, 4);
    if (u == 0) return 0;
    const int e = static_cast<int>(u >> 23) - 127 - 8;   // an fp32 subnormal lands below -127
    return e < -127 ? -127 : e;                           // bf16 input: e <= 119
  }

  __device__ static float inv_scale(int e) {   // 2^-e
    return __uint_as_float(static_cast<uint32_t>(127 - e) << 23);
  }

  // RNE of a finite fp32 with |v| <= 448 to an e4m3fn byte.
  __device__ static uint32_t convert(float v) {
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    const uint32_t sign = (u >> 24) & 0x80u;
    u &= 0x7FFFFFFFu;
    uint32_t r;
    if (u >= 0x3C800000u) {                 // >= 2^-6: a normal e4m3
      u += 0x7FFFFu + ((u >> 20) & 1u);     // round to 3 mantissa bits, ties to even
      r = (u >> 20) - (120u << 3);          // rebias 127 -> 7
    } else {                                // subnormal: units of 2^-9
      float a;
      __builtin_memcpy(&a, &u, 4);
      a += 16384.0f;                        // 2^14: the sum's last bit is 2^-9
      uint32_t b;
      __builtin_memcpy(&b, &a, 4);
      r = b - 0x46800000u;
    }
    return r | sign;
  }
};

// one packed dword per lane
struct E2m1 {
  static constexpr int kBits = 4;
  static constexpr float kMax = mxfp4::kMax;
  __device__ static int block_exp(float amax) { return mxfp4::block_exp(amax); }
  __device__ static float inv_scale(int e) { return mxfp4::block_inv_scale(e); }
  __device__ static uint32_t convert(float v) { return mxfp4::f32_to_e2m1(v); }
};

struct E2m1Sr {
  static constexpr int kBits = 4;   // no kMax: the block exponent does not clip
  __device__ static int block_exp(float amax) { return mxfp4::block_exp_noclip(amax); }
  __device__ static float inv_scale(int e) { return mxfp4::block_inv_scale(e); }
  __device__ static void random(const mxk::mx::SrLane& l, uint32_t (&r)[4]) {
    philox::philox4x32_10(l.g, l.i, 0u, 0u, static_cast<uint32_t>(l.seed),
                          static_cast<uint32_t>(l.seed >> 32), r);
  }
  __device__ static uint32_t convert(float v, uint32_t u16) { return mxfp4::f32_to_e2m1_sr(v, u16); }
};

}  // namespace
