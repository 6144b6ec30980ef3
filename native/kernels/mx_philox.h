// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3",
// SC'11): the counter-based generator behind the stochastic rounding of the
// MXFP4 gradient quantisers (quantize_mxfp4_sr.hip), shared with the host sweep
// (tests/mxfp4_sr_sweep.cc).  Stateless: a (counter, key) pair always gives the
// same four words, so there is no state buffer and no launch-order dependence.
// mxk8s/ops/_philox.py is the same function in numpy.
//
// Known answers (the Random123 test vectors):
//   ctr 0 0 0 0, key 0 0                      6627e8d5 e169c58d bc57ac4c 9b00dbd8
//   ctr and key all ffffffff                  408f276d 41c83b0e a20bc7c6 6d5451fd
//   ctr 243f6a88 85a308d3 13198a2e 03707344,
//   key a4093822 299f31d0                     d16cfe09 94fdcceb 5001e420 24126ea1
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MXPHILOX_HD __host__ __device__
#else
#define MXPHILOX_HD
#endif

namespace philox {

constexpr uint32_t kMul0 = 0xD2511F53u, kMul1 = 0xCD9E8D57u;     // multipliers
constexpr uint32_t kWeyl0 = 0x9E3779B9u, kWeyl1 = 0xBB67AE85u;   // key increments

// out = Philox4x32-10(counter c0..c3, key k0 k1).  The 32 x 32 -> 64 products
// become one v_mul_hi_u32 and one v_mul_lo_u32 each on the device; a
// wave-uniform key stays in scalar registers with its ten increments.
MXPHILOX_HD inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                      uint32_t k1, uint32_t (&out)[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = static_cast<uint64_t>(kMul0) * c0;
    const uint64_t p1 = static_cast<uint64_t>(kMul1) * c2;
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    c1 = static_cast<uint32_t>(p1);
    c3 = static_cast<uint32_t>(p0);
    c0 = n0;
    c2 = n2;
    k0 += kWeyl0;
    k1 += kWeyl1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

}  // namespace philox
