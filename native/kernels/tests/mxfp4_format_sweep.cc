// Host sweep of mxfp4_format.h, the arithmetic the device quantiser runs:
//   * f32_to_e2m1 over every finite bf16 bit pattern at every block exponent
//     that keeps |x 2^-e| < 8, against a brute-force nearest-value search over
//     the eight magnitudes (ties to the even code, saturation at 6, no -0);
//   * e2m1_to_f32 over the 16 codes;
//   * block_exp at its clamps, for fp32-subnormal amax and for zero, and
//     block_inv_scale over the whole exponent range.
// Built with ASan + UBSan (make test-mxfp4-format).
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "mxfp4_format.h"

namespace {

const double kMag[8] = {0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0};
long g_fail = 0;

void fail(const char* what, double a, double b, long got, long want) {
  if (++g_fail <= 20) std::fprintf(stderr, "FAIL %s: (%a, %g) got %ld want %ld\n", what, a, b, got, want);
}

float bf16_bits_to_f32(uint32_t b) {
  const uint32_t u = b << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

// nearest of the eight magnitudes to min(|v|, 6) in double, ties to the even code
uint32_t brute_e2m1(double v) {
  double a = std::fabs(v);
  if (a > 6.0) a = 6.0;
  int best = 0;
  for (int c = 1; c < 8; ++c) {
    const double d = std::fabs(a - kMag[c]), db = std::fabs(a - kMag[best]);
    if (d < db || (d == db && (c & 1) == 0)) best = c;
  }
  return best ? static_cast<uint32_t>(best) | (std::signbit(v) ? 8u : 0u) : 0u;
}

int floor_log2(float amax) {   // amax > 0, finite
  int ex;
  std::frexp(static_cast<double>(amax), &ex);   // amax = m 2^ex, m in [0.5, 1)
  return ex - 1;
}

int want_block_exp(float amax) {
  if (amax == 0.f) return 0;
  const int e = floor_log2(amax) - 2;
  return e < -127 ? -127 : (e > 127 ? 127 : e);
}

void check_block_exp(float amax) {
  const int got = mxfp4::block_exp(amax), want = want_block_exp(amax);
  if (got != want) fail("block_exp", amax, 0, got, want);
}

}  // namespace

int main() {
  // ---- decode ----------------------------------------------------------------
  for (uint32_t c = 0; c < 16; ++c) {
    const float got = mxfp4::e2m1_to_f32(c);
    const float want = static_cast<float>((c & 8) ? -kMag[c & 7] : kMag[c & 7]);
    if (got != want || std::signbit(got) != ((c & 8) != 0)) fail("e2m1_to_f32", c, 0, 0, 0);
  }

  // ---- block exponent and inverse scale --------------------------------------
  check_block_exp(0.f);
  if (mxfp4::block_exp(0.f) != 0) fail("block_exp(0)", 0, 0, mxfp4::block_exp(0.f), 0);
  for (int k = -149; k <= 127; ++k) {
    const float p = std::ldexp(1.f, k);   // fp32 subnormal below k = -126
    check_block_exp(p);
    check_block_exp(std::nextafterf(p, 0.f) > 0.f ? std::nextafterf(p, 0.f) : p);
    check_block_exp(std::nextafterf(p, FLT_MAX));
    if (k < 127) check_block_exp(p * 1.75f);
  }
  check_block_exp(FLT_MAX);
  if (mxfp4::block_exp(FLT_MAX) != 125) fail("block_exp(FLT_MAX)", FLT_MAX, 0, mxfp4::block_exp(FLT_MAX), 125);
  if (mxfp4::block_exp(std::ldexp(1.f, -133)) != -127) fail("block_exp(2^-133)", 0, 0, 0, -127);
  if (mxfp4::block_exp(std::ldexp(1.f, -125)) != -127) fail("block_exp(2^-125)", 0, 0, 0, -127);
  if (mxfp4::block_exp(std::ldexp(1.f, -124)) != -126) fail("block_exp(2^-124)", 0, 0, 0, -126);
  if (mxfp4::block_exp(std::ldexp(1.f, 127)) != 125) fail("block_exp(2^127)", 0, 0, 0, 125);
  for (int e = -127; e <= 125; ++e)
    if (mxfp4::block_inv_scale(e) != std::ldexp(1.f, -e)) fail("block_inv_scale", e, 0, 0, 0);

  // ---- conversion: every finite bf16 at every admissible block exponent ------
  long checked = 0;
  for (uint32_t b = 0; b < 0x10000u; ++b) {
    if (((b >> 7) & 0xFFu) == 0xFFu) continue;   // Inf / NaN
    const float x = bf16_bits_to_f32(b);
    for (int e = -127; e <= 125; ++e) {
      const double exact = std::ldexp(static_cast<double>(x), -e);
      if (!(std::fabs(exact) < 8.0)) continue;
      // what the quantiser does: fp32 product, explicit saturation, convert
      float v = x * mxfp4::block_inv_scale(e);
      v = std::fmin(std::fmax(v, -mxfp4::kMax), mxfp4::kMax);
      const uint32_t got = mxfp4::f32_to_e2m1(v), want = brute_e2m1(exact);
      if (got != want) fail("f32_to_e2m1", x, e, got, want);
      ++checked;
    }
  }
  if (checked < 1000000) fail("sweep size", 0, 0, checked, 1000000);
  if (g_fail) {
    std::fprintf(stderr, "mxfp4_format_sweep: %ld failure(s)\n", g_fail);
    return 1;
  }
  std::printf("mxfp4_format_sweep: %ld conversions, all equal to the brute-force search\n", checked);
  return 0;
}
