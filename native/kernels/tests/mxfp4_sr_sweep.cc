// Host sweep of the stochastic-rounding arithmetic of the MXFP4 gradient
// quantisers (mx_philox.h, and block_exp_noclip / f32_to_e2m1_sr of
// mxfp4_format.h), the code the device kernels run:
//   * the three known answers of Philox4x32-10;
//   * block_exp_noclip over every finite non-negative bf16: block_exp or one
//     more, the scaled amax at most 6, and above 3 unless the lower clamp binds;
//   * f32_to_e2m1_sr over every bf16 with |v| <= 6: with T = ceil(t) from exact
//     integer arithmetic, u in {0, T - 1, T, 65535} gives the upper neighbour
//     below T and the lower one from T on, so exactly T of the 65536 values
//     round up; values on the grid are fixed; sign and zero rule.
// Built with ASan + UBSan (make test-mxfp4-sr).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "mx_philox.h"
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

void check_philox(const uint32_t (&c)[4], const uint32_t (&k)[2], const uint32_t (&want)[4]) {
  uint32_t got[4];
  philox::philox4x32_10(c[0], c[1], c[2], c[3], k[0], k[1], got);
  for (int i = 0; i < 4; ++i)
    if (got[i] != want[i]) fail("philox4x32_10", c[0], i, got[i], want[i]);
}

// ceil((a - lo) / gap 2^16) for 2^-20 <= a <= 6 with at most 8 significant
// bits: a 2^30 is an integer below 2^33
long ceil_t(double a, int c) {
  const int64_t A = static_cast<int64_t>(std::ldexp(a, 30));
  const int64_t lo = static_cast<int64_t>(std::ldexp(kMag[c], 30));
  const int64_t gap = static_cast<int64_t>(std::ldexp(kMag[c + 1] - kMag[c], 30));
  const int64_t num = (A - lo) * 65536;   // < 2^31 2^16
  return static_cast<long>((num + gap - 1) / gap);
}

}  // namespace

int main() {
  // ---- Philox4x32-10 ---------------------------------------------------------
  check_philox({0, 0, 0, 0}, {0, 0}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u});
  check_philox({0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu},
               {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu});
  check_philox({0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u},
               {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u});

  // ---- non-clipping block exponent -------------------------------------------
  long amaxes = 0;
  if (mxfp4::block_exp_noclip(0.f) != 0) fail("block_exp_noclip(0)", 0, 0, mxfp4::block_exp_noclip(0.f), 0);
  for (uint32_t b = 1; b < 0x7F80u; ++b) {   // every finite positive bf16
    const float amax = bf16_bits_to_f32(b);
    const int e = mxfp4::block_exp(amax), es = mxfp4::block_exp_noclip(amax);
    if (es != e && es != e + 1) fail("block_exp_noclip range", amax, 0, es, e);
    if (es < -127 || es > 127) fail("block_exp_noclip clamp", amax, 0, es, 127);
    const double scaled = std::ldexp(static_cast<double>(amax), -es);
    if (!(scaled <= 6.0)) fail("scaled amax <= 6", amax, scaled, es, e);
    if (!(scaled > 3.0) && es != -127) fail("scaled amax > 3", amax, scaled, es, e);
    // what the quantiser multiplies by is a normal fp32 and the product is exact
    if (static_cast<double>(amax * mxfp4::block_inv_scale(es)) != scaled) fail("inv_scale", amax, scaled, es, e);
    ++amaxes;
  }

  // ---- stochastic conversion ---------------------------------------------------
  long values = 0, on_grid = 0;
  for (uint32_t b = 0; b < 0x10000u; ++b) {
    if (((b >> 7) & 0xFFu) == 0xFFu) continue;   // Inf / NaN
    const float v = bf16_bits_to_f32(b);
    const double a = std::fabs(static_cast<double>(v));
    if (a > 6.0) continue;
    const uint32_t sign = std::signbit(v) ? 8u : 0u;
    int c = 0;
    while (c < 7 && kMag[c + 1] <= a) ++c;       // lower neighbour
    long T;                                      // how many of the 65536 u round up
    if (c == 7 || a == kMag[c]) T = 0;
    else if (a < std::ldexp(1.0, -20)) T = 1;    // 0 < t < 1
    else T = ceil_t(a, c);
    if (T < 0 || T > 65535 + (c < 7)) fail("T range", v, 0, T, 65536);
    const uint32_t lo = c ? static_cast<uint32_t>(c) | sign : 0u;
    const uint32_t hi = c == 7 ? lo : static_cast<uint32_t>(c + 1) | sign;
    if (T == 0) ++on_grid;
    const long us[4] = {0, T - 1, T, 65535};
    for (long u : us) {
      if (u < 0 || u > 65535) continue;
      const uint32_t got = mxfp4::f32_to_e2m1_sr(v, static_cast<uint32_t>(u));
      const uint32_t want = u < T ? hi : lo;
      if (got != want) fail("f32_to_e2m1_sr", v, static_cast<double>(u), got, want);
      if (got == 8u) fail("-0 produced", v, static_cast<double>(u), got, 0);
    }
    // bits above the low 16 of u are ignored
    if (mxfp4::f32_to_e2m1_sr(v, 0xABCD0000u) != mxfp4::f32_to_e2m1_sr(v, 0u)) fail("u16 mask", v, 0, 0, 0);
    ++values;
  }
  if (on_grid != 16) fail("grid values (8 magnitudes, both signs)", 0, 0, on_grid, 16);
  if (amaxes != 0x7F80 - 1 || values < 30000) fail("sweep size", 0, 0, values, 30000);
  if (g_fail) {
    std::fprintf(stderr, "mxfp4_sr_sweep: %ld failure(s)\n", g_fail);
    return 1;
  }
  std::printf("mxfp4_sr_sweep: Philox known answers, %ld block maxima and %ld values, all as defined\n",
              amaxes, values);
  return 0;
}
