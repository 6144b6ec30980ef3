// The bf16 GEMM plans over the invariant sweep of tests/test_gemm_plan.py and
// over hostile integers, as a host program for the ASan + UBSan build
// (make test-gemm-plan).
#include <climits>
#include <cstdio>
#include <initializer_list>

#include "gemm_plan.h"

namespace {
long n = 0, bad = 0;

void check_ex(const GemmOperands& o, int variant, int cus, int order, bool exp, unsigned ws_bits,
              long ws_bytes) {
  const GemmExPlan p = gemm_ex_plan(o, variant, cus, order, exp, ws_bits, ws_bytes);
  ++n;
  if (p.status) {
    if (p.split || p.tail || p.grid) ++bad;   // nothing launched
    return;
  }
  if (!gemm_ex_ok(o) || variant < 0 || variant > 4) ++bad;
  const long nwg = gemm_tiles(o);
  if (p.grid < 0 || p.grid + 2L * p.tail < 1) ++bad;             // something runs
  if (p.q_full + p.tail != nwg) ++bad;
  if (p.split != (p.tail > 0)) ++bad;
  if (p.split && (p.ws_bytes > ws_bytes || p.ws_bytes > gemm_split_workspace(cus) ||
                  p.family != GEMM_X2 || p.grid != p.q_full || 2 * p.tail > cus))
    ++bad;
  if (!p.split && p.family != GEMM_X2T && p.grid != nwg) ++bad;
  if (p.family == GEMM_X2T &&
      (!exp || p.grid < 1 || p.grid > (cus > 1 ? cus : 1) || p.grid > nwg || !p.wide))
    ++bad;
  if (p.order && !(exp && order && p.family == GEMM_X2)) ++bad;
}

void check_dgrad(const GemmOperands& o, unsigned gu_bits, int mode, int order, bool exp, int cus) {
  for (int ws_ok = 0; ws_ok < 2; ++ws_ok, ++n) {
    const GemmDgradSwigluPlan p = gemm_dgrad_swiglu_plan(o, gu_bits, mode, order, exp, cus, ws_ok);
    if (p.status) continue;
    const long nwg = gemm_tiles(o);
    if (p.epi < 2 || p.epi > 6 || p.grid < 1) ++bad;
    if (!exp && (p.epi > 4 || p.order || p.stag)) ++bad;
    if (p.stag ? !(ws_ok && p.epi == 4 && p.cx > 0 && p.grid == nwg + 8 * p.cx) : p.grid != nwg) ++bad;
    if (p.order && p.epi != 4) ++bad;
    if (p.epi != 2 && (gu_bits % 16 || o.c_bits % 16 || o.K < 2 * GEMM_BK)) ++bad;
    // no g / u prefetch (EPI 4 / 6, STAG) over a gu the 32-bit offset cannot span
    if (static_cast<long>(o.M) * o.ldc * 2 > GEMM_BUF_RANGE - 16 &&
        (p.epi == 4 || p.epi == 6 || p.stag || p.order))
      ++bad;
  }
}
}  // namespace

int main() {
  // layouts x variants x CUs x tile counts x K, with and without a workspace
  for (int lay = 0; lay < 4; ++lay)
    for (int variant = -1; variant <= 5; ++variant)
      for (int cus : {256, 240, 192, 4})
        for (int tm : {1, 2, 3, 6, 8, 16, 17, 24, 56})
          for (int tn : {1, 3, 16, 17})
            for (int K : {64, 512, 960, 1024, 1088, 1152, 4096})
              for (int exp = 0; exp < 2; ++exp)
                for (int narrow = 0; narrow < 2; ++narrow) {
                  const int M = tm * GEMM_TILE, N = tn * GEMM_TILE, ak = lay & 1, bk = lay >> 1;
                  const GemmOperands o{M, N, K, ak ? K : M, bk ? K : N, N + 8 * narrow + 4 * narrow,
                                       ak, bk, 0, 0, 0};
                  for (long ws : {0L, gemm_split_workspace(cus) - 1, gemm_split_workspace(cus)})
                    check_ex(o, variant, cus, exp, exp, 0, ws);
                  check_ex(o, variant, cus, 1, exp, 8, gemm_split_workspace(cus));
                  if (ak && !bk)
                    for (int mode : {0, 3, 4, 5, 6, 8, -1})
                      check_dgrad({M, N, K, K, N, gemm_twice(N), 1, 0, 0, 0, 0}, narrow ? 8 : 0, mode,
                                  exp, exp, cus);
                }
  // dgrad-SwiGLU with gu on both sides of 4 GiB (M * 2F * 2 bytes): every mode, and exactly
  // which side takes the prefetching default
  for (int F : {256, 1024, 8192})
    for (int dm : {-512, -256, 0, 256})
      for (int K : {64, 128, 1024})
        for (int exp = 0; exp < 2; ++exp)
          for (int cus : {256, 240, 4}) {
            const int M = static_cast<int>(GEMM_BUF_RANGE / (4L * F)) + dm;
            const GemmOperands o{M, F, K, K, F, gemm_twice(F), 1, 0, 0, 0, 0};
            for (int mode : {0, 3, 4, 5, 6, 8, -1})
              for (int narrow = 0; narrow < 2; ++narrow)
                check_dgrad(o, narrow ? 8 : 0, mode, exp, exp, cus);
            const GemmDgradSwigluPlan p = gemm_dgrad_swiglu_plan(o, 0, 4, 0, exp, cus, true);
            ++n;
            if (p.status || p.epi != (K < 2 * GEMM_BK ? 2 : dm < 0 ? 4 : 3)) ++bad;
          }
  // hostile integers: every field from {<= 0, odd, INT_MAX and near it}
  const int H[] = {INT_MIN, -256, -1, 0, 1, 64, 256, 1 << 24, INT_MAX - 255, INT_MAX - 63, INT_MAX};
  for (int M : H)
    for (int N : H)
      for (int K : H)
        for (int ld : H)
          for (int cus : {INT_MIN, -1, 0, 1, 256, INT_MAX})
            for (int lay = 0; lay < 4; ++lay) {
              const GemmOperands o{M, N, K, ld, ld, ld, lay & 1, lay >> 1, 0, 0, 0};
              check_ex(o, 1, cus, 1, true, 0, LONG_MAX);
              check_ex(o, 4, cus, 0, true, 0, LONG_MIN);
              check_dgrad({M, N, K, ld, ld, gemm_twice(N), 1, 0, 0, 0, 0}, 0, 8, 1, true, cus);
              const GemmTnPlan t = gemm_tn_plan(o, 52);
              ++n;
              if (!t.status && (t.grid < 1 || t.grid_y < 1)) ++bad;
              long q = -1;
              const int tail = gemm_split_plan(static_cast<long>(M) * N, K, cus, &q);
              if (tail < 0 || q + tail != static_cast<long>(M) * N) ++bad;
              (void)gemm_stagger_plan(static_cast<long>(M) * N, K, cus);
            }
  // tile counts near INT_MAX: 65536 x 32768 tiles = 2^31 is refused, one row less is planned
  for (int tm : {65535, 65536})
    for (int cus : {256, 4}) {
      const int M = tm * GEMM_TILE, N = 32768 * GEMM_TILE;
      const GemmOperands o{M, N, 1024, 1024, 1024, N, 1, 1, 0, 0, 0};
      const GemmExPlan p = gemm_ex_plan(o, 3, cus, 0, false, 0, 0);
      ++n;
      if ((p.status == 0) != (tm == 65535)) ++bad;
      check_ex(o, 1, cus, 0, true, 0, gemm_split_workspace(cus));
      const GemmTnPlan t = gemm_tn_plan(o, 52);
      if ((t.status == 0) != (tm == 65535)) ++bad;
    }
  std::printf("gemm plan sweep: %ld points, %ld bad\n", n, bad);
  return bad != 0;
}
