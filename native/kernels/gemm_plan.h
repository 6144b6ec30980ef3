// Which bf16 GEMM kernel takes which call: the argument gate, written once,
// and the plans of the entry points of gemm_bf16.hip and
// gemm_bf16_layouts.hip.  Plain C++17 with no HIP call, so the kernel library
// and the stand-alone host program (native/kernels/tests/gemm_plan_sweep.cc)
// share it.  Environment knobs and the device's CU count are inputs: the entry
// points read them and pass them in.  A plan says what is launched, with which
// template constants and grid; the launchers only carry it out.
#pragma once
#include <climits>
#include <cstdint>

namespace {
constexpr int GEMM_TILE = 256;   // output tile, M and N
constexpr int GEMM_BK = 64;      // K per stage
// a buffer resource (LDS-DMA loads) addresses 32-bit byte offsets
constexpr long GEMM_BUF_RANGE = 1L << 32;

// C[M][N] = A . B in bf16.  a_kmajor: A stored [M][K] (else [K][M]); b_kmajor:
// B stored [N][K] (else [K][N]); row strides in elements; *_bits: the low
// address bits of the operand (gemm_addr_bits)
struct GemmOperands {
  int M, N, K, lda, ldb, ldc;
  int a_kmajor, b_kmajor;
  unsigned a_bits, b_bits, c_bits;
};
inline unsigned gemm_addr_bits(const void* p) {
  return static_cast<unsigned>(reinterpret_cast<uintptr_t>(p) & 15);
}
// 2 n (the [g | u] width of the SwiGLU GEMMs), or -1 where it leaves an int: no gate takes it
inline int gemm_twice(int n) { return n >= 0 && n <= INT_MAX / 2 ? 2 * n : -1; }

// whole 256 x 256 x 64 tiles, 16-B LDS-DMA rows of A and B, 8-B stores of C
inline bool gemm_tiles_ok(const GemmOperands& o) {
  return o.M % GEMM_TILE == 0 && o.N % GEMM_TILE == 0 && o.K % GEMM_BK == 0 && o.lda % 8 == 0 &&
         o.ldb % 8 == 0 && o.ldc % 4 == 0 && o.a_bits % 16 == 0 && o.b_bits % 16 == 0 &&
         o.c_bits % 8 == 0;
}
// ... and what the layout kernels add: the strides cover the rows, and an
// N/M-major panel (K rows of ld elements) stays inside one buffer resource
inline bool gemm_ex_ok(const GemmOperands& o) {
  const auto fits = [&](long ld) { return o.K * ld < GEMM_BUF_RANGE / 2; };   // 2 B per element
  return o.M > 0 && o.N > 0 && o.K > 0 && gemm_tiles_ok(o) &&
         (o.a_kmajor ? o.lda >= o.K : o.lda >= o.M) && (o.b_kmajor ? o.ldb >= o.K : o.ldb >= o.N) &&
         o.ldc >= o.N && (o.a_kmajor || fits(o.lda)) && (o.b_kmajor || fits(o.ldb));
}
// C takes 16-B stores (every epilogue but the 8-B ones)
inline bool gemm_wide_c(const GemmOperands& o) { return o.ldc % 8 == 0 && o.c_bits % 16 == 0; }
// output tiles; a grid is an int, so a plan refuses more than INT_MAX
inline long gemm_tiles(const GemmOperands& o) {
  return static_cast<long>(o.M / GEMM_TILE) * (o.N / GEMM_TILE);
}

// ---------------------------------------------------------------------------
// Split tail: nwg output tiles over `cus` CUs and depth K.  When the last
// round is at most half full, its tiles run as two K halves each on twice as
// many workgroups.  Returns the tail tiles (0: no split) and sets *q_full to
// the tiles that run whole.
inline int gemm_split_plan(long nwg, int K, int cus, long* q_full) {
  const int tail = nwg > 0 && cus > 0 ? static_cast<int>(nwg % cus) : 0;
  const bool want = tail > 0 && 2 * static_cast<long>(tail) <= cus && K % (2 * GEMM_BK) == 0 &&
                    K >= 16 * GEMM_BK;
  if (q_full) *q_full = want ? nwg - tail : nwg;
  return want ? tail : 0;
}
// fp32 partials of `tail` split tiles, two [256][256] halves each
inline long gemm_split_bytes(long tail) { return 2 * tail * GEMM_TILE * GEMM_TILE * 4; }
// what a caller allocates: half a round of the whole chip (any reservation fits)
inline long gemm_split_workspace(int hw_cus) { return gemm_split_bytes(hw_cus / 2); }

// Staggered rounds (TN schedule 54): split tiles per XCD (half the XCD's CUs),
// or 0 when it does not apply - T % 8, fewer than two whole rounds, or K
// halves shorter than two K-tiles / not whole K-tiles.
inline int gemm_stagger_plan(long T, int K, int cus) {
  if (T <= 0 || T % 8 || cus < 16 || K % (2 * GEMM_BK) || K < 4 * GEMM_BK) return 0;
  const long tx = T / 8;
  const int cx = cus / 8;
  const int sx = cx / 2;
  if (sx <= 0 || tx < 2 * cx) return 0;
  return sx;
}

// ---------------------------------------------------------------------------
// mxk_gemm_bf16_ex / _ex_variant / _ex_ws.  variant:
//   1 (default) both K-major -> the validator's TN entry (gemm_bf16.hip);
//     both N/M-major (weight gradients) -> x2 at hipBLASLt's positions
//     (+2-10 % on the Llama-3-8B wgrad shapes); mixed (dgrad) -> x2
//   2 x2 at hipBLASLt's positions, 3 x2, 0 the one-barrier x kernel
//     (2, 3 and 0 run every layout on the layout kernel, for A/B)
//   4 x2t (experiments build: persistent, trickled C stores; hipBLASLt
//     positions when a_kmajor == b_kmajor); as 1 in a production build, when
//     K < 18 * 64 or when C does not take 16-B stores
// Routes that surprise, kept as they are until a measurement decides on them:
//  * A split tail (ws given, variant 1) on both-K-major operands runs its
//    WHOLE tiles on x2, not on the TN kernel the same call without a tail
//    hands off to.
//  * Variant 4 that does not reach x2t resolves as 1, the TN hand-off
//    included.
//  * The B-outer order bit (MXK_X2_ORDER=1, experiments build) reaches the
//    whole-tile x2 launch only: the x kernel, x2t and the K halves of a split
//    tail have no such instance.
enum GemmFamily : int {
  GEMM_TN,    // hand-off to mxk_gemm_bf16_tn (gemm_tn_plan resolves it)
  GEMM_X,     // mxk_gemm_bf16_x_kernel<AN, BN>
  GEMM_X2,    // mxk_gemm_bf16_x2_kernel<AN, BN, wide, hb | 2 order>
  GEMM_X2T,   // mxk_gemm_bf16_x2t_kernel<AN, BN, hb>
};
struct GemmExPlan {
  int status;      // 0, or 1: arguments no kernel takes, nothing launched
  GemmFamily family;
  int hb;          // schedule bit: hipBLASLt's instruction positions
  int order;       // order bit: B-fragment outer MFMA loop
  int wide;        // 16-B C stores
  int grid;        // workgroups of the whole-tile launch; q_full under a split, 0: none
  int tail;        // split: tiles run as K halves (grid 2 tail, then the fixup)
  int q_full;      // split: tiles run whole
  long ws_bytes;   // split: workspace the partials take
  int split;       // the split out-flag
};

// ws_bits / ws_bytes: the low address bits and size of the caller's split
// workspace, 0 bytes for none (a null pointer, or an entry point without one)
inline GemmExPlan gemm_ex_plan(const GemmOperands& o, int variant, int cus, int x2_order,
                               bool experiments_built, unsigned ws_bits, long ws_bytes) {
  GemmExPlan p{1, GEMM_TN, 0, 0, 0, 0, 0, 0, 0, 0};
  if (!gemm_ex_ok(o) || variant < 0 || variant > 4 || gemm_tiles(o) > INT_MAX) return p;
  if (cus < 1) cus = 1;   // as the entry points' probe: never an empty grid
  const int nwg = static_cast<int>(gemm_tiles(o));
  const bool both_k = o.a_kmajor && o.b_kmajor, both_n = !o.a_kmajor && !o.b_kmajor;
  p.status = 0;
  p.wide = gemm_wide_c(o);
  p.grid = p.q_full = nwg;
  const int tail = variant == 1 ? gemm_split_plan(nwg, o.K, cus, nullptr) : 0;
  if (tail > 0 && ws_bytes >= gemm_split_bytes(tail) && ws_bits % 16 == 0) {
    p.family = GEMM_X2;
    p.hb = both_n;
    p.order = experiments_built && x2_order;
    p.tail = tail;
    p.grid = p.q_full = nwg - tail;
    p.ws_bytes = gemm_split_bytes(tail);
    p.split = 1;
    return p;
  }
  if (variant == 4 && experiments_built && o.K >= 18 * GEMM_BK && p.wide) {
    p.family = GEMM_X2T;
    p.hb = o.a_kmajor == o.b_kmajor;
    p.grid = nwg < cus ? nwg : cus;   // one workgroup per CU at most
    return p;
  }
  if (variant == 4) variant = 1;
  if (variant == 1 && both_k) return p;   // GEMM_TN
  p.family = variant == 0 ? GEMM_X : GEMM_X2;
  p.hb = variant == 2 || (variant == 1 && both_n);
  p.order = p.family == GEMM_X2 && experiments_built && x2_order;
  return p;
}

// ---------------------------------------------------------------------------
// mxk_gemm_bf16_tn: the 256-tile kernel at schedule `variant` (the resolved
// default, MXK_TN_VARIANT, or the 8-B-store schedule 1 for a narrow C), or
// the bounds-checked 64 x 64 kernel for everything that does not tile.
constexpr int GEMM_TN_NARROW_C = 1;
struct GemmTnPlan {
  int status;    // 0, or 1: nothing launched
  int generic;   // mxk_gemm_bf16_tn_generic on grid (grid, grid_y)
  int variant;   // schedule of the 256-tile kernel
  int grid, grid_y;
};
inline GemmTnPlan gemm_tn_plan(const GemmOperands& o, int default_variant) {
  GemmTnPlan p{1, 0, 0, 0, 1};
  if (o.M <= 0 || o.N <= 0 || o.K <= 0) return p;
  if (!gemm_tiles_ok(o)) {
    p = {0, 1, -1, static_cast<int>((o.N + 63L) / 64), static_cast<int>((o.M + 63L) / 64)};
    return p;
  }
  if (gemm_tiles(o) > INT_MAX) return p;
  p = {0, 0, gemm_wide_c(o) ? default_variant : GEMM_TN_NARROW_C, static_cast<int>(gemm_tiles(o)), 1};
  return p;
}

// ---------------------------------------------------------------------------
// mxk_gemm_bf16_dgrad_swiglu: d(act) = dy W2 with the SwiGLU backward in the
// epilogue (A = dy K-major, B = W2 F-major, C = dgu [M][2F], aux = gu).
// mode (MXK_SWIGLU_WIDE): 4 (default) EPI 4, LDS-staged whole lines with pass
// 0's g / u prefetched during the last K-tiles; 3 EPI 3, permlane pairs; 0 the
// 8-B form, EPI 2; and in the experiments build 5 EPI 5 (4 without the
// prefetch), 6 EPI 6 (4 without the SwiGLU math, timing only), 8 EPI 4
// staggered by XCD group (STAG) where it fits.  A production build runs
// EPI 4 for 5 / 6 / 8, as for any other non-zero mode.  gu or dgu not 16-B
// aligned, or K < 2 K-tiles, gives EPI 2 whatever the mode.
// The g / u prefetch (EPI 4, EPI 6 and STAG) addresses gu through one buffer
// resource based at gu's first row, with a 32-bit byte offset over the whole
// [M][2F] matrix: past 4 GiB the offset wraps and pass 0 would read g / u of
// rows 2^32 / (4F) further up.  So a gu of more than GEMM_BUF_RANGE - 16 bytes
// (the resource's num_records, 0xFFFFFFF0) runs EPI 3 unstaggered wherever a
// prefetching plan would have been taken: the same arithmetic through 64-bit
// pointers (EPI 2 / 3 / 5 never prefetch and are left alone).
// A route that surprises, kept as it is: in the experiments build the B-outer
// order (MXK_X2_ORDER=1) exists for EPI 4 only and wins over the mode, so mode
// 3 (and any other but 0 / 5 / 6) with order 1 runs EPI 4 B-outer, not EPI 3.
struct GemmDgradSwigluPlan {
  int status;   // 0, or 1: nothing launched
  int epi;      // 2 / 3 / 4 / 5 / 6
  int order;    // B-fragment outer MFMA loop (EPI 4 only)
  int stag;     // rounds staggered by XCD group
  int grid;     // tiles, + 8 cx when staggered
  int cx;       // STAG: CUs per XCD the stagger plans for
};
// o: gemm_ex_ok's view of the call, {M, F, K, ld_dy, ld_w2, gemm_twice(F), 1,
// 0, bits of dy / w2 / dgu}; stag_ws_ok: the staggered form's workspace is there
inline GemmDgradSwigluPlan gemm_dgrad_swiglu_plan(const GemmOperands& o, unsigned gu_bits, int mode,
                                                  int x2_order, bool experiments_built, int cus,
                                                  bool stag_ws_ok) {
  GemmDgradSwigluPlan p{1, 2, 0, 0, 0, 0};
  if (!gemm_ex_ok(o) || gu_bits % 8 != 0 || gemm_tiles(o) > INT_MAX) return p;
  const int nwg = static_cast<int>(gemm_tiles(o));
  p.status = 0;
  p.grid = nwg;
  const bool wide = mode != 0 && gu_bits % 16 == 0 && o.c_bits % 16 == 0 && o.K >= 2 * GEMM_BK;
  if (!wide) return p;
  // bytes of gu [M][2F]: the prefetch's resource covers GEMM_BUF_RANGE - 16
  const bool gu_fits = static_cast<long>(o.M) * o.ldc * 2 <= GEMM_BUF_RANGE - 16;
  p.epi = 4;
  if (!gu_fits) {
    p.epi = experiments_built && mode == 5 ? 5 : 3;   // 5 does not prefetch
    return p;
  }
  if (experiments_built) {
    const int cx = cus / 8;
    if (mode == 8 && nwg % 8 == 0 && cx > 0 && nwg / 8 >= 2 * cx && o.K % (2 * GEMM_BK) == 0 &&
        stag_ws_ok) {
      p.stag = 1;
      p.cx = cx;
      p.grid = nwg + 8 * cx;
      return p;
    }
    if (mode == 5 || mode == 6) p.epi = mode;
    else if (x2_order) p.order = 1;
  }
  if (mode == 3 && !p.order) p.epi = 3;
  return p;
}
}  // namespace
