// CDNA4 bf16 MFMA GEMM for every operand layout of a linear layer's training
// step:  C[M][N] (bf16) = sum_k A(m, k) B(k, n), fp32 accumulation.
//
//   forward  y  = x  W^T : A = x  [M][K] (K-major), B = W  [N][K] (K-major)
//   dgrad    dx = dy W   : A = dy [M][K] (K-major), B = W  [K][N] (N-major)
//   wgrad    dW = dy^T x : A = dy [K][M] (M-major), B = x  [K][N] (N-major)
//
// hipBLASLt runs the N-major ("NT"/"NN") layouts of the Llama-3-8B step at
// 970-1280 TF/s against ~1590 for the K-major forward GEMMs (profiles/r1_ddp),
// so the backward GEMMs get the same 4-wave BK=64 LDS-DMA schedule as
// gemm_bf16.hip's w4b kernel with an operand-layout template:
//
// * K-major operand: LDS-DMA pieces of 8 rows x 128 B, 16-B chunk c of row r
//   at c ^ ((r>>1)&7), fragments by ds_read_b128 (as w4b).
// * N/M-major operand: the stage is 64 k-rows x 256 columns (512 B per row);
//   a DMA piece is 2 k-rows, rows grouped by 8 with a 128-B pad per group
//   (group stride 4224 B) and chunk c of row k at c ^ 2(k&3).  Fragments are
//   the transposed reads ds_read_b64_tr_b16 (two per 16x16x32 operand), which
//   deliver 8 consecutive k of one column exactly like a ds_read_b128 of a
//   K-major row - so both kinds mix in one MFMA.  The pad puts the two 16-lane
//   groups of each half-wave (rows k and k+8) on disjoint bank halves and the
//   XOR separates the four rows of a group: conflict-free
//   (tests/test_gemm_layouts.py).
// LDS: 2 stages x (A + B) <= 132 KiB, one 4-wave workgroup per CU, 128x128
// AGPR accumulators per wave, one barrier per 64-deep stage.
//
// The kernel templates are in gemm_x2_core.h; this file instantiates what
// ships and holds the entry points.  The A/B records (the persistent
// trickle-store kernel x2t, the B-outer order, the staggered / ablated
// dgrad-SwiGLU epilogues) are in experiments/gemm_layouts_exp.h, included
// only into `make gemm-exp`'s library.
#include <mutex>
#include <map>
#include <algorithm>

#include "gemm_plan.h"
#include "gemm_x2_core.h"
#ifdef MXK_GEMM_EXPERIMENTS
#include "experiments/gemm_layouts_exp.h"
#endif

// C tile of split pair t = ws[2t] + ws[2t + 1]; grid (32, tail tiles), each
// thread 8 consecutive columns of one row (two 8-B stores: ldc % 4 == 0).
__global__ void __launch_bounds__(256)
mxk_gemm_split_fixup(const float* __restrict__ ws, uint16_t* __restrict__ C, int M, int N, int ldc,
                     int q_full) {
  const int t = blockIdx.y;
  int m0, n0;
  mxk::w4b_tile<1>(q_full + t, (M / XBM) * (N / XBM), M / XBM, N / XBM, &m0, &n0);
  const int e = (blockIdx.x * 256 + threadIdx.x) * 8;
  const int r = e / XBM, c = e % XBM;
  const float* p0 = ws + static_cast<size_t>(2 * t) * (XBM * XBM) + e;
  const float* p1 = p0 + XBM * XBM;
  const f32x4_t a0 = *reinterpret_cast<const f32x4_t*>(p0);
  const f32x4_t a1 = *reinterpret_cast<const f32x4_t*>(p0 + 4);
  const f32x4_t b0 = *reinterpret_cast<const f32x4_t*>(p1);
  const f32x4_t b1 = *reinterpret_cast<const f32x4_t*>(p1 + 4);
  uint2 lo, hi;
  lo.x = mxk::pack2bf(a0[0] + b0[0], a0[1] + b0[1]);
  lo.y = mxk::pack2bf(a0[2] + b0[2], a0[3] + b0[3]);
  hi.x = mxk::pack2bf(a1[0] + b1[0], a1[1] + b1[1]);
  hi.y = mxk::pack2bf(a1[2] + b1[2], a1[3] + b1[3]);
  uint16_t* cp = C + static_cast<size_t>(m0 + r) * ldc + n0 + c;
  *reinterpret_cast<uint2*>(cp) = lo;
  *reinterpret_cast<uint2*>(cp + 4) = hi;
}

// ---------------------------------------------------------------------------
// Host side.  gemm_plan.h decides what a call runs; the entry points below
// read the knobs, ask it and carry the plan out.
// ---------------------------------------------------------------------------

// ---- host state shared with gemm_bf16.hip --------------------------------
// Compute units the GEMMs may plan for: every round / split-tail decision
// assumes `cus` workgroups run at once.
// With collectives in flight (the ZeRO-1 reduce-scatter under the backward,
// the parameter all-gather under the forward) RCCL's kernels hold some CUs
// for the whole collective, and a GEMM whose tiles exactly fill the chip then
// runs one extra, nearly empty round.  mxk_gemm_set_reserved_cus(k) (or
// MXK_GEMM_RESERVED_CUS=k) tells the planner that k CUs are taken: rounds and
// the split tail are sized for the CUs that are left.
namespace {
int fix_reserved_cus(int v) { return std::max(0, v); }
mxk::EnvKnob g_reserved_cus{"MXK_GEMM_RESERVED_CUS", 0, fix_reserved_cus};

int hw_cus() {
  static thread_local int dev_cached = -1, cus = 256;
  int dev = 0;
  if (hipGetDevice(&dev) == hipSuccess && dev != dev_cached) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
      cus = n;
    dev_cached = dev;
  }
  return cus;
}

int device_cus() { return std::max(1, hw_cus() - g_reserved_cus.get()); }

int fix_exclusive(int v) { return v ? 1 : 0; }
mxk::EnvKnob g_exclusive{"MXK_GEMM_EXCLUSIVE", 0, fix_exclusive};
std::mutex g_excl_mu;
std::map<std::pair<int, const void*>, size_t> g_excl;
}  // namespace

// exclusive mode (mx_common.h MXK_LAUNCH_GEMM)
size_t mxk_excl_lds(const void* kernel) {
  if (!g_exclusive.get()) return 0;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  std::lock_guard<std::mutex> lk(g_excl_mu);
  auto it = g_excl.find({dev, kernel});
  if (it != g_excl.end()) return it->second;
  hipFuncAttributes fa{};
  int max_lds = 0;
  size_t add = 0;
  if (hipFuncGetAttributes(&fa, kernel) == hipSuccess &&
      hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess &&
      fa.sharedSizeBytes < static_cast<size_t>(max_lds))
    add = static_cast<size_t>(max_lds) - fa.sharedSizeBytes;
  g_excl[{dev, kernel}] = add;
  return add;
}

MXK_API void mxk_gemm_set_exclusive(int on) { g_exclusive.set(on); }
MXK_API int mxk_gemm_exclusive(void) { return g_exclusive.get(); }
MXK_API void mxk_gemm_set_reserved_cus(int n) { g_reserved_cus.set(n); }
MXK_API int mxk_gemm_reserved_cus(void) { return g_reserved_cus.get(); }
MXK_API int mxk_gemm_available_cus(void) { return device_cus(); }

// ---- the layout entry points -----------------------------------------------
namespace {
// MFMA order of the layout kernel's K-tile: 0 A-fragment outer (default), 1
// B-fragment outer.  The B-outer instances are built into the experiments
// library only; gemm_plan.h ignores the knob elsewhere.
int fix_x2_order(int v) { return v == 1 ? 1 : 0; }
mxk::EnvKnob g_x2_order{"MXK_X2_ORDER", 0, fix_x2_order};
// dgrad-SwiGLU epilogue mode, raw (gemm_plan.h gemm_dgrad_swiglu_plan)
mxk::EnvKnob g_swiglu_epi{"MXK_SWIGLU_WIDE", 4, nullptr};
}  // namespace

MXK_API void mxk_gemm_x2_set_order(int v) { g_x2_order.set(v); }
MXK_API void mxk_gemm_swiglu_set_epi(int v) { g_swiglu_epi.set(v); }

// 1 if layout-kernel variant v is in this build (4, x2t: experiments only)
MXK_API int mxk_gemm_bf16_ex_variant_built(int v) { return v >= 0 && v <= (kMxkExperiments ? 4 : 3); }

// gemm_split_plan (gemm_plan.h) for the host tests (tests/test_gemm_plan.py)
MXK_API int mxk_gemm_split_plan(long nwg, int K, int cus, long* q_full) {
  return gemm_split_plan(nwg, K, cus, q_full);
}

// Bytes of fp32 workspace the split tail of an (M, N) output needs at most
// (half a round of tiles, two partial tiles each).
MXK_API long mxk_gemm_bf16_split_workspace(void) { return gemm_split_workspace(hw_cus()); }

MXK_API int mxk_gemm_bf16_tn(const void* A, const void* Bt, void* C, int M, int N, int K,
                             int lda, int ldb, int ldc, hipStream_t stream);

namespace {
// Carries out a GemmExPlan of a layout-kernel family: the whole-tile launch,
// then under a split the K halves of the tail tiles and the fixup.  The tile
// map is over all tiles, not the grid, so the whole-tile launch of a split
// covers tiles [0, q_full).
template <bool AN, bool BN>
void launch_ex(const GemmExPlan& p, hipStream_t stream, const uint16_t* a, const uint16_t* b,
               uint16_t* c, int M, int N, int K, int lda, int ldb, int ldc, float* ws) {
#define MXK_EX(KERNEL, grid, ...) \
  MXK_LAUNCH_GEMM((KERNEL), dim3(grid), dim3(XT), stream, a, b, c, M, N, K, lda, ldb, __VA_ARGS__)
  if (p.family == GEMM_X2T || p.order) {
    // x2t and the B-outer x2: A/B records, planned in the experiments build only
#ifdef MXK_GEMM_EXPERIMENTS
    if (p.grid > 0)
      gemm_x2_exp_launch(AN, BN, p.family == GEMM_X2T, p.hb, p.wide, p.grid, stream, a, b, c, M, N,
                         K, lda, ldb, ldc);
#endif
    if (p.family == GEMM_X2T) return;
  } else if (p.grid > 0 && p.family == GEMM_X) {
    MXK_EX((mxk_gemm_bf16_x_kernel<AN, BN>), p.grid, ldc);
  } else if (p.grid > 0) {
    MXK_WITH_BOOL(HB, p.hb,
                  MXK_WITH_BOOL(W, p.wide,
                                MXK_EX((mxk_gemm_bf16_x2_kernel<AN, BN, W, HB>), p.grid, ldc)));
  }
  if (!p.split) return;
  MXK_WITH_BOOL(HB, p.hb,
                MXK_EX((mxk_gemm_bf16_x2_kernel<AN, BN, 0, HB, true>), 2 * p.tail, ldc, nullptr, ws,
                       p.q_full));
  hipLaunchKernelGGL(mxk_gemm_split_fixup, dim3(XBM * XBM / (256 * 8), p.tail), dim3(256), 0, stream,
                     ws, c, M, N, ldc, p.q_full);
#undef MXK_EX
}

// The three mxk_gemm_bf16_ex* entry points: resolve once (gemm_plan.h
// gemm_ex_plan says which call runs what), then hand off or launch.
int run_ex(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
           int a_kmajor, int b_kmajor, int variant, void* ws, long ws_bytes, int* split,
           hipStream_t stream) {
  if (split) *split = 0;
  const GemmOperands o{M, N, K, lda, ldb, ldc, a_kmajor, b_kmajor,
                       gemm_addr_bits(A), gemm_addr_bits(B), gemm_addr_bits(C)};
  const GemmExPlan p = gemm_ex_plan(o, variant, device_cus(), g_x2_order.get(), kMxkExperiments,
                                    gemm_addr_bits(ws), ws ? ws_bytes : 0);
  if (p.status) return static_cast<int>(hipErrorInvalidValue);
  if (p.family == GEMM_TN) return mxk_gemm_bf16_tn(A, B, C, M, N, K, lda, ldb, ldc, stream);
  MXK_WITH_BOOL(AK, a_kmajor,
                MXK_WITH_BOOL(BK, b_kmajor,
                              (launch_ex<!AK, !BK>(p, stream, bf(A), bf(B), bf(C), M, N, K, lda, ldb,
                                                   ldc, static_cast<float*>(ws)))));
  if (split) *split = p.split;
  MXK_RETURN_LAUNCH_STATUS();
}
}  // namespace

// a_kmajor: A stored [M][K] (1) or [K][M] (0); b_kmajor: B stored [N][K] (1)
// or [K][N] (0).  Row strides lda/ldb/ldc in elements.  Tiles exactly:
// M % 256, N % 256, K % 64; returns hipErrorInvalidValue otherwise (callers
// keep the library GEMM for other shapes).  gemm_plan.h lists the variants.
MXK_API int mxk_gemm_bf16_ex_variant(const void* A, const void* B, void* C, int M, int N, int K,
                                     int lda, int ldb, int ldc, int a_kmajor, int b_kmajor,
                                     int variant, hipStream_t stream) {
  return run_ex(A, B, C, M, N, K, lda, ldb, ldc, a_kmajor, b_kmajor, variant, nullptr, 0, nullptr,
                stream);
}

MXK_API int mxk_gemm_bf16_ex(const void* A, const void* B, void* C, int M, int N, int K, int lda,
                             int ldb, int ldc, int a_kmajor, int b_kmajor, hipStream_t stream) {
  return run_ex(A, B, C, M, N, K, lda, ldb, ldc, a_kmajor, b_kmajor, 1, nullptr, 0, nullptr, stream);
}

// mxk_gemm_bf16_ex (variant 1) with the split tail: when the output's 256^2
// tiles fill q whole rounds of the CUs plus a last round at most half full
// (e.g. 384 tiles on 256 CUs), the tail tiles run as K halves on twice as
// many workgroups (fp32 partials in ws, summed by a fixup kernel) instead of
// leaving half the chip idle for a whole round.  Every operand layout; on
// both-K-major operands the whole tiles of a split then run on x2, not on the
// TN kernel.  Every other case runs mxk_gemm_bf16_ex unchanged.  `ws` holds
// >= ws_bytes (mxk_gemm_bf16_split_workspace()); sets *split to 1 when the
// split path ran.
MXK_API int mxk_gemm_bf16_ex_ws(const void* A, const void* B, void* C, int M, int N, int K, int lda,
                                int ldb, int ldc, int a_kmajor, int b_kmajor, void* ws,
                                long ws_bytes, int* split, hipStream_t stream) {
  return run_ex(A, B, C, M, N, K, lda, ldb, ldc, a_kmajor, b_kmajor, 1, ws, ws_bytes, split, stream);
}

// gemm_ex_plan of a call, for the host tests: out[0..8] = GemmFamily, schedule
// bit, order bit, wide C, grid, tail, q_full, workspace bytes, split flag.
// Every input explicit (knobs, CU count, build); host arithmetic only,
// launches nothing.
MXK_API int mxk_gemm_bf16_ex_plan(int M, int N, int K, int lda, int ldb, int ldc, int a_kmajor,
                                  int b_kmajor, int a_bits, int b_bits, int c_bits, int variant,
                                  int cus, int x2_order, int experiments_built, int ws_bits,
                                  long ws_bytes, long* out) {
  const GemmOperands o{M, N, K, lda, ldb, ldc, a_kmajor, b_kmajor, static_cast<unsigned>(a_bits),
                       static_cast<unsigned>(b_bits), static_cast<unsigned>(c_bits)};
  const GemmExPlan p = gemm_ex_plan(o, variant, cus, x2_order, experiments_built != 0,
                                    static_cast<unsigned>(ws_bits), ws_bytes);
  if (p.status || !out) return static_cast<int>(hipErrorInvalidValue);
  const long f[9] = {p.family, p.hb, p.order, p.wide, p.grid, p.tail, p.q_full, p.ws_bytes, p.split};
  for (int i = 0; i < 9; ++i) out[i] = f[i];
  return 0;
}

namespace {
template <int EPI>
void launch_dgrad_swiglu(int grid, hipStream_t stream, const void* dy, const void* w2, const void* gu,
                         void* dgu, int M, int F, int K, int ld_dy, int ld_w2) {
  MXK_LAUNCH_GEMM((mxk_gemm_bf16_x2_kernel<false, true, EPI>), dim3(grid), dim3(XT), stream, bf(dy),
                  bf(w2), bf(dgu), M, F, K, ld_dy, ld_w2, 2 * F, bf(gu), nullptr, 0, nullptr, 0);
}
}  // namespace

// Down-projection input gradient with the SwiGLU backward fused into the
// epilogue: d(act) = dy W2 (dy [M][K] K-major, W2 [K][F] F-major) never
// reaches memory; dgu [M][2F] = d[g | u] is written from gu [M][2F].
// Tiles exactly (M % 256, F % 256, K % 64); hipErrorInvalidValue otherwise.
// gemm_plan.h gemm_dgrad_swiglu_plan lists the epilogues (MXK_SWIGLU_WIDE).
MXK_API int mxk_gemm_bf16_dgrad_swiglu(const void* dy, const void* w2, const void* gu, void* dgu,
                                       int M, int F, int K, int ld_dy, int ld_w2,
                                       hipStream_t stream) {
  const GemmOperands o{M, F, K, ld_dy, ld_w2, gemm_twice(F), 1, 0,
                       gemm_addr_bits(dy), gemm_addr_bits(w2), gemm_addr_bits(dgu)};
  const auto plan = [&](bool stag_ws_ok) {
    return gemm_dgrad_swiglu_plan(o, gemm_addr_bits(gu), g_swiglu_epi.get(), g_x2_order.get(),
                                  kMxkExperiments, device_cus(), stag_ws_ok);
  };
  GemmDgradSwigluPlan p = plan(true);
  if (p.status) return static_cast<int>(hipErrorInvalidValue);
#define MXK_DGRAD_ARGS p.grid, stream, dy, w2, gu, dgu, M, F, K, ld_dy, ld_w2
#ifdef MXK_GEMM_EXPERIMENTS
  // the A/B records first; a call planned staggered whose workspace cannot be
  // had (it is allocated outside a capture only) runs as mode 4
  if (p.stag && gemm_dgrad_swiglu_exp_launch(p.epi, p.order, 1, p.cx, MXK_DGRAD_ARGS) == 0)
    MXK_RETURN_LAUNCH_STATUS();
  if (p.stag) p = plan(false);
  if (gemm_dgrad_swiglu_exp_launch(p.epi, p.order, 0, 0, MXK_DGRAD_ARGS) == 0)
    MXK_RETURN_LAUNCH_STATUS();
#endif
  if (p.epi == 3) launch_dgrad_swiglu<3>(MXK_DGRAD_ARGS);
  else if (p.epi == 4) launch_dgrad_swiglu<4>(MXK_DGRAD_ARGS);
  else launch_dgrad_swiglu<2>(MXK_DGRAD_ARGS);
#undef MXK_DGRAD_ARGS
  MXK_RETURN_LAUNCH_STATUS();
}

// gemm_dgrad_swiglu_plan of a call, for the host tests: out[0..4] = EPI, order
// bit, STAG, grid, cx.  Every input explicit; launches nothing.
MXK_API int mxk_gemm_bf16_dgrad_swiglu_plan(int M, int F, int K, int ld_dy, int ld_w2, int dy_bits,
                                            int w2_bits, int gu_bits, int dgu_bits, int mode,
                                            int x2_order, int experiments_built, int cus,
                                            int stag_ws_ok, long* out) {
  const GemmOperands o{M, F, K, ld_dy, ld_w2, gemm_twice(F), 1, 0, static_cast<unsigned>(dy_bits),
                       static_cast<unsigned>(w2_bits), static_cast<unsigned>(dgu_bits)};
  const GemmDgradSwigluPlan p =
      gemm_dgrad_swiglu_plan(o, static_cast<unsigned>(gu_bits), mode, x2_order,
                             experiments_built != 0, cus, stag_ws_ok != 0);
  if (p.status || !out) return static_cast<int>(hipErrorInvalidValue);
  const long f[5] = {p.epi, p.order, p.stag, p.grid, p.cx};
  for (int i = 0; i < 5; ++i) out[i] = f[i];
  return 0;
}
