// Layout bf16 GEMM A/B records, built only into the experiments library
// (`make gemm-exp` -> libmxkernels_exp.so; -DMXK_GEMM_EXPERIMENTS), reached
// from the entry points of gemm_bf16_layouts.hip through gemm_x2_exp_launch
// and gemm_dgrad_swiglu_exp_launch.
//
// A header that gemm_bf16_layouts.hip includes under the flag, not a source
// file of its own: hipcc's code for every layout kernel depends on which other
// instances of the same operand layouts its translation unit holds, so moving
// these records into their own object changes the instruction streams of the
// experiments library (register counts and SGPR spills of x2t included;
// profiles/layout_gemm_ktile/isa_identity.txt).
#pragma once
#include <map>
#include <mutex>

#include "gemm_x2_core.h"

// x2t: persistent x2 with the C store tail trickled into the next tile's
// main loop (gemm_bf16.hip schedule 31, same mechanism): rows 64..127 of
// each wave block leave as a burst after the next tile's prologue DMA, rows
// 0..63 stay in 64 VGPRs and go out one whole-line store per K-tile in the
// next tile's first 16 K-tiles.  Needs K >= 18 * 64 (the launcher falls
// back to x2 below that).
template <int Q, int NB, int SCHED, bool AN, bool BN>
__device__ __forceinline__ void x2_trickle(f32x4_t (&acc)[8][8], bf16x8_t (&f0a)[8],
                                           bf16x8_t (&f0b)[8], bf16x8_t (&f1a)[8],
                                           bf16x8_t (&f1b)[8], char* smem, const XOp<AN>& oa,
                                           const XOp<BN>& ob, int wm, int wn, uint32_t& sa,
                                           uint32_t& sb, uint32_t ka, uint32_t kb, int wave,
                                           const u32x4_t (&buf)[16], uint16_t* tp, size_t tstride) {
  using H = mxk::TrickleStoreT<false>;
  const H h0{{}, buf[Q], tp + Q * tstride};
  const H h1{{}, buf[Q + 1], tp + (Q + 1) * tstride};
  // K-tile 0: the 16 burst stores and its own trickle store are younger than stage 1
  // (pieces through dma16m, as the record was measured: QDMA false)
  x2_ktile_s<SCHED, AN, BN, 0, 1, (Q == 0 ? 17 : 1), H, false>(acc, f0a, f0b, f1a, f1b, smem, oa, ob,
                                                               wm, wn, sa, sb, wave, 0, h0);
  x2_ktile_s<SCHED, AN, BN, 1, 1, 1, H, false>(acc, f0a, f0b, f1a, f1b, smem, oa, ob, wm, wn,
                                               sa + ka, sb + kb, wave, 0, h1);
  sa += 2 * ka;
  sb += 2 * kb;
  if constexpr (Q + 2 < NB)
    x2_trickle<Q + 2, NB, SCHED, AN, BN>(acc, f0a, f0b, f1a, f1b, smem, oa, ob, wm, wn, sa, sb, ka, kb,
                                     wave, buf, tp, tstride);
}

template <bool AN, bool BN, int SCHED, int NB = (AN && BN ? 8 : AN ? 12 : 16)>
__global__ void __launch_bounds__(XT, 1)
mxk_gemm_bf16_x2t_kernel(const uint16_t* __restrict__ A, const uint16_t* __restrict__ B,
                         uint16_t* __restrict__ C, int M, int N, int K, int lda, int ldb, int ldc) {
  constexpr int A_BYTES = XOp<AN>::BYTES;
  constexpr int STAGE = A_BYTES + XOp<BN>::BYTES;
  static_assert(4 * mxk::kStoreLdsWave <= 2 * STAGE, "LDS slice per wave");
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1;
  const int wn = wave & 1;
  const int tiles_m = M / XBM, tiles_n = N / XBM;
  const int ntiles = tiles_m * tiles_n;
  const int ns = K / XBK;                       // >= 18 (launcher)
  const int rr = lane >> 4, cc = (lane & 15) * 8;
  const size_t tstride = static_cast<size_t>(4) * ldc;

  int t = blockIdx.x;
  int m0, n0;
  mxk::w4b_tile<1>(t, ntiles, tiles_m, tiles_n, &m0, &n0);
  XOp<AN> oa;
  XOp<BN> ob;
  auto setup = [&]() {
    oa.init(A, lda, m0, K, lane, wave);
    ob.init(B, ldb, n0, K, lane, wave);
    oa.set_lds(smem, mxk::lds_addr32(smem));
    ob.set_lds(smem, mxk::lds_addr32(smem));
  };
  setup();
  const uint32_t ka = oa.kstep(), kb = ob.kstep();
  auto prologue = [&]() {
#pragma unroll
    for (int p = 0; p < 8; ++p) oa.issue_s(smem, p, 0, wave);
#pragma unroll
    for (int p = 0; p < 8; ++p) ob.issue_s(smem + A_BYTES, p, 0, wave);
#pragma unroll
    for (int p = 0; p < 8; ++p) oa.issue_s(smem + STAGE, p, ka, wave);
#pragma unroll
    for (int p = 0; p < 8; ++p) ob.issue_s(smem + STAGE + A_BYTES, p, kb, wave);
  };
  prologue();
  asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  static_assert(NB % 2 == 0 && NB <= 16, "trickle vectors");
  u32x4_t buf[16];                                    // 0..NB-1 trickled
  uint16_t* tp = C;
  bool trickle = false;
  while (true) {
    f32x4_t acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    bf16x8_t f0a[8], f0b[8], f1a[8], f1b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) f0b[j] = ob.frag(smem + A_BYTES, wn * 8 + j, 0);
#pragma unroll
    for (int i = 0; i < 8; ++i) f0a[i] = oa.frag(smem, wm * 8 + i, 0);
    __builtin_amdgcn_s_waitcnt(0xC07F);

    int s = 0;
    uint32_t sa = 2 * ka, sb = 2 * kb;
    if (trickle) {
      x2_trickle<0, NB, SCHED, AN, BN>(acc, f0a, f0b, f1a, f1b, smem, oa, ob, wm, wn, sa, sb, ka,
                                       kb, wave, buf, tp, tstride);
      s = NB;
    }
    for (; s + 2 <= ns - 2; s += 2) {
      x2_ktile_s<SCHED, AN, BN, 0, 1, 0, mxk::NoHook, false>(acc, f0a, f0b, f1a, f1b, smem, oa, ob, wm,
                                                             wn, sa, sb, wave);
      x2_ktile_s<SCHED, AN, BN, 1, 1, 0, mxk::NoHook, false>(acc, f0a, f0b, f1a, f1b, smem, oa, ob, wm,
                                                             wn, sa + ka, sb + kb, wave);
      sa += 2 * ka;
      sb += 2 * kb;
    }
    if (s < ns - 2) {
      x2_ktile_s<SCHED, AN, BN, 0, 1, 0, mxk::NoHook, false>(acc, f0a, f0b, f1a, f1b, smem, oa, ob, wm,
                                                             wn, sa, sb, wave);
      ++s;
    }
    x2_ktile_s<SCHED, AN, BN, 2, 2>(acc, f0a, f0b, f1a, f1b, smem, oa, ob, wm, wn, 0, 0, wave, s & 1);
    ++s;
    x2_ktile_s<SCHED, AN, BN, 2, 3>(acc, f0a, f0b, f1a, f1b, smem, oa, ob, wm, wn, 0, 0, wave, s & 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    mxk::mfma_drain(acc);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();

    char* lds = smem + wave * mxk::kStoreLdsWave;
    uint16_t* row0 = C + static_cast<size_t>(m0 + wm * 128 + rr) * ldc + n0 + wn * 128 + cc;
    const int tn = t + static_cast<int>(gridDim.x);
    u32x4_t hi[16];
    mxk::stage_half(acc, 0, lane, lds, buf);
    mxk::stage_half(acc, 1, lane, lds, hi);
    if (tn >= ntiles) {
#pragma unroll
      for (int it = 0; it < 16; ++it) {
        *reinterpret_cast<u32x4_t*>(row0 + it * tstride) = buf[it];
        *reinterpret_cast<u32x4_t*>(row0 + (16 + it) * tstride) = hi[it];
      }
      break;
    }
    // vectors beyond NB go out now, ahead of the next prologue (the stage-0
    // wait then covers them, so no count below changes)
#pragma unroll
    for (int it = NB; it < 16; ++it) *reinterpret_cast<u32x4_t*>(row0 + it * tstride) = buf[it];
    tp = row0;
    __builtin_amdgcn_s_barrier();                     // every wave read its slice back
    t = tn;
    mxk::w4b_tile<1>(t, ntiles, tiles_m, tiles_n, &m0, &n0);
    setup();
    prologue();
#pragma unroll
    for (int it = 0; it < 16; ++it) *reinterpret_cast<u32x4_t*>(tp + (16 + it) * tstride) = hi[it];
    asm volatile("s_waitcnt vmcnt(32)" ::: "memory");  // stage 0 (stage 1 + 16 stores in flight)
    __builtin_amdgcn_s_barrier();
    trickle = true;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

namespace {
// Per-(device, stream) uncached workspace of the staggered dgrad-SwiGLU GEMM:
// fp32 partial tiles (256 KiB each) and their flags, zeroed once; each
// consumer resets its flag, so later launches and graph replays start clean.
struct SwigluStagWs {
  float* ws = nullptr;
  int* flags = nullptr;
  int slots = 0;
};
std::mutex g_sstag_mu;
std::map<std::pair<int, hipStream_t>, SwigluStagWs> g_sstag;

const SwigluStagWs* swiglu_stag_ws(hipStream_t stream, int slots) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(g_sstag_mu);
  SwigluStagWs& w = g_sstag[{dev, stream}];
  if (w.slots >= slots) return &w;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone)
    return nullptr;
  if (w.ws) (void)hipFree(w.ws);
  if (w.flags) (void)hipFree(w.flags);
  w = SwigluStagWs{};
  void *ws = nullptr, *fl = nullptr;
  if (hipExtMallocWithFlags(&ws, static_cast<size_t>(slots) * XBM * XBM * 4,
                            hipDeviceMallocUncached) != hipSuccess ||
      hipExtMallocWithFlags(&fl, static_cast<size_t>(slots) * 4, hipDeviceMallocUncached) != hipSuccess ||
      hipMemsetAsync(fl, 0, static_cast<size_t>(slots) * 4, stream) != hipSuccess) {
    if (ws) (void)hipFree(ws);
    if (fl) (void)hipFree(fl);
    return nullptr;
  }
  w.ws = static_cast<float*>(ws);
  w.flags = static_cast<int*>(fl);
  w.slots = slots;
  return &w;
}

// x2t (mixed against x2 on the Llama-3-8B step shapes,
// profiles/r3_pass1/layouts_ab.log), else the B-outer x2 (step-neutral,
// profiles/r4_step/step_ab_set2.txt), at schedule bit hb
template <bool AN, bool BN>
void launch_x2_exp(bool x2t, int hb, int wide, int grid, hipStream_t stream, const uint16_t* a,
                   const uint16_t* b, uint16_t* c, int M, int N, int K, int lda, int ldb, int ldc) {
#define MXK_EX(KERNEL) \
  MXK_LAUNCH_GEMM((KERNEL), dim3(grid), dim3(XT), stream, a, b, c, M, N, K, lda, ldb, ldc)
  if (x2t) MXK_WITH_BOOL(HB, hb, MXK_EX((mxk_gemm_bf16_x2t_kernel<AN, BN, HB>)));
  else
    MXK_WITH_BOOL(HB, hb,
                  MXK_WITH_BOOL(W, wide, MXK_EX((mxk_gemm_bf16_x2_kernel<AN, BN, W, 2 + HB>))));
#undef MXK_EX
}

// (an, bn: the operand is N/M-major; plain integers and pointers, as in the
// dgrad-SwiGLU hook below, so that a caller in another object would do)
void gemm_x2_exp_launch(int an, int bn, bool x2t, int hb, int wide, int grid, hipStream_t stream,
                        const uint16_t* a, const uint16_t* b, uint16_t* c, int M, int N, int K,
                        int lda, int ldb, int ldc) {
  MXK_WITH_BOOL(AN, an,
                MXK_WITH_BOOL(BN, bn,
                              (launch_x2_exp<AN, BN>(x2t, hb, wide, grid, stream, a, b, c, M, N, K,
                                                     lda, ldb, ldc))));
}

// The dgrad-SwiGLU records: staggered by XCD group over cx CUs per XCD (stag;
// +0.8 %, profiles/r4_step/swiglu_epilogue_stagger.log), no SwiGLU math (EPI
// 6, timing ablation), no g/u prefetch (EPI 5), and EPI 4 with the B-outer
// MFMA order.  Returns 0, or -1 with nothing launched: the call is none of
// them, or the staggered form's workspace cannot be had.
template <int EPI, int SCHED = 0, bool STAG = false>
void launch_dgrad_swiglu_exp(int grid, hipStream_t stream, const void* dy, const void* w2,
                             const void* gu, void* dgu, int M, int F, int K, int ld_dy, int ld_w2,
                             float* ws = nullptr, int* flags = nullptr, int cx = 0) {
  MXK_LAUNCH_GEMM((mxk_gemm_bf16_x2_kernel<false, true, EPI, SCHED, false, STAG>), dim3(grid),
                  dim3(XT), stream, bf(dy), bf(w2), bf(dgu), M, F, K, ld_dy, ld_w2, 2 * F, bf(gu), ws,
                  0, flags, cx);
}

int gemm_dgrad_swiglu_exp_launch(int epi, int order, int stag, int cx, int grid, hipStream_t stream,
                                 const void* dy, const void* w2, const void* gu, void* dgu, int M,
                                 int F, int K, int ld_dy, int ld_w2) {
#define MXK_DGRAD_ARGS grid, stream, dy, w2, gu, dgu, M, F, K, ld_dy, ld_w2
  if (stag) {
    const SwigluStagWs* w = swiglu_stag_ws(stream, 4 * cx);
    if (!w) return -1;
    launch_dgrad_swiglu_exp<4, 0, true>(MXK_DGRAD_ARGS, w->ws, w->flags, cx);
  } else if (epi == 6) launch_dgrad_swiglu_exp<6>(MXK_DGRAD_ARGS);
  else if (epi == 5) launch_dgrad_swiglu_exp<5>(MXK_DGRAD_ARGS);
  else if (order) launch_dgrad_swiglu_exp<4, 2>(MXK_DGRAD_ARGS);
  else return -1;
#undef MXK_DGRAD_ARGS
  return 0;
}
}  // namespace

