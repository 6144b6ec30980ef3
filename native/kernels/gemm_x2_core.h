// Shared core of the layout-generic bf16 MFMA GEMM (gemm_bf16_layouts.hip,
// whose header describes the operand images): tile constants, the operand
// template XOp<>, the table-driven three-barrier K-tile and the x / x2 kernel
// templates.  gemm_bf16_layouts.hip instantiates what ships; the A/B records
// (experiments/gemm_layouts_exp.hip) include this header too.
#pragma once
#include <type_traits>

#include "mx_common.h"

namespace {
constexpr int XT = 256;          // threads (4 waves)
constexpr int XBM = 256;         // macro tile M = N = 256
constexpr int XBK = 64;          // k per stage
constexpr int XGROUP_M = 8;
constexpr int TGROUP = 4224;     // bytes per 8 k-rows (4096 + 128 pad)
constexpr int KSTEP_T = 4 * TGROUP;   // 32 k-rows

typedef __attribute__((address_space(3))) void lds_void;

__device__ __forceinline__ void xmfma(f32x4_t& acc, bf16x8_t a, bf16x8_t b) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}

using mxk::u32x4;
using mxk::make_rsrc;
using mxk::dma16;

__device__ __forceinline__ bf16x4_t tr_b64(const char* p) {
  typedef short s4 __attribute__((ext_vector_type(4)));
  // a plain address-space cast (not via an integer) keeps `base + constant`
  // visible, so the constant lands in the instruction's offset field
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)p);
}

template <bool NMAJOR>
struct XOp;

// K-major operand [rows][K]: identical to the w4b kernel's operand.
template <>
struct XOp<false> {
  static constexpr int BYTES = 256 * 128;
  u32x4 rsrc;
  uint32_t lane_off, piece_stride;
  uint32_t voff[8];              // lane_off + (p*4 + wave) * piece_stride
  const char* base;
  unsigned bytes;
  int off0, off1;
  __device__ __forceinline__ void init(const uint16_t* src, int ld, int row0, int K, int lane,
                                       int wave) {
    rsrc = make_rsrc(src + static_cast<size_t>(row0) * ld, 256u * ld * 2u);
    base = reinterpret_cast<const char*>(src + static_cast<size_t>(row0) * ld);
    bytes = 256u * ld * 2u;
    const int r = lane >> 3;
    const int c = (lane & 7) ^ ((4 * (wave & 1) + (r >> 1)) & 7);
    lane_off = static_cast<uint32_t>(r * ld * 2 + c * 16);
    piece_stride = static_cast<uint32_t>(8 * ld * 2);
#pragma unroll
    for (int p = 0; p < 8; ++p) voff[p] = lane_off + (p * 4 + wave) * piece_stride;
    const int frow = lane & 15;
    const int fch = (lane >> 4) ^ (frow >> 1);
    off0 = frow * 128 + fch * 16;
    off1 = frow * 128 + (fch ^ 4) * 16;
    (void)K;
  }
  __device__ __forceinline__ void issue(char* lds, int p, int kstage, int wave) const {
    const int g = p * 4 + wave;
    // hipBLASLt-style addressing: per-piece VGPR offset, k folded into the base
    dma16(make_rsrc(base + kstage * (XBK * 2), bytes), lds + g * 1024, voff[p], 0);
  }
  // x2 kernel: fixed panel descriptor, the k offset of the stage as soffset
  __device__ __forceinline__ uint32_t kstep() const { return XBK * 2; }
  // x2 kernel: LDS destinations as smem32 + (lds - smem), scalar arithmetic
  const char* sm = nullptr;
  uint32_t sm32 = 0;
  __device__ __forceinline__ void set_lds(const char* smem, uint32_t smem32) {
    sm = smem;
    sm32 = smem32;
  }
  __device__ __forceinline__ uint32_t dst32(char* lds, int p, int wave) const {
    return sm32 + static_cast<uint32_t>(lds - sm) + (p * 4 + wave) * 1024;
  }
  __device__ __forceinline__ void issue_s(char* lds, int p, uint32_t soff, int wave) const {
    mxk::dma16m(rsrc, dst32(lds, p, wave), voff[p], soff);
  }
  // K loop: M0 <- dst32 of the piece in a gap ahead of it (mxk::m0_put), then the bare piece
  __device__ __forceinline__ void issue_q(int p, uint32_t soff) const {
    mxk::dma16q(rsrc, voff[p], soff);
  }
  // fragment of 16-row subtile i (i = 0..15 over the 256 rows), k-step ks
  __device__ __forceinline__ bf16x8_t frag(const char* lds, int i, int ks) const {
    return *reinterpret_cast<const bf16x8_t*>(lds + i * 2048 + (ks ? off1 : off0));
  }
};

// N/M-major operand [K][cols]: 64 k-rows x 256 columns per stage.
template <>
struct XOp<true> {
  static constexpr int BYTES = 8 * TGROUP;
  u32x4 rsrc;
  uint32_t lane_off, piece_stride, kstride;
  uint32_t voff[8];
  const char* base;
  unsigned bytes;
  int roff[4];                   // read offset of subtile r (mod 4), XOR folded in
  __device__ __forceinline__ void init(const uint16_t* src, int ld, int col0, int K, int lane,
                                       int wave) {
    rsrc = make_rsrc(src + col0, static_cast<unsigned>(K) * ld * 2u);
    base = reinterpret_cast<const char*>(src + col0);
    bytes = static_cast<unsigned>(K) * ld * 2u;
    // piece g = 4p + wave holds k-rows 8p + 2 wave + h (h = lane >> 5)
    const int h = lane >> 5, slot = lane & 31;
    const int c = slot ^ (2 * ((2 * wave + h) & 3));
    lane_off = static_cast<uint32_t>(h * ld * 2 + c * 16);
    piece_stride = static_cast<uint32_t>(2 * ld * 2);
    kstride = static_cast<uint32_t>(XBK * ld * 2);
#pragma unroll
    for (int p = 0; p < 8; ++p) voff[p] = lane_off + (p * 4 + wave) * piece_stride;
    // transposed-read lane constants: group G, row q, column pair b, half-chunk
    const int G = lane >> 4, i16 = lane & 15, q = i16 >> 2;
    // subtile i sits at column byte (32 i) ^ 32q = 32 (i & ~3) + ((32 (i & 3)) ^ 32q):
    // one VGPR per (i & 3), everything else an immediate offset of the read
    const int base_off = G * TGROUP + q * 512 + ((i16 & 3) >> 1) * 16 + 8 * (i16 & 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) roff[r] = base_off + ((32 * r) ^ (32 * q));
  }
  __device__ __forceinline__ void issue(char* lds, int p, int kstage, int wave) const {
    const uint32_t k_off = kstage * kstride;
    dma16(make_rsrc(base + k_off, bytes - k_off), lds + p * TGROUP + wave * 1024, voff[p], 0);
  }
  __device__ __forceinline__ uint32_t kstep() const { return kstride; }
  const char* sm = nullptr;
  uint32_t sm32 = 0;
  __device__ __forceinline__ void set_lds(const char* smem, uint32_t smem32) {
    sm = smem;
    sm32 = smem32;
  }
  __device__ __forceinline__ uint32_t dst32(char* lds, int p, int wave) const {
    return sm32 + static_cast<uint32_t>(lds - sm) + p * TGROUP + wave * 1024;
  }
  __device__ __forceinline__ void issue_s(char* lds, int p, uint32_t soff, int wave) const {
    mxk::dma16m(rsrc, dst32(lds, p, wave), voff[p], soff);
  }
  __device__ __forceinline__ void issue_q(int p, uint32_t soff) const {
    mxk::dma16q(rsrc, voff[p], soff);
  }
  __device__ __forceinline__ bf16x8_t frag(const char* lds, int i, int ks) const {
    const char* p = lds + roff[i & 3] + 32 * (i & ~3) + ks * KSTEP_T;
    const bf16x4_t lo = tr_b64(p);
    const bf16x4_t hi = tr_b64(p + 2048);
    bf16x8_t a;
    a[0] = lo[0]; a[1] = lo[1]; a[2] = lo[2]; a[3] = lo[3];
    a[4] = hi[0]; a[5] = hi[1]; a[6] = hi[2]; a[7] = hi[3];
    return a;
  }
};
}  // namespace

template <bool AN, bool BN>
__global__ void __launch_bounds__(XT, 1)
mxk_gemm_bf16_x_kernel(const uint16_t* __restrict__ A, const uint16_t* __restrict__ B,
                       uint16_t* __restrict__ C, int M, int N, int K, int lda, int ldb, int ldc) {
  constexpr int A_BYTES = XOp<AN>::BYTES;
  constexpr int STAGE = A_BYTES + XOp<BN>::BYTES;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1;
  const int wn = wave & 1;

  const int tiles_m = M / XBM, tiles_n = N / XBM;
  const int wgid = mxk::xcd_remap(blockIdx.x, gridDim.x);
  const int per_group = XGROUP_M * tiles_n;
  const int group = wgid / per_group;
  const int first_m = group * XGROUP_M;
  const int gsize = min(tiles_m - first_m, XGROUP_M);
  const int in_group = wgid - group * per_group;
  const int m0 = (first_m + in_group % gsize) * XBM;
  const int n0 = (in_group / gsize) * XBM;

  XOp<AN> oa;
  XOp<BN> ob;
  oa.init(A, lda, m0, K, lane, wave);
  ob.init(B, ldb, n0, K, lane, wave);

  f32x4_t acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int ns = K / XBK;
  auto kst = [&](int st) { return st < ns ? st : ns - 1; };
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    char* buf = smem + s * STAGE;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      oa.issue(buf, p, kst(s), wave);
      ob.issue(buf + A_BYTES, p, kst(s), wave);
    }
  }
  asm volatile("s_waitcnt vmcnt(16)" ::: "memory");   // own pieces of stage 0 landed
  __builtin_amdgcn_s_barrier();

  // wave (wm, wn) owns subtiles wm*8 .. wm*8+7 of A and wn*8 .. of B
  bf16x8_t f0a[8], f0b[8], f1a[8], f1b[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) f0a[i] = oa.frag(smem, wm * 8 + i, 0);
#pragma unroll
  for (int j = 0; j < 8; ++j) f0b[j] = ob.frag(smem + A_BYTES, wn * 8 + j, 0);

  for (int s = 0; s < ns; ++s) {
    char* cur = smem + (s & 1) * STAGE;
    char* nxt = smem + ((s + 1) & 1) * STAGE;
    // ---- k-step s.0: MFMAs on set 0, prefetch set 1 from `cur`
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        xmfma(acc[i][j], f0b[j], f0a[i]);
        if ((j & 3) == 3) {
          const int r = i * 2 + (j >> 2);
          if (r < 8) f1b[r] = ob.frag(cur + A_BYTES, wn * 8 + r, 1);
          else f1a[r - 8] = oa.frag(cur, wm * 8 + r - 8, 1);
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_s_waitcnt(0xC07F);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // own pieces of stage s+1 landed
    __builtin_amdgcn_s_barrier();
    // ---- k-step s.1: MFMAs on set 1, prefetch set 0 of stage s+1 from
    //      `nxt`, DMA stage s+2 into `cur` (consumed: certified by the barrier)
    const int k2 = kst(s + 2);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        xmfma(acc[i][j], f1b[j], f1a[i]);
        if ((j & 3) == 1) {
          const int r = i * 2 + (j >> 2);
          if (r < 8) f0b[r] = ob.frag(nxt + A_BYTES, wn * 8 + r, 0);
          else f0a[r - 8] = oa.frag(nxt, wm * 8 + r - 8, 0);
        }
        if ((j & 3) == 3) {
          const int p = i * 2 + (j >> 2);
          if (p < 8) oa.issue(cur, p, k2, wave);
          else ob.issue(cur + A_BYTES, p - 8, k2, wave);
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  mxk::mfma_drain(acc);

  const int crow = lane & 15;
  const int ccol = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int m = m0 + wm * 128 + i * 16 + crow;
    uint16_t* cp = C + static_cast<size_t>(m) * ldc + n0 + wn * 128 + ccol;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const f32x4_t v = acc[i][j];
      uint2 pk;
      pk.x = mxk::pack2bf(v[0], v[1]);
      pk.y = mxk::pack2bf(v[2], v[3]);
      *reinterpret_cast<uint2*>(cp + j * 16) = pk;
    }
  }
}

// ---------------------------------------------------------------------------
// x2: the layout-generic GEMM on gemm_bf16.hip's w4i schedule (three
// barriers per K-tile with in-place refill of the consumed stage, K loop
// unrolled by two with compile-time LDS bases, the stage's k offset as the
// DMA soffset on a fixed descriptor, DMA-free last two K-tiles, XCD
// super-block tile map, widened store tail).
// ---------------------------------------------------------------------------
// The K-tile, table-driven: S (mx_common.h: SchedX2, the kernel's own
// positions, or SchedHB, hipBLASLt's) gives, per MFMA index m = 0..127, the
// fragment reads, DMA pieces, waits and barriers that follow MFMA m.
// MODE 1: with DMA; 2: no DMA, vmcnt(0) at barrier #3; 3: last K-tile.
// PRIO: s_setprio 1 / 0 around the K-tile.  VMD is added to the stage wait's
// vmcnt: the vector-memory ops beyond the schedule's own pieces that are
// younger than the stage being waited for (the trickle kernel's C stores sit
// among the DMA pieces); HOOK(m) runs after MFMA m.
// The pieces go out bare (mxk::dma16q), each with its LDS address written to
// M0 in an earlier, piece-free MFMA gap (S::am0 / S::bm0): nothing else in a
// MODE 1 K-tile uses M0, and no descriptor or offset SGPR of a piece is
// VALU-written there (both audited on the listing, tests/test_isa_dma_gaps.py
// and test_isa_hazards.py).  A HOOK must not touch M0 in a MODE 1 K-tile.
// QDMA false: every piece through dma16m, M0 write and nop beside it (the
// trickle-store A/B records keep it: they sit at the VGPR limit, and the
// bare pieces tipped one of them into spills).
template <class S, bool AN, bool BN, int PAR, int MODE, int PRIO = 0, int VMD = 0,
          class HOOK = mxk::NoHook, int ORDER = 0, bool QDMA = true>
__device__ __forceinline__ void x2_ktile(f32x4_t (&acc)[8][8], bf16x8_t (&f0a)[8],
                                         bf16x8_t (&f0b)[8], bf16x8_t (&f1a)[8],
                                         bf16x8_t (&f1b)[8], char* smem, const XOp<AN>& oa,
                                         const XOp<BN>& ob, int wm, int wn, uint32_t soa,
                                         uint32_t sob, int wave, int par = 0,
                                         const HOOK& hook = HOOK{}) {
  constexpr int A_BYTES = XOp<AN>::BYTES;
  constexpr int STAGE = A_BYTES + XOp<BN>::BYTES;
  const int px = PAR == 2 ? par : PAR;
  char* X = smem + px * STAGE;
  char* Y = smem + (px ^ 1) * STAGE;
  if constexpr (PRIO) __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
#pragma unroll
    for (int o = 0; o < 8; ++o) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int m = h * 64 + o * 8 + q;
        // ORDER 0: A fragment outer; 1: B outer (srcA held for 8 MFMAs)
        const int i = ORDER ? q : o, j = ORDER ? o : q;
        if (h == 0) xmfma(acc[i][j], f0b[j], f0a[i]);
        else xmfma(acc[i][j], f1b[j], f1a[i]);
        hook(m);
        if (S::a1(m) >= 0) f1a[S::a1(m)] = oa.frag(X, wm * 8 + S::a1(m), 1);
        if (MODE == 1 && m == S::W1) __builtin_amdgcn_s_waitcnt(0xC07F);
        if (MODE == 1 && m == S::B1) __builtin_amdgcn_s_barrier();
        if constexpr (QDMA && MODE == 1) {
          if (S::am0(m) >= 0) mxk::m0_put(oa.dst32(X, S::am0(m), wave));
          if (S::bm0(m) >= 0) mxk::m0_put(ob.dst32(X + A_BYTES, S::bm0(m), wave));
        }
        if (MODE == 1 && S::adma(m) >= 0) {
          if constexpr (QDMA) oa.issue_q(S::adma(m), soa);
          else oa.issue_s(X, S::adma(m), soa, wave);
        }
        if (S::b1(m) >= 0) f1b[S::b1(m)] = ob.frag(X + A_BYTES, wn * 8 + S::b1(m), 1);
        if (MODE == 1 && m == S::W2) __builtin_amdgcn_s_waitcnt(0xC07F);
        if (MODE == 1 && m == S::B2) __builtin_amdgcn_s_barrier();
        if (MODE == 1 && S::bdma(m) >= 0) {
          if constexpr (QDMA) ob.issue_q(S::bdma(m), sob);
          else ob.issue_s(X + A_BYTES, S::bdma(m), sob, wave);
        }
        if (MODE != 3 && m == S::W3) {
          if constexpr (MODE == 1) mxk::vm_wait_n<S::VM3 + VMD>();
          else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        if (MODE != 3 && m == S::B3) __builtin_amdgcn_s_barrier();
        if (MODE != 3 && S::k0(m) >= 0) {
          const int r = S::k0(m);
          if (r < 8) f0b[r] = ob.frag(Y + A_BYTES, wn * 8 + r, 0);
          else f0a[r - 8] = oa.frag(Y, wm * 8 + r - 8, 0);
        }
      }
    }
  }
  if constexpr (PRIO) __builtin_amdgcn_s_setprio(0);
}

// SCHED bit 0: hipBLASLt's positions (SchedHB, no raised priority), else the
// kernel's own (SchedX2, raised priority); bit 1: B-outer MFMA order
template <int SCHED, bool AN, bool BN, int PAR, int MODE, int VMD = 0, class HOOK = mxk::NoHook,
          bool QDMA = true>
__device__ __forceinline__ void x2_ktile_s(f32x4_t (&acc)[8][8], bf16x8_t (&f0a)[8],
                                           bf16x8_t (&f0b)[8], bf16x8_t (&f1a)[8],
                                           bf16x8_t (&f1b)[8], char* smem, const XOp<AN>& oa,
                                           const XOp<BN>& ob, int wm, int wn, uint32_t soa,
                                           uint32_t sob, int wave, int par = 0,
                                           const HOOK& hook = HOOK{}) {
  constexpr bool HB = (SCHED & 1) == 1;
  using S = std::conditional_t<HB, mxk::SchedHB, mxk::SchedX2>;
  x2_ktile<S, AN, BN, PAR, MODE, !HB, VMD, HOOK, (SCHED >> 1) & 1, QDMA>(
      acc, f0a, f0b, f1a, f1b, smem, oa, ob, wm, wn, soa, sob, wave, par, hook);
}

// EPI 0: 8-B stores, 1: 16-B stores through LDS (whole lines), 2: SwiGLU backward, 3: SwiGLU
// backward with 16-B g / u accesses (mxk::swiglu_bwd_block_wide), 4: the same
// staged through LDS so each access covers whole lines (swiglu_bwd_block_lds)
// (mxk::swiglu_bwd_block: C = d[g | u], aux = [g | u], both row stride ldc,
// u at column offset N).
// SPLIT (split tail): the launch after the whole-tile one (grid q_full,
// tiles [0, q_full) of the same map) covers the last T - q_full tiles (at
// most half a round) as two K halves each, one workgroup per half
// (blockIdx 2t + h), so the 2(T - q_full) halves fill the final round
// instead of leaving half the CUs idle.  A half writes its fp32 partial
// tile to ws[2t + h] ([256][256]); mxk_gemm_split_fixup sums the pair into
// C.  A separate kernel (not a branch of the whole-tile one): with both
// epilogues in one body the allocator spilled accumulators, and a spill
// store of an AGPR right behind its inline-asm MFMA reads a stale value.
// EPI 4 (SwiGLU backward): pass 0's g / u rows of each wave by LDS-DMA into
// the stage the last K-tile does not read, issued right after the second-to-
// last K-tile's stage barrier (m 96; that stage is free everywhere by then):
// 16 pieces per wave (8 of g, 8 of u), each 4 rows x 256 B, one per MFMA from
// m 97.  The epilogue's vmcnt(0) + barrier covers them.
struct GuPrefetch : mxk::NoHook {
  mxk::u32x4 rsrc;
  uint32_t voff;     // this lane's (row, column) of piece 0, bytes
  uint32_t rowstep;  // 4 rows, bytes
  uint32_t fbytes;   // F columns (g -> u), bytes
  uint32_t lds;      // LDS address of this wave's 16 KiB
  __device__ __forceinline__ void operator()(int m) const {
    if (m >= 97 && m < 113) {
      const int q = m - 97, u = q >> 3, i = q & 7;
      mxk::dma16m(rsrc, lds + u * 8192 + i * 1024, voff + i * rowstep + u * fbytes, 0);
    }
  }
};

// STAG (EPI 4 only, the down projection's dgrad-SwiGLU): rounds staggered by
// XCD group (mx_common.h stagger_part_xcd; TN schedule 57's mapping): XCDs 4-7
// run half a tile out of phase with XCDs 0-3, so the two halves of the chip
// take turns with the epilogue's HBM traffic (1.9 GB per Llama-3-8B layer,
// +19 % over a plain store when every CU bursts at once,
// profiles/r4_step/swiglu_epilogue_price.log) instead of all bursting at once.
// A first K half leaves d as fp32 rows in ws[slot] and raises flags[slot]; the
// second half (later on the same XCD) waits for it, adds it in the epilogue.
template <bool AN, bool BN, int EPI, int SCHED = 0, bool SPLIT = false, bool STAG = false>
__global__ void __launch_bounds__(XT, 1)
mxk_gemm_bf16_x2_kernel(const uint16_t* __restrict__ A, const uint16_t* __restrict__ B,
                        uint16_t* __restrict__ C, int M, int N, int K, int lda, int ldb, int ldc,
                        const uint16_t* __restrict__ aux = nullptr, float* __restrict__ ws = nullptr,
                        int q_full = 0, int* __restrict__ flags = nullptr, int stag_cx = 0) {
  constexpr int A_BYTES = XOp<AN>::BYTES;
  constexpr int STAGE = A_BYTES + XOp<BN>::BYTES;
  // EPI 4: 1 KiB more, so the epilogue's acc slices (4 x kSwigluLdsWave from
  // the last K-tile's stage) and the g / u prefetch (64 KiB at the other
  // stage + 1 KiB) never overlap, whichever stage is which
  // EPI 6: EPI 4 with the SwiGLU math removed (timing ablation, wrong values)
  constexpr bool PFEPI = EPI == 4 || EPI == 6;
  static_assert(!PFEPI || (4 * mxk::kSwigluLdsWave <= STAGE + 1024 && 65536 + 1024 <= STAGE),
                "EPI 4 LDS plan");
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE + (PFEPI ? 1024 : 0)];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1;
  const int wn = wave & 1;
  int tile = blockIdx.x, kbeg = 0, klen = K;
  if constexpr (SPLIT) {
    tile = q_full + (static_cast<int>(blockIdx.x) >> 1);
    klen = K >> 1;
    kbeg = (blockIdx.x & 1) * klen;
  }
  mxk::StaggerPart sp{static_cast<int>(blockIdx.x), 0, -1};
  if constexpr (STAG) {
    static_assert(EPI == 4 && !SPLIT, "STAG: the dgrad-SwiGLU epilogue only");
    sp = mxk::stagger_part_xcd(blockIdx.x, (M / XBM) * (N / XBM), stag_cx);
    if (sp.part < 0) return;
    tile = sp.vtile;
    if (sp.part) {
      klen = K >> 1;
      kbeg = sp.part == 2 ? klen : 0;
    }
  }
  int m0, n0;
  mxk::w4b_tile<1>(tile, (M / XBM) * (N / XBM), M / XBM, N / XBM, &m0, &n0);

  XOp<AN> oa;
  XOp<BN> ob;
  // the K range [kbeg, kbeg + klen): K-major operands start kbeg columns in,
  // N/M-major ones kbeg rows down
  oa.init(AN ? A + static_cast<size_t>(kbeg) * lda : A + kbeg, lda, m0, klen, lane, wave);
  ob.init(BN ? B + static_cast<size_t>(kbeg) * ldb : B + kbeg, ldb, n0, klen, lane, wave);
  oa.set_lds(smem, mxk::lds_addr32(smem));
  ob.set_lds(smem, mxk::lds_addr32(smem));

  f32x4_t acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int ns = klen / XBK;
  const uint32_t ka = oa.kstep(), kb = ob.kstep();
#pragma unroll
  for (int p = 0; p < 8; ++p) oa.issue_s(smem, p, 0, wave);
#pragma unroll
  for (int p = 0; p < 8; ++p) ob.issue_s(smem + A_BYTES, p, 0, wave);
  if (ns > 1) {
#pragma unroll
    for (int p = 0; p < 8; ++p) oa.issue_s(smem + STAGE, p, ka, wave);
#pragma unroll
    for (int p = 0; p < 8; ++p) ob.issue_s(smem + STAGE + A_BYTES, p, kb, wave);
    asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();

  bf16x8_t f0a[8], f0b[8], f1a[8], f1b[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) f0b[j] = ob.frag(smem + A_BYTES, wn * 8 + j, 0);
#pragma unroll
  for (int i = 0; i < 8; ++i) f0a[i] = oa.frag(smem, wm * 8 + i, 0);
  __builtin_amdgcn_s_waitcnt(0xC07F);

  int s = 0;
  uint32_t sa = 2 * ka, sb = 2 * kb;
  for (; s + 2 <= ns - 2; s += 2) {
    x2_ktile_s<SCHED, AN, BN, 0, 1>(acc, f0a, f0b, f1a, f1b, smem, oa, ob, wm, wn, sa, sb, wave);
    x2_ktile_s<SCHED, AN, BN, 1, 1>(acc, f0a, f0b, f1a, f1b, smem, oa, ob, wm, wn, sa + ka, sb + kb, wave);
    sa += 2 * ka;
    sb += 2 * kb;
  }
  if (s < ns - 2) {
    x2_ktile_s<SCHED, AN, BN, 0, 1>(acc, f0a, f0b, f1a, f1b, smem, oa, ob, wm, wn, sa, sb, wave);
    ++s;
  }
  if (ns >= 2) {
    if constexpr (PFEPI && (SCHED & 1) == 0 && !SPLIT) {
      // stage s & 1 is read by this K-tile; the last one reads the other
      GuPrefetch pf;
      pf.rsrc = mxk::make_rsrc(aux, 0xFFFFFFF0u);
      const int rr = lane >> 4, cc = (lane & 15) * 8;
      pf.voff = static_cast<uint32_t>(
          (static_cast<long>(m0 + wm * 128 + rr) * ldc + n0 + wn * 128 + cc) * 2);
      pf.rowstep = static_cast<uint32_t>(4L * ldc * 2);
      pf.fbytes = static_cast<uint32_t>(N * 2);
      pf.lds = mxk::lds_addr32(smem) + (s & 1) * STAGE + 1024 + wave * 16384;
      x2_ktile<mxk::SchedX2, AN, BN, 2, 2, 1, 0, GuPrefetch, (SCHED >> 1) & 1>(
          acc, f0a, f0b, f1a, f1b, smem, oa, ob, wm, wn, 0, 0, wave, s & 1, pf);
    } else {
      x2_ktile_s<SCHED, AN, BN, 2, 2>(acc, f0a, f0b, f1a, f1b, smem, oa, ob, wm, wn, 0, 0, wave,
                                      s & 1);
    }
    ++s;
  }
  x2_ktile_s<SCHED, AN, BN, 2, 3>(acc, f0a, f0b, f1a, f1b, smem, oa, ob, wm, wn, 0, 0, wave, s & 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  mxk::mfma_drain(acc);

  if constexpr (SPLIT) {
    // fp32 partial: lane holds 4 consecutive columns of row i*16 + (lane & 15)
    float* wp = ws + static_cast<size_t>(blockIdx.x) * (XBM * XBM);
    const int r0 = wm * 128 + (lane & 15), c0 = wn * 128 + (lane >> 4) * 4;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        *reinterpret_cast<f32x4_t*>(wp + (r0 + i * 16) * XBM + c0 + j * 16) = acc[i][j];
  } else if constexpr (EPI == 2)
    mxk::swiglu_bwd_block(acc, aux, C, ldc, N, m0 + wm * 128, n0 + wn * 128, lane);
  else if constexpr (EPI == 3)
    mxk::swiglu_bwd_block_wide(acc, aux, C, ldc, N, m0 + wm * 128, n0 + wn * 128, lane);
  else if constexpr (EPI == 5) {
    // EPI 4 without the g / u prefetch (A/B: MXK_SWIGLU_WIDE=5)
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();
    mxk::swiglu_bwd_block_lds(acc, aux, C, ldc, N, m0 + wm * 128, n0 + wn * 128, lane,
                              smem + wave * mxk::kSwigluLdsWave);
  }
  else if constexpr (PFEPI) {
    static_assert(4 * mxk::kSwigluLdsWave <= 2 * STAGE, "LDS slice per wave");
    // every wave's last-stage fragment reads retired before any slice is written
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();
    // acc slices in the stage the last K-tile read (s & 1); the g / u rows of
    // pass 0 were prefetched into the other one (ns >= 2)
    // (the launcher takes EPI 4 only for K >= 2 * XBK, so that K-tile ran)
    char* last = smem + (s & 1) * STAGE;
    const char* gul = smem + ((s & 1) ^ 1) * STAGE + 1024 + wave * 16384;
    constexpr bool PFX = (SCHED & 1) == 0 && !SPLIT;
    if constexpr (STAG) {
      float* part = ws + static_cast<size_t>(sp.slot) * (XBM * XBM) + wave * (128 * 128);
      if (sp.part == 1) {
        mxk::swiglu_bwd_block_lds<PFX, false, 1>(acc, aux, C, ldc, N, m0 + wm * 128, n0 + wn * 128,
                                                 lane, last + wave * mxk::kSwigluLdsWave, gul, part);
        __builtin_amdgcn_s_waitcnt(0);            // this wave's partial reached memory
        __syncthreads();
        if (tid == 0) __hip_atomic_store(flags + sp.slot, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
      }
      if (sp.part == 2) {
        if (tid == 0)
          while (__hip_atomic_load(flags + sp.slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
            __builtin_amdgcn_s_sleep(4);
        __syncthreads();
        mxk::swiglu_bwd_block_lds<PFX, false, 2>(acc, aux, C, ldc, N, m0 + wm * 128, n0 + wn * 128,
                                                 lane, last + wave * mxk::kSwigluLdsWave, gul, part);
        __syncthreads();                          // every wave read its partial
        if (tid == 0) __hip_atomic_store(flags + sp.slot, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
      }
    }
    mxk::swiglu_bwd_block_lds<PFX, EPI == 6>(acc, aux, C, ldc, N, m0 + wm * 128, n0 + wn * 128,
                                             lane, last + wave * mxk::kSwigluLdsWave, gul);
  }
  else if constexpr (EPI == 1) {
    // whole-line stores through LDS (as the TN kernel's default schedule);
    // every wave's last fragment reads retired before a slice is written
    static_assert(4 * mxk::kStoreLdsWave <= 2 * STAGE, "LDS slice per wave");
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();
    mxk::store_block_lds<false>(acc, C, ldc, m0 + wm * 128, n0 + wn * 128, lane,
                                smem + wave * mxk::kStoreLdsWave);
  }
  else
    mxk::store_block_narrow(acc, C, ldc, m0 + wm * 128, n0 + wn * 128, lane);
}
