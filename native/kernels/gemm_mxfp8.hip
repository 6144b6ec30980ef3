// MXFP8 (OCP MX, e4m3 elements, one E8M0 scale per 32 K elements) quantiser
// and block-scaled MFMA GEMM for gfx950.
//
//   mxk_quantize_mxfp8   bf16 rows -> e4m3 bytes + E8M0 scale bytes
//   mxk_quantize_mxfp8_t     the same of x^T (blocks of 32 rows), stored transposed
//   mxk_quantize_mxfp8_dual  both images from one read of x
//   mxk_gemm_mxfp8_tn    C[M][N] = dequant(A) . dequant(B)^T, fp32
//                        accumulation, bf16 output; both operands K-contiguous
//
// ---- operand and scale lane map of v_mfma_scale_f32_32x32x64_f8f6f4 --------
// (cbsz = blgp = 0: both operands e4m3; established with the one-hot test of
// tests/test_gpu_mxfp8.py, which puts a distinct value and a distinct scale on
// every (row, K-block))
//   * lane l holds row (A operand) / column (B operand) l & 31; with h = l >> 5,
//     the bytes of its first 4 operand VGPRs are k = 16 h + 0..15 and those of
//     its last 4 VGPRs k = 32 + 16 h + 0..15, in memory order: each half of the
//     8 VGPRs is laid out like the operand of a K = 32 instruction.  (Measured:
//     with 32 consecutive k per lane every product at k % 64 in [16, 48) took
//     the scale of the k-step's other block; unscaled, that permutation is
//     invisible because both operands share it.)
//   * so a lane holds 16 elements of each of the k-step's two MX blocks.  The
//     scale of block b (k = 32 b .. 32 b + 31) of row r comes from the scale
//     VGPR of lane r + 32 b; op_sel picks which of that register's 4 bytes.
//   * C/D is the 32x32 map of every other dtype: column l & 31, row
//     (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
// The kernel hands the B fragment to the instruction's first operand, so the
// lane index is the row of C and each lane owns runs of 4 consecutive columns.
//
// ---- structure --------------------------------------------------------------
// The quantiser kernels are mx_quantize.h's templates on struct E4m3, which the
// MXFP4 file shares.  The GEMM:
// 256x256 output tile, 4 waves (2 x 2, 128x128 each = 4 x 4 MFMA blocks), K-tile
// of 128 elements = 128 B per row = two MFMA k-steps.  A K-tile costs the same
// matrix-core time and stages the same bytes as a bf16 K-tile of 64
// (gemm_tn_core.h); the LDS image (LDS-DMA, 16-B chunks XOR-swizzled by
// (row >> 1) & 7) is the bf16 kernel's.  The 4 scale bytes of a row's K-tile
// are one dword, staged by one 4-B LDS-DMA per wave and operand beside the
// tile.  Two 66 KiB stages; one barrier per K-tile, in its middle:
//   k-step 0 MFMAs  | k-step-1 fragments of stage t (buffer t & 1)
//   lgkmcnt(0), vmcnt(0) (stage t+1 landed), barrier
//   k-step 1 MFMAs  | DMA of stage t+2 into buffer t & 1, k-step-0 fragments
//                     and scales of stage t+1
// so a stage has one whole K-tile to land.  The MFMAs are the compiler
// builtin: it places the hazard waits and the accumulators.
#include "mx_gemm_core.h"
#include "mx_quantize.h"
#include "mx_formats.h"   // struct E4m3, the element format of the shared quantiser kernels

namespace {

using namespace mxk::mx;

// ---------------------------------------------------------------------------
// GEMM
// ---------------------------------------------------------------------------
constexpr int kBK = 128;   // elements per K-tile: 128 B of a row
// one scale dword per row and K-tile, 32 element bytes per scale byte
using Dma8 = Dma<1, 5>;
constexpr int kStageBytes = 2 * kOpBytes + 2048; // 66 KiB: A scales, then B scales (1 KiB each)
constexpr int kDmaPerStage = 18;                 // vector-memory ops per wave and stage

__device__ __forceinline__ i32x8_t lds_frag(const char* p, int off_lo, int off_hi) {
  const i32x4_t lo = *reinterpret_cast<const i32x4_t*>(p + off_lo);
  const i32x4_t hi = *reinterpret_cast<const i32x4_t*>(p + off_hi);
  return i32x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

struct Frags {
  i32x8_t a[4], b[4];
};

// The 16 MFMAs of one k-step.  sa / sb: per row block the lane's scale dword,
// already shifted so that byte 0 / 2 is block lane >> 5 of k-step 0 / 1.
template <int KS>
__device__ __forceinline__ void mfma_kstep(f32x16_t (&acc)[4][4], const Frags& f,
                                           const int (&sa)[4], const int (&sb)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(f.b[j], f.a[i], acc[i][j], 0, 0,
                                                                  2 * KS, sb[j], 2 * KS, sa[i]);
}

__device__ __forceinline__ void read_frags(Frags& f, const char* stage, int a_base, int b_base,
                                           const FragOff& fo, int ks) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
    f.b[j] = lds_frag(stage + kOpBytes + b_base + j * 4096, fo.lo[ks], fo.hi[ks]);
#pragma unroll
  for (int i = 0; i < 4; ++i) f.a[i] = lds_frag(stage + a_base + i * 4096, fo.lo[ks], fo.hi[ks]);
}

__device__ __forceinline__ void read_scales(int (&sa)[4], int (&sb)[4], const char* stage,
                                            int a_row, int b_row, int shift) {
  const int* pa = reinterpret_cast<const int*>(stage + kScaleOff) + a_row;
  const int* pb = reinterpret_cast<const int*>(stage + kScaleOff + 1024) + b_row;
#pragma unroll
  for (int i = 0; i < 4; ++i) sa[i] = static_cast<int>(static_cast<uint32_t>(pa[i * 32]) >> shift);
#pragma unroll
  for (int j = 0; j < 4; ++j) sb[j] = static_cast<int>(static_cast<uint32_t>(pb[j * 32]) >> shift);
}

// K-tile t, read from stage buffer X (Y: the other one).  DMA: stage t+2
// exists and goes out here, at k offset kb2 bytes (every K-tile but the last
// two).  The reads of stage t+1 are unconditional: in the last K-tile they
// fetch stale LDS that nothing uses, which keeps each loop to one body with
// plain loop-carried registers.
// The MFMAs are no memory operations, so the compiler would move them across
// the waits; the sched barriers keep each k-step in its phase and interleave
// it with that phase's LDS reads and DMA pieces (masks: 0x008 MFMA, 0x080 DS,
// 0x010 vector memory).
template <bool DMA>
__device__ __forceinline__ void ktile(f32x16_t (&acc)[4][4], Frags& f0, int (&sa)[4], int (&sb)[4],
                                      char* X, char* Y, const Dma8& dma_a, const Dma8& dma_b,
                                      int a_base, int b_base, int a_row, int b_row, int shift,
                                      const FragOff& fo, int kb2, int wave) {
  Frags f1;
  read_frags(f1, X, a_base, b_base, fo, 1);
  mfma_kstep<0>(acc, f0, sa, sb);
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x080, 1, 0);
  }
  __builtin_amdgcn_sched_barrier(0);
  // every read of stage t retired; this wave's pieces of stage t+1 landed
  lds_fence();
  mxk::vm_wait_n<0>();
  block_barrier();
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (DMA) {
    dma_a.issue(X, X + kScaleOff, kb2, wave);
    dma_b.issue(X + kOpBytes, X + kScaleOff + 1024, kb2, wave);
  }
  int na[4], nb[4];
  read_scales(na, nb, Y, a_row, b_row, shift);
  read_frags(f0, Y, a_base, b_base, fo, 0);
  mfma_kstep<1>(acc, f1, sa, sb);
  // 24 LDS reads behind the first 8 MFMAs, the 18 DMA pieces spread over all 16
  if constexpr (DMA) __builtin_amdgcn_sched_group_barrier(0x010, 2, 0);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x080, 3, 0);
    if constexpr (DMA) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    if constexpr (DMA) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    sa[i] = na[i];
    sb[i] = nb[i];
  }
}

__global__ void __launch_bounds__(kThreads, 1)
mxk_gemm_mxfp8_tn_kernel(const uint8_t* __restrict__ Aq, const uint8_t* __restrict__ As,
                         const uint8_t* __restrict__ Bq, const uint8_t* __restrict__ Bs,
                         uint16_t* __restrict__ C, int M, int N, int K, int lda, int ldsa, int ldb,
                         int ldsb, int ldc) {
  static_assert(4 * mxk::kStoreLdsWave <= 2 * kStageBytes, "epilogue slices fit the stages");
  __shared__ __attribute__((aligned(16))) char smem[2 * kStageBytes];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  int m0, n0;
  mxk::w4b_tile<1>(blockIdx.x, gridDim.x, M / kBM, N / kBN, &m0, &n0);
  const Dma8 dma_a = Dma8::make(Aq, As, lda, ldsa, m0, lane, wave);
  const Dma8 dma_b = Dma8::make(Bq, Bs, ldb, ldsb, n0, lane, wave);
  const int ns = K / kBK;

  const int r32 = lane & 31, h = lane >> 5;
  const int sw = (r32 >> 1) & 7;
  FragOff fo;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    fo.lo[ks] = r32 * 128 + (((4 * ks + h) ^ sw) << 4);
    fo.hi[ks] = r32 * 128 + (((4 * ks + 2 + h) ^ sw) << 4);
  }
  const int a_base = wm * 128 * 128, b_base = wn * 128 * 128;   // byte offset of the wave's rows
  const int a_row = wm * 128 + r32, b_row = wn * 128 + r32;
  const int shift = 8 * h;

  f32x16_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  // An (empty) asm with an AGPR operand makes hipcc select the MFMAs' AGPR
  // form, so the 256 accumulator registers live in the AGPR half of the file
  // and the operands in the VGPR half; without it the builtin's VGPR form has
  // to fit both into v0-v255 and spills.
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" : "+a"(acc[i][j]));

  // stages 0 and 1
  dma_a.issue(smem, smem + kScaleOff, 0, wave);
  dma_b.issue(smem + kOpBytes, smem + kScaleOff + 1024, 0, wave);
  if (ns > 1) {
    dma_a.issue(smem + kStageBytes, smem + kStageBytes + kScaleOff, kBK, wave);
    dma_b.issue(smem + kStageBytes + kOpBytes, smem + kStageBytes + kScaleOff + 1024, kBK, wave);
    mxk::vm_wait_n<kDmaPerStage>();
  } else {
    mxk::vm_wait_n<0>();
  }
  block_barrier();

  Frags f0;
  int sa[4], sb[4];
  read_frags(f0, smem, a_base, b_base, fo, 0);
  read_scales(sa, sb, smem, a_row, b_row, shift);

  int kb2 = 2 * kBK;
  int t = 0;
#pragma clang loop unroll(disable)
  for (; t + 2 < ns; ++t) {
    char* X = smem + (t & 1) * kStageBytes;
    char* Y = smem + ((t & 1) ^ 1) * kStageBytes;
    ktile<true>(acc, f0, sa, sb, X, Y, dma_a, dma_b, a_base, b_base, a_row, b_row, shift, fo, kb2,
                wave);
    kb2 += kBK;
  }
  // the last two K-tiles (or the only one): no DMA
#pragma clang loop unroll(disable)
  for (; t < ns; ++t) {
    char* X = smem + (t & 1) * kStageBytes;
    char* Y = smem + ((t & 1) ^ 1) * kStageBytes;
    ktile<false>(acc, f0, sa, sb, X, Y, dma_a, dma_b, a_base, b_base, a_row, b_row, shift, fo, 0,
                 wave);
  }

  // every wave's last fragment reads retired before the slices overwrite the stages
  lds_fence();
  block_barrier();
  store_block32_lds(acc, C, ldc, m0 + wm * 128, n0 + wn * 128, lane,
                    smem + wave * mxk::kStoreLdsWave);
}

}  // namespace

MXK_API int mxk_gemm_mxfp8_tn_is_fast(int M, int N, int K) {
  return gemm_tn_shape_ok(M, N, K, kBK) ? 1 : 0;
}

// The contract is gemm_tn_args_ok's (mx_gemm_core.h), one element per byte.
MXK_API int mxk_gemm_mxfp8_tn(const void* Aq, const void* As, const void* Bq, const void* Bs,
                              void* C, int M, int N, int K, int lda, int ldsa, int ldb, int ldsb,
                              int ldc, hipStream_t stream) {
  return launch_gemm_tn<kBK>(mxk_gemm_mxfp8_tn_kernel, Aq, As, Bq, Bs, C, M, N, K, lda, ldsa, ldb, ldsb,
                               ldc, stream);
}

// x: bf16 [R][K] (row stride ldx elements), K % 32 == 0, finite values only.
// q: e4m3 bytes [R][K] (row stride ldq), s: E8M0 bytes [R][K / 32] (row stride
// lds).  Per block of 32: e = clamp(floor(log2(amax)) - 8, -127, 127), scale
// byte e + 127 (127 for a zero block), element RNE(clamp(x 2^-e, +-448)).
MXK_API int mxk_quantize_mxfp8(const void* x, void* q, void* s, long R, int K, long ldx, long ldq,
                               long lds, hipStream_t stream) {
  return launch_quantize_rows<E4m3>(x, q, s, R, K, ldx, ldq, lds, stream);
}

// x: bf16 [R][C] (row stride ldx elements), R % 32 == 0, finite values only.
// qt: e4m3 bytes [C][R] (row stride ldqt), st: E8M0 bytes [C][R / 32] (row
// stride ldst): mxk_quantize_mxfp8 of x^T, the MX blocks being 32 consecutive
// rows of x.  Nothing outside the [C][R] and [C][R / 32] extents is written.
MXK_API int mxk_quantize_mxfp8_t(const void* x, void* qt, void* st, long R, long C, long ldx,
                                 long ldqt, long ldst, hipStream_t stream) {
  return launch_quantize_tr<E4m3>(false, x, nullptr, nullptr, qt, st, R, C, ldx, 0, 0, ldqt, ldst, stream);
}

// q / s: the image mxk_quantize_mxfp8 writes (C % 32 == 0 as well); qt / st:
// that of mxk_quantize_mxfp8_t; x is read once.
MXK_API int mxk_quantize_mxfp8_dual(const void* x, void* q, void* s, void* qt, void* st, long R,
                                    long C, long ldx, long ldq, long lds, long ldqt, long ldst,
                                    hipStream_t stream) {
  return launch_quantize_tr<E4m3>(true, x, q, s, qt, st, R, C, ldx, ldq, lds, ldqt, ldst, stream);
}
