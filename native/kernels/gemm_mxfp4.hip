// MXFP4 (OCP MX, e2m1 elements, one E8M0 scale per 32 K elements) quantiser
// and block-scaled MFMA GEMM for gfx950.
//
//   mxk_quantize_mxfp4   bf16 rows -> packed e2m1 nibbles + E8M0 scale bytes
//   mxk_quantize_mxfp4_t     the same of x^T (blocks of 32 rows), stored transposed
//   mxk_quantize_mxfp4_dual  both images from one read of x
//   mxk_gemm_mxfp4_tn    C[M][N] = dequant(A) . dequant(B)^T, fp32
//                        accumulation, bf16 output; both operands K-contiguous
//
// Storage (mxfp4_format.h has the arithmetic): element 2 i of a row sits in
// bits 3:0 of byte i, element 2 i + 1 in bits 7:4; row strides of the packed
// elements (lda, ldb, ldq, ldqt) count bytes.  So byte i of row c of qt holds
// x[2 i][c] in bits 3:0 and x[2 i + 1][c] in bits 7:4.
//
// ---- operand and scale lane map of v_mfma_scale_f32_32x32x64_f8f6f4 --------
// (cbsz = blgp = 4: both operands e2m1, 4 VGPRs each; established with a
// one-wave one-hot probe, every nibble position of one operand against every
// position of the other and a distinct scale in every lane and register byte,
// and held by the one-hot test of tests/test_gpu_mxfp4.py)
//   * lane l holds row (A operand) / column (B operand) l & 31; the 32 nibbles
//     of its 4 operand VGPRs are one whole MX block, k = 32 (l >> 5) + 0..31:
//     nibble n of VGPR v (bits 4 n + 3 : 4 n) pairs with the same nibble of
//     the same VGPR of the other operand's lanes of that half, and with no
//     other (all 64 x 64 position pairs measured).  Any k order inside the
//     block that both operands share is invisible to the product, so memory
//     order (k = 32 (l >> 5) + 8 v + n, the packing of the storage format)
//     serves: the 16 packed bytes of a block go into the VGPRs as they lie.
//     This differs from e4m3, whose lanes hold 16 elements of each block.
//   * the scale of a lane's 32 elements is byte op_sel of that same lane's
//     scale VGPR (measured for op_sel 0..3 and both operands): lane
//     r + 32 b scales block b of row r, as for e4m3, which here is simply
//     "every lane scales what it holds".
//   * the codes multiply as the e2m1 table says, sign in bit 3.
//   * C/D is the 32x32 map of every other dtype: column l & 31, row
//     (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
// The kernel hands the B fragment to the instruction's first operand, so the
// lane index is the row of C and each lane owns runs of 4 consecutive columns.
//
// ---- structure --------------------------------------------------------------
// The tile of mx_gemm_core.h, which the MXFP8 kernel (gemm_mxfp8.hip) shares:
// 256x256 output tile, 4 waves (2 x 2, 128x128 each = 4 x 4 MFMA blocks),
// K-tile of 256 elements = 128 B per row, LDS image (LDS-DMA, 16-B chunks
// XOR-swizzled by (row >> 1) & 7), two stages, one barrier per K-tile.  That
// header holds the staging (LDS-DMA descriptor), barrier and epilogue-store
// helpers and the validation and launch of the GEMM entry point, and
// mx_quantize.h the quantiser kernels as templates on the format, once for
// both formats; this file keeps the format, the kernel with its K-tile, MFMA,
// fragment and scale helpers, and the entry points.  A K-tile is four MFMA
// k-steps of 64; each costs half the matrix-core time of an e4m3 k-step, so
// they are issued in pairs and a pair stands where the MXFP8 kernel has one
// k-step:
//   pair 0 MFMAs  | pair-1 fragments and scales of stage t (buffer t & 1)
//   lgkmcnt(0), vmcnt(0) (stage t+1 landed), barrier
//   pair 1 MFMAs  | DMA of stage t+2 into buffer t & 1, pair-0 fragments and
//                   scales of stage t+1
// A lane's two 16-B fragment reads of a pair are the chunks 4 p + (lane >> 5)
// and 4 p + 2 + (lane >> 5) of its row, which are exactly the MXFP8 kernel's
// reads.  The 8 scale bytes of a row's K-tile are two dwords (pair 0, pair 1),
// staged by two 4-B LDS-DMAs per wave and operand into two 1 KiB planes beside
// the tile.  Two 68 KiB stages.  The MFMAs are the compiler builtin: it places
// the hazard waits and the accumulators.
#include "mx_gemm_core.h"
#include "mx_quantize.h"
#include "mxfp4_format.h"
#include "mx_formats.h"   // struct E2m1, the element format of the shared quantiser kernels

namespace {

using namespace mxk::mx;

// ---------------------------------------------------------------------------
// GEMM
// ---------------------------------------------------------------------------
constexpr int kBK = 256;   // elements per K-tile: 128 B of a row
// two scale dwords (pair 0, pair 1) per row and K-tile, 16 packed bytes per scale byte
using Dma4 = Dma<2, 4>;
constexpr int kStageBytes = 2 * kOpBytes + 4096; // 68 KiB: A pair 0, A pair 1, B pair 0, B pair 1 (1 KiB each)
constexpr int kDmaPerStage = 20;                 // vector-memory ops per wave and stage

// One pair of k-steps: per 32-row block the lane's operand of the first
// (lo) and second (hi) k-step.
struct Frags {
  i32x4_t alo[4], ahi[4], blo[4], bhi[4];
};

// The instruction's 8-dword operand type; with cbsz / blgp = 4 only the first
// 4 dwords are read, the rest stays undefined.
__device__ __forceinline__ i32x8_t widen(i32x4_t v) {
  return __builtin_shufflevector(v, v, 0, 1, 2, 3, -1, -1, -1, -1);
}

// The 32 MFMAs of one pair of k-steps.  sa / sb: per row block the lane's
// scale dword of this pair, already shifted so that byte 0 / 2 is the block
// this lane holds in the pair's first / second k-step.
__device__ __forceinline__ void mfma_pair(f32x16_t (&acc)[4][4], const Frags& f, const int (&sa)[4],
                                          const int (&sb)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(widen(f.blo[j]), widen(f.alo[i]),
                                                                  acc[i][j], 4, 4, 0, sb[j], 0, sa[i]);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(widen(f.bhi[j]), widen(f.ahi[i]),
                                                                  acc[i][j], 4, 4, 2, sb[j], 2, sa[i]);
}

__device__ __forceinline__ void read_frags(Frags& f, const char* stage, int a_base, int b_base,
                                           const FragOff& fo, int p) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const char* b = stage + kOpBytes + b_base + j * 4096;
    f.blo[j] = *reinterpret_cast<const i32x4_t*>(b + fo.lo[p]);
    f.bhi[j] = *reinterpret_cast<const i32x4_t*>(b + fo.hi[p]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const char* a = stage + a_base + i * 4096;
    f.alo[i] = *reinterpret_cast<const i32x4_t*>(a + fo.lo[p]);
    f.ahi[i] = *reinterpret_cast<const i32x4_t*>(a + fo.hi[p]);
  }
}

// The lane's scale dwords of one pair of k-steps, per 32-row block, shifted
// so that byte 0 / 2 is the block this lane holds in the pair's first / second
// k-step.
struct Scales {
  int a[4], b[4];
};

__device__ __forceinline__ void read_scales(Scales& s, const char* stage, int a_row, int b_row,
                                            int shift, int p) {
  const int* pa = reinterpret_cast<const int*>(stage + kScaleOff) + p * 256 + a_row;
  const int* pb = reinterpret_cast<const int*>(stage + kScaleOff + 2048) + p * 256 + b_row;
#pragma unroll
  for (int i = 0; i < 4; ++i) s.a[i] = static_cast<int>(static_cast<uint32_t>(pa[i * 32]) >> shift);
#pragma unroll
  for (int j = 0; j < 4; ++j) s.b[j] = static_cast<int>(static_cast<uint32_t>(pb[j * 32]) >> shift);
}

// K-tile t, read from stage buffer X (Y: the other one).  DMA: stage t+2
// exists and goes out here, at k offset kb2 bytes (every K-tile but the last
// two).  The reads of stage t+1 are unconditional: in the last K-tile they
// fetch stale LDS that nothing uses, which keeps each loop to one body with
// plain loop-carried registers.
// The MFMAs are no memory operations, so the compiler would move them across
// the waits; the sched barriers keep each pair in its phase and interleave it
// with that phase's LDS reads and DMA pieces (masks: 0x008 MFMA, 0x080 DS,
// 0x010 vector memory).
template <bool DMA>
__device__ __forceinline__ void ktile(f32x16_t (&acc)[4][4], Frags& f0, Scales& s0, char* X, char* Y,
                                      const Dma4& dma_a, const Dma4& dma_b, int a_base, int b_base,
                                      int a_row, int b_row, int shift, const FragOff& fo, int kb2,
                                      int wave) {
  Frags f1;
  Scales s1;
  read_scales(s1, X, a_row, b_row, shift, 1);
  read_frags(f1, X, a_base, b_base, fo, 1);
  mfma_pair(acc, f0, s0.a, s0.b);
  // 24 LDS reads (8 scale dwords, 16 fragments) under the 32 MFMAs
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
    __builtin_amdgcn_sched_group_barrier(0x080, 2, 0);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
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
    dma_b.issue(X + kOpBytes, X + kScaleOff + 2048, kb2, wave);
  }
  // pair 0's scale registers are free again: its MFMAs retired before the barrier
  read_scales(s0, Y, a_row, b_row, shift, 0);
  read_frags(f0, Y, a_base, b_base, fo, 0);
  mfma_pair(acc, f1, s1.a, s1.b);
  // 24 LDS reads behind the first 16 MFMAs, the 20 DMA pieces spread over all 32
  if constexpr (DMA) __builtin_amdgcn_sched_group_barrier(0x010, 4, 0);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
    __builtin_amdgcn_sched_group_barrier(0x080, 3, 0);
    if constexpr (DMA) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
    if constexpr (DMA) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
  }
  __builtin_amdgcn_sched_barrier(0);
}

__global__ void __launch_bounds__(kThreads, 1)
mxk_gemm_mxfp4_tn_kernel(const uint8_t* __restrict__ Aq, const uint8_t* __restrict__ As,
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
  const Dma4 dma_a = Dma4::make(Aq, As, lda, ldsa, m0, lane, wave);
  const Dma4 dma_b = Dma4::make(Bq, Bs, ldb, ldsb, n0, lane, wave);
  const int ns = K / kBK;

  const int r32 = lane & 31, h = lane >> 5;
  const int sw = (r32 >> 1) & 7;
  FragOff fo;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    fo.lo[p] = r32 * kRowBytes + (((4 * p + h) ^ sw) << 4);
    fo.hi[p] = r32 * kRowBytes + (((4 * p + 2 + h) ^ sw) << 4);
  }
  const int a_base = wm * 128 * kRowBytes, b_base = wn * 128 * kRowBytes;   // the wave's rows
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
  // and the operands in the VGPR half.
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) asm volatile("" : "+a"(acc[i][j]));

  // stages 0 and 1
  dma_a.issue(smem, smem + kScaleOff, 0, wave);
  dma_b.issue(smem + kOpBytes, smem + kScaleOff + 2048, 0, wave);
  if (ns > 1) {
    dma_a.issue(smem + kStageBytes, smem + kStageBytes + kScaleOff, kRowBytes, wave);
    dma_b.issue(smem + kStageBytes + kOpBytes, smem + kStageBytes + kScaleOff + 2048, kRowBytes, wave);
    mxk::vm_wait_n<kDmaPerStage>();
  } else {
    mxk::vm_wait_n<0>();
  }
  block_barrier();

  Frags f0;
  Scales s0;
  read_frags(f0, smem, a_base, b_base, fo, 0);
  read_scales(s0, smem, a_row, b_row, shift, 0);

  int kb2 = 2 * kRowBytes;
  int t = 0;
#pragma clang loop unroll(disable)
  for (; t + 2 < ns; ++t) {
    char* X = smem + (t & 1) * kStageBytes;
    char* Y = smem + ((t & 1) ^ 1) * kStageBytes;
    ktile<true>(acc, f0, s0, X, Y, dma_a, dma_b, a_base, b_base, a_row, b_row, shift, fo, kb2, wave);
    kb2 += kRowBytes;
  }
  // the last two K-tiles (or the only one): no DMA
#pragma clang loop unroll(disable)
  for (; t < ns; ++t) {
    char* X = smem + (t & 1) * kStageBytes;
    char* Y = smem + ((t & 1) ^ 1) * kStageBytes;
    ktile<false>(acc, f0, s0, X, Y, dma_a, dma_b, a_base, b_base, a_row, b_row, shift, fo, 0, wave);
  }

  // every wave's last fragment reads retired before the slices overwrite the stages
  lds_fence();
  block_barrier();
  store_block32_lds(acc, C, ldc, m0 + wm * 128, n0 + wn * 128, lane,
                    smem + wave * mxk::kStoreLdsWave);
}

}  // namespace

MXK_API int mxk_gemm_mxfp4_tn_is_fast(int M, int N, int K) {
  return gemm_tn_shape_ok(M, N, K, kBK) ? 1 : 0;
}

// The contract is gemm_tn_args_ok's (mx_gemm_core.h), two elements per byte:
// lda / ldb count bytes between packed rows (>= K / 2).
MXK_API int mxk_gemm_mxfp4_tn(const void* Aq, const void* As, const void* Bq, const void* Bs,
                              void* C, int M, int N, int K, int lda, int ldsa, int ldb, int ldsb,
                              int ldc, hipStream_t stream) {
  return launch_gemm_tn<kBK>(mxk_gemm_mxfp4_tn_kernel, Aq, As, Bq, Bs, C, M, N, K, lda, ldsa, ldb, ldsb,
                               ldc, stream);
}

// x: bf16 [R][K] (row stride ldx elements), K % 32 == 0, finite values only.
// q: packed e2m1 [R][K / 2] bytes (row stride ldq bytes), s: E8M0 bytes
// [R][K / 32] (row stride lds).  The definition is in mxfp4_format.h.
MXK_API int mxk_quantize_mxfp4(const void* x, void* q, void* s, long R, int K, long ldx, long ldq,
                               long lds, hipStream_t stream) {
  return launch_quantize_rows<E2m1>(x, q, s, R, K, ldx, ldq, lds, stream);
}

// x: bf16 [R][C] (row stride ldx elements), R % 32 == 0, any C > 0, finite
// values only.  qt: packed e2m1 [C][R / 2] bytes (row stride ldqt bytes), st:
// E8M0 bytes [C][R / 32] (row stride ldst): mxk_quantize_mxfp4 of x^T, bit for
// bit, the MX blocks being 32 consecutive rows of x.  Nothing outside the
// [C][R / 2] and [C][R / 32] extents is written.
MXK_API int mxk_quantize_mxfp4_t(const void* x, void* qt, void* st, long R, long C, long ldx,
                                 long ldqt, long ldst, hipStream_t stream) {
  return launch_quantize_tr<E2m1>(false, x, nullptr, nullptr, qt, st, R, C, ldx, 0, 0, ldqt, ldst, stream);
}

// q / s: the image mxk_quantize_mxfp4 writes ([R][C / 2] and [R][C / 32]; C %
// 32 == 0 as well); qt / st: that of mxk_quantize_mxfp4_t; x is read once.
MXK_API int mxk_quantize_mxfp4_dual(const void* x, void* q, void* s, void* qt, void* st, long R,
                                    long C, long ldx, long ldq, long lds, long ldqt, long ldst,
                                    hipStream_t stream) {
  return launch_quantize_tr<E2m1>(true, x, q, s, qt, st, R, C, ldx, ldq, lds, ldqt, ldst, stream);
}
