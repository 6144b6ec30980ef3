// MXFP4 (OCP MX, e2m1 elements, one E8M0 scale per 32 K elements) quantiser
// and block-scaled MFMA GEMM for gfx950.
//
//   mxk_quantize_mxfp4   bf16 rows -> packed e2m1 nibbles + E8M0 scale bytes
//   mxk_gemm_mxfp4_tn    C[M][N] = dequant(A) . dequant(B)^T, fp32
//                        accumulation, bf16 output; both operands K-contiguous
//
// Storage (mxfp4_format.h has the arithmetic): element 2 i of a row sits in
// bits 3:0 of byte i, element 2 i + 1 in bits 7:4; row strides of the packed
// elements (lda, ldb, ldq) count bytes.
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
// The MXFP8 kernel's (gemm_mxfp8.hip), byte for byte: 256x256 output tile, 4
// waves (2 x 2, 128x128 each = 4 x 4 MFMA blocks), K-tile of 256 elements =
// 128 B per row, the same LDS image (LDS-DMA, 16-B chunks XOR-swizzled by
// (row >> 1) & 7), two stages, one barrier per K-tile.  A K-tile is four MFMA
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
// the hazard waits and the accumulators.  The staging, barrier and store
// helpers repeat those of gemm_mxfp8.hip on purpose: that file's kernels stay
// exactly as they are measured, and the two K loops differ in every phase.
#include "mx_common.h"
#include "mxfp4_format.h"

namespace {

constexpr int kBM = 256, kBN = 256, kBK = 256;
constexpr int kRowBytes = kBK / 2;               // 128 B of a row per K-tile
constexpr int kThreads = 256;
constexpr int kOpBytes = 256 * kRowBytes;        // 32 KiB per operand per stage
constexpr int kScaleOff = 2 * kOpBytes;          // A pair 0, A pair 1, B pair 0, B pair 1 (1 KiB each)
constexpr int kStageBytes = 2 * kOpBytes + 4096; // 68 KiB
constexpr int kDmaPerStage = 20;                 // vector-memory ops per wave and stage

typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void_t;

// ---------------------------------------------------------------------------
// Quantiser
// ---------------------------------------------------------------------------
// 8 consecutive elements of an MX block (4 dwords of two bf16 each, memory
// order) whose other 24 are in the lane's DPP quad: the 8 e2m1 nibbles in
// memory order; returns the block's exponent.  Every lane of the quad must be
// active.
__device__ __forceinline__ int quantize_quarter(const uint32_t (&w)[4], uint32_t& out) {
  float f[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u);
  }
  float amax = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(f[i]));
  // the block's other three lanes: quad_perm [1,0,3,2] then [2,3,0,1]
  amax = fmaxf(amax, __uint_as_float(__builtin_amdgcn_mov_dpp(__float_as_uint(amax), 0xB1, 0xF, 0xF, true)));
  amax = fmaxf(amax, __uint_as_float(__builtin_amdgcn_mov_dpp(__float_as_uint(amax), 0x4E, 0xF, 0xF, true)));
  const int e = mxfp4::block_exp(amax);
  const float inv = mxfp4::block_inv_scale(e);
  out = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float v = fminf(fmaxf(f[i] * inv, -mxfp4::kMax), mxfp4::kMax);   // explicit saturation
    out |= mxfp4::f32_to_e2m1(v) << (4 * i);
  }
  return e;
}

// One lane per 8 consecutive elements (one packed dword), 4 lanes (a DPP quad)
// per MX block.
template <bool VEC>
__global__ void __launch_bounds__(256)
quantize_mxfp4_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ q,
                      uint8_t* __restrict__ s, long R, int K, long ldx, long ldq, long lds) {
  const long per_row = K >> 3;
  const long gid = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  // K % 32 == 0, so a quad never straddles a row and leaves the grid whole
  if (gid >= R * per_row) return;
  const long row = gid / per_row;
  const int c8 = static_cast<int>(gid - row * per_row);
  const uint16_t* xp = x + row * ldx + c8 * 8;
  uint32_t w[4];
  if constexpr (VEC) {
    const uint4 v = *reinterpret_cast<const uint4*>(xp);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = xp[2 * i] | (static_cast<uint32_t>(xp[2 * i + 1]) << 16);
  }
  uint32_t out;
  const int e = quantize_quarter(w, out);
  uint8_t* qp = q + row * ldq + c8 * 4;
  if constexpr (VEC) {
    *reinterpret_cast<uint32_t*>(qp) = out;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) qp[i] = static_cast<uint8_t>(out >> (8 * i));
  }
  if ((c8 & 3) == 0) s[row * lds + (c8 >> 2)] = static_cast<uint8_t>(e + 127);
}

// ---------------------------------------------------------------------------
// GEMM
// ---------------------------------------------------------------------------
// LDS-DMA descriptor of one 256-row operand panel (bytes) and of its scale
// rows.
struct Dma4 {
  __amdgpu_buffer_rsrc_t rsrc;    // 256 rows of ld bytes
  __amdgpu_buffer_rsrc_t srsrc;   // 256 rows of lds scale bytes
  uint32_t voff;                  // row lane >> 3 of a piece, swizzled 16-B chunk
  uint32_t svoff;                 // first scale dword of row 64 wave + lane
  int piece;                      // bytes between pieces (32 rows), scalar
  int wave_off;                   // this wave's 8 rows inside a piece, scalar
  // piece p: rows (4p + wave) 8 .. + 8; the row part rides in the scalar offset.
  // lds_sc: the operand's two scale planes (pair 0, pair 1), 1 KiB each.
  __device__ __forceinline__ void issue(char* lds_op, char* lds_sc, int k_bytes, int wave) const {
#pragma unroll
    for (int p = 0; p < 8; ++p)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void_t*)(lds_op + (p * 4 + wave) * 1024),
                                               16, voff, k_bytes + wave_off + p * piece, 0, 0);
    // k_bytes >> 4: 16 packed bytes per scale byte
    __builtin_amdgcn_raw_ptr_buffer_load_lds(srsrc, (lds_void_t*)(lds_sc + wave * 256), 4, svoff,
                                             k_bytes >> 4, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(srsrc, (lds_void_t*)(lds_sc + 1024 + wave * 256), 4,
                                             svoff, (k_bytes >> 4) + 4, 0, 0);
  }
};

__device__ __forceinline__ Dma4 make_dma4(const uint8_t* q, const uint8_t* sc, int ld, int lds,
                                          int row0, int lane, int wave) {
  Dma4 d;
  d.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(q + static_cast<size_t>(row0) * ld),
                                             0, 256 * ld, 0x00020000);
  d.srsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t*>(sc + static_cast<size_t>(row0) * lds), 0, 256 * lds, 0x00020000);
  const int r = lane >> 3;
  const int c = (lane & 7) ^ ((4 * (wave & 1) + (r >> 1)) & 7);
  d.voff = static_cast<uint32_t>(r * ld + c * 16);
  d.piece = 32 * ld;
  d.wave_off = wave * 8 * ld;
  d.svoff = static_cast<uint32_t>((wave * 64 + lane) * lds);
  return d;
}

// Fragment byte offsets of this lane inside a 32-row block: pair p takes the
// 16-B chunks 4 p + (lane >> 5) (its first k-step) and 4 p + 2 + (lane >> 5)
// (its second) of row lane & 31.
struct FragOff {
  int lo[2], hi[2];
};

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

__device__ __forceinline__ void lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void block_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
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

// bf16 store of a wave's 128x128 block through its LDS slice, two 64-row
// passes with 272-B padded rows, read back row-major so every global store
// covers 4 rows x 256 B (the 32x32 C map: lane = row, register group g =
// columns 8 g + 4 (lane >> 5) .. + 3).
__device__ __forceinline__ void store_block32_lds(const f32x16_t (&acc)[4][4], uint16_t* C, int ldc,
                                                  int row0, int col0, int lane, char* lds) {
  const int r32 = lane & 31, h = lane >> 5;
  const int rr = lane >> 4, cc = (lane & 15) * 8;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x16_t& v = acc[2 * p + ii][j];
          uint2 pk;
          pk.x = mxk::pack2bf(v[4 * g], v[4 * g + 1]);
          pk.y = mxk::pack2bf(v[4 * g + 2], v[4 * g + 3]);
          *reinterpret_cast<uint2*>(lds + (ii * 32 + r32) * mxk::kStoreLdsRow +
                                    (j * 32 + 8 * g + 4 * h) * 2) = pk;
        }
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int r = it * 4 + rr;
      const u32x4_t v = *reinterpret_cast<const u32x4_t*>(lds + r * mxk::kStoreLdsRow + cc * 2);
      uint16_t* cp = C + static_cast<size_t>(row0 + p * 64 + r) * ldc + col0 + cc;
      __builtin_nontemporal_store(v, reinterpret_cast<u32x4_t*>(cp));
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __asm__ volatile("" ::: "memory");
  }
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
  const Dma4 dma_a = make_dma4(Aq, As, lda, ldsa, m0, lane, wave);
  const Dma4 dma_b = make_dma4(Bq, Bs, ldb, ldsb, n0, lane, wave);
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

bool mxfp4_shape_ok(int M, int N, int K) {
  return M > 0 && N > 0 && K > 0 && M % kBM == 0 && N % kBN == 0 && K % kBK == 0;
}

bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

MXK_API int mxk_gemm_mxfp4_tn_is_fast(int M, int N, int K) { return mxfp4_shape_ok(M, N, K) ? 1 : 0; }

// lda / ldb: bytes between packed rows (>= K / 2).  Elements: 16-B aligned
// base, row stride a multiple of 16 B.  Scales: 4-B aligned base, row stride a
// multiple of 4 B (a dword carries the 4 block scales of half a K-tile).  C:
// 16-B aligned, ldc % 8 == 0.  Row strides below 2^23.
MXK_API int mxk_gemm_mxfp4_tn(const void* Aq, const void* As, const void* Bq, const void* Bs,
                              void* C, int M, int N, int K, int lda, int ldsa, int ldb, int ldsb,
                              int ldc, hipStream_t stream) {
  if (!mxfp4_shape_ok(M, N, K) || !Aq || !As || !Bq || !Bs || !C)
    return static_cast<int>(hipErrorInvalidValue);
  constexpr int kMaxLd = 1 << 23;
  if (lda < K / 2 || ldb < K / 2 || ldsa < K / 32 || ldsb < K / 32 || ldc < N || lda >= kMaxLd ||
      ldb >= kMaxLd || ldsa >= kMaxLd || ldsb >= kMaxLd)
    return static_cast<int>(hipErrorInvalidValue);
  if (!aligned(Aq, 16) || !aligned(Bq, 16) || lda % 16 || ldb % 16 || !aligned(As, 4) ||
      !aligned(Bs, 4) || ldsa % 4 || ldsb % 4 || !aligned(C, 16) || ldc % 8)
    return static_cast<int>(hipErrorInvalidValue);
  const int tiles = (M / kBM) * (N / kBN);
  hipLaunchKernelGGL(mxk_gemm_mxfp4_tn_kernel, dim3(tiles), dim3(kThreads), 0, stream,
                     static_cast<const uint8_t*>(Aq), static_cast<const uint8_t*>(As),
                     static_cast<const uint8_t*>(Bq), static_cast<const uint8_t*>(Bs),
                     static_cast<uint16_t*>(C), M, N, K, lda, ldsa, ldb, ldsb, ldc);
  MXK_RETURN_LAUNCH_STATUS();
}

// x: bf16 [R][K] (row stride ldx elements), K % 32 == 0, finite values only.
// q: packed e2m1 [R][K / 2] bytes (row stride ldq bytes), s: E8M0 bytes
// [R][K / 32] (row stride lds).  The definition is in mxfp4_format.h.
MXK_API int mxk_quantize_mxfp4(const void* x, void* q, void* s, long R, int K, long ldx, long ldq,
                               long lds, hipStream_t stream) {
  if (!x || !q || !s || R <= 0 || K <= 0 || K % 32 || ldx < K || ldq < K / 2 || lds < K / 32)
    return static_cast<int>(hipErrorInvalidValue);
  const long lanes = R * (K / 8);
  const long blocks = (lanes + 255) / 256;
  if (blocks > 0x7FFFFFFFL) return static_cast<int>(hipErrorInvalidValue);
  // 16-B loads of x, 4-B stores of q: everything else goes by element
  const bool vec = aligned(x, 16) && ldx % 8 == 0 && aligned(q, 4) && ldq % 4 == 0;
  if (vec)
    hipLaunchKernelGGL(quantize_mxfp4_kernel<true>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0,
                       stream, static_cast<const uint16_t*>(x), static_cast<uint8_t*>(q),
                       static_cast<uint8_t*>(s), R, K, ldx, ldq, lds);
  else
    hipLaunchKernelGGL(quantize_mxfp4_kernel<false>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0,
                       stream, static_cast<const uint16_t*>(x), static_cast<uint8_t*>(q),
                       static_cast<uint8_t*>(s), R, K, ldx, ldq, lds);
  MXK_RETURN_LAUNCH_STATUS();
}
