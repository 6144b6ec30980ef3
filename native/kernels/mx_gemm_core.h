// What the block-scaled (OCP MX) GEMMs share, written once: the staging,
// barrier and epilogue-store helpers and the host side of the entry points.
// gemm_mxfp8.hip (e4m3) and gemm_mxfp4.hip (e2m1) keep their format, their
// kernels and the lane maps of their MFMA operands; the quantisers of both are
// in mx_quantize.h.
//
// Shared tile: 256x256 output, 4 waves (2 x 2, 128x128 each = 4 x 4 MFMA
// blocks of 32x32), K-tile rows of 128 B whatever the element width, LDS image
// of gemm_tn_core.h (LDS-DMA, 16-B chunks XOR-swizzled by (row >> 1) & 7), two
// stages, one barrier per K-tile.  A row's E8M0 scale bytes of a K-tile are
// PLANES dwords (4 scales each), staged as PLANES 1 KiB planes per operand
// behind the two operand panels: A planes, then B planes.
//
// hipcc optimises a __device__ function before it inlines it, so moving code
// across a function boundary can move instructions: scripts/isa_stream.py
// compares the streams.  With what is here, every kernel of the two files has
// the instruction stream it had with its own copy of each helper.  The two GEMM
// kernel bodies (prologue, K loops, epilogue) stay in the formats' files: as
// one function called from both files they compile to other streams
// (profiles/mx_gemm_core/).  A kernel template does not have that problem,
// each instantiation being the code a copy would be: the quantiser kernels are
// written that way (mx_quantize.h, profiles/mx_quantize/).
#pragma once
#include "mx_common.h"

typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void_t;

namespace mxk {
namespace mx {

constexpr int kBM = 256, kBN = 256;
constexpr int kRowBytes = 128;                   // of a row per K-tile
constexpr int kThreads = 256;
constexpr int kOpBytes = 256 * kRowBytes;        // 32 KiB per operand per stage
constexpr int kScaleOff = 2 * kOpBytes;          // the scale planes (1 KiB each)

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// ---------------------------------------------------------------------------
// GEMM helpers
// ---------------------------------------------------------------------------
// LDS-DMA descriptor of one 256-row operand panel (bytes; gemm_tn_core.h DmaK
// for 1-byte elements) and of its scale rows.  PLANES: scale dwords per row and
// K-tile; KSHIFT: K byte offset -> scale byte offset (32 e4m3 or 16 packed
// e2m1 bytes per scale byte).
template <int PLANES, int KSHIFT>
struct Dma {
  __amdgpu_buffer_rsrc_t rsrc;    // 256 rows of ld bytes
  __amdgpu_buffer_rsrc_t srsrc;   // 256 rows of lds scale bytes
  uint32_t voff;                  // row lane >> 3 of a piece, swizzled 16-B chunk
  uint32_t svoff;                 // first scale dword of row 64 wave + lane
  int piece;                      // bytes between pieces (32 rows), scalar
  int wave_off;                   // this wave's 8 rows inside a piece, scalar
  // piece p: rows (4p + wave) 8 .. + 8; the row part rides in the scalar offset.
  // lds_sc: the operand's scale planes.  The second plane is a second call, not
  // a loop over PLANES: the loop form schedules differently.
  __device__ __forceinline__ void issue(char* lds_op, char* lds_sc, int k_bytes, int wave) const {
#pragma unroll
    for (int p = 0; p < 8; ++p)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void_t*)(lds_op + (p * 4 + wave) * 1024),
                                               16, voff, k_bytes + wave_off + p * piece, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(srsrc, (lds_void_t*)(lds_sc + wave * 256), 4, svoff,
                                             k_bytes >> KSHIFT, 0, 0);
    if constexpr (PLANES == 2)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(srsrc, (lds_void_t*)(lds_sc + 1024 + wave * 256), 4,
                                               svoff, (k_bytes >> KSHIFT) + 4, 0, 0);
  }

  __device__ __forceinline__ static Dma make(const uint8_t* q, const uint8_t* sc, int ld, int lds,
                                             int row0, int lane, int wave) {
    Dma d;
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
};

// Fragment byte offsets of this lane inside a 32-row block: half p of the
// K-tile takes the 16-B chunks 4 p + (lane >> 5) (lo) and 4 p + 2 + (lane >> 5)
// (hi) of row lane & 31.  The kernels fill it inline.
struct FragOff {
  int lo[2], hi[2];
};

__device__ __forceinline__ void lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void block_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// bf16 store of a wave's 128x128 block through its LDS slice, two 64-row
// passes with 272-B padded rows, read back row-major so every global store
// covers 4 rows x 256 B (mx_common.h store_block_lds for the 32x32 C map:
// lane = row, register group g = columns 8 g + 4 (lane >> 5) .. + 3).
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
          pk.x = pack2bf(v[4 * g], v[4 * g + 1]);
          pk.y = pack2bf(v[4 * g + 2], v[4 * g + 3]);
          *reinterpret_cast<uint2*>(lds + (ii * 32 + r32) * kStoreLdsRow +
                                    (j * 32 + 8 * g + 4 * h) * 2) = pk;
        }
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int r = it * 4 + rr;
      const u32x4_t v = *reinterpret_cast<const u32x4_t*>(lds + r * kStoreLdsRow + cc * 2);
      uint16_t* cp = C + static_cast<size_t>(row0 + p * 64 + r) * ldc + col0 + cc;
      __builtin_nontemporal_store(v, reinterpret_cast<u32x4_t*>(cp));
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __asm__ volatile("" ::: "memory");
  }
}

inline bool gemm_tn_shape_ok(int M, int N, int K, int bk) {
  return M > 0 && N > 0 && K > 0 && M % kBM == 0 && N % kBN == 0 && K % bk == 0;
}

// What both mxk_gemm_mx*_tn entry points require.  Elements (per_byte of them
// in a byte; lda / ldb count bytes): 16-B aligned base, row stride a multiple
// of 16 B.  Scales: 4-B aligned base, row stride a multiple of 4 B (a dword
// carries 4 block scales).  C: 16-B aligned, ldc % 8 == 0.  Row strides below
// 2^23.
inline bool gemm_tn_args_ok(const void* Aq, const void* As, const void* Bq, const void* Bs,
                            const void* C, int M, int N, int K, int lda, int ldsa, int ldb, int ldsb,
                            int ldc, int bk, int per_byte) {
  if (!gemm_tn_shape_ok(M, N, K, bk) || !Aq || !As || !Bq || !Bs || !C) return false;
  constexpr int kMaxLd = 1 << 23;
  if (lda < K / per_byte || ldb < K / per_byte || ldsa < K / 32 || ldsb < K / 32 || ldc < N ||
      lda >= kMaxLd || ldb >= kMaxLd || ldsa >= kMaxLd || ldsb >= kMaxLd)
    return false;
  return aligned(Aq, 16) && aligned(Bq, 16) && lda % 16 == 0 && ldb % 16 == 0 && aligned(As, 4) &&
         aligned(Bs, 4) && ldsa % 4 == 0 && ldsb % 4 == 0 && aligned(C, 16) && ldc % 8 == 0;
}

// Host side of mxk_gemm_mx*_tn: hipErrorInvalidValue with nothing launched
// unless gemm_tn_args_ok, else the kernel on one workgroup per tile.  BK:
// elements per K-tile (128 B of a row).
using GemmTnKernel = void (*)(const uint8_t*, const uint8_t*, const uint8_t*, const uint8_t*, uint16_t*,
                              int, int, int, int, int, int, int, int);
template <int BK>
int launch_gemm_tn(GemmTnKernel kernel, const void* Aq, const void* As, const void* Bq, const void* Bs,
                   void* C, int M, int N, int K, int lda, int ldsa, int ldb, int ldsb, int ldc,
                   hipStream_t stream) {
  if (!gemm_tn_args_ok(Aq, As, Bq, Bs, C, M, N, K, lda, ldsa, ldb, ldsb, ldc, BK, BK / kRowBytes))
    return static_cast<int>(hipErrorInvalidValue);
  const int tiles = (M / kBM) * (N / kBN);
  hipLaunchKernelGGL(kernel, dim3(tiles), dim3(kThreads), 0, stream, static_cast<const uint8_t*>(Aq),
                     static_cast<const uint8_t*>(As), static_cast<const uint8_t*>(Bq),
                     static_cast<const uint8_t*>(Bs), static_cast<uint16_t*>(C), M, N, K, lda, ldsa,
                     ldb, ldsb, ldc);
  MXK_RETURN_LAUNCH_STATUS();
}

}  // namespace mx
}  // namespace mxk
