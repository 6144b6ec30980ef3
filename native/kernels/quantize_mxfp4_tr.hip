// Transposing MXFP4 (OCP MX, e2m1 elements, one E8M0 scale per 32 elements)
// quantisers for gfx950: the images of x^T that the backward products of a
// linear layer contract over, without a transposed copy of x.
//
//   mxk_quantize_mxfp4_t     mxk_quantize_mxfp4 (gemm_mxfp4.hip) of x^T: the MX
//                            blocks are 32 consecutive ROWS of x, stored transposed
//   mxk_quantize_mxfp4_dual  that and the row image of mxk_quantize_mxfp4 from
//                            one read of x
//
// Storage (mxfp4_format.h has the arithmetic): byte i of row c of qt holds
// x[2 i][c] in bits 3:0 and x[2 i + 1][c] in bits 7:4; ldqt and ldq count bytes.
//
// The structure is that of quantize_mxfp8_tr_kernel (gemm_mxfp8.hip).  A
// workgroup takes a kTrRows-row x 64-column tile of x (kTrRows = 128):
//   load   lane = (row pair, 8-column chunk): two 16-B row accesses (rows r and
//          r + 1), per wave instruction 8 row pairs x 128 B.  DUAL: the two
//          rows are also quantised along the row (the chunks of a 32-column
//          block sit in one DPP quad) and stored, 4 B per lane, the image of
//          quantize_mxfp4_kernel.
//   LDS    transposed image T[c][r] of bf16: x[r][c], x[r + 1][c] go out as one
//          dword (4-B stores, which hipcc pairs into ds_write2_b32; either way
//          served per dword in two groups of 32 lanes, bank = dword address
//          mod 32).  A T row is 2 kTrRows B + 8 B of padding: 66 dwords,
//          and 8 T rows, the distance between two chunks, 528 = 16 (mod 32).  A
//          32-lane store group holds chunks k = 0..3 (or 4..7) of 8 row pairs,
//          T row 8 k + j in its j-th store: bank 16 (k & 1) + 2 j + pair
//          (mod 32), so chunks k and k + 2 meet, 2-way, which a 4-B LDS store
//          hides (its cycles are set by the register transfer, not the
//          array).  Unpadded (64 dwords) all 4 chunks of a group would meet on
//          one bank per row pair, 4-way.  The same holds for a 256-row tile:
//          130 dwords per T row, 8 rows 1040 = 16 (mod 32).
//          A column read is the lane's 8 rows, 16 B at an address that is 8-B
//          but not 16-B aligned in odd T rows (66 c dwords), so it is one
//          ds_read2_b64, not a ds_read_b128: each of its two accesses goes in
//          groups of 16 contiguous lanes, which here are exactly the 16 lanes
//          of one T row, 8 B each at a stride of 16 B over 256 contiguous
//          bytes; banks (mod 32) 4 r8 and 4 r8 + 1, so lanes r8 and r8 + 8
//          meet, 2-way, whatever the padding.  Making a T row a multiple of 16 B
//          for a ds_read_b128 would need 68 dwords, where 8 T rows are 544 =
//          0 (mod 32) and the stores go 4-way; the read side is 4 instructions
//          per lane against 16 stored dwords, so the stores decide.
//   store  lane = (column, 8 rows): amax over the quad that shares the block,
//          the 8 codes are one dword, 4 contiguous bytes of qt per lane: 16
//          lanes write the 64 contiguous bytes a column has in the tile, a wave
//          instruction 4 such runs (MXFP8: 8 B per lane, 128 B per column).
// Rows >= R and columns >= C of a ragged tile load zeros and store nothing.
//
// Measured (profiles/mxfp4_linear/): 0.059 / 0.179 / 0.054 ms at [16384, 4096] /
// [16384, 14336] / [14336, 4096], 1.08-1.21x the time of quantize_mxfp8_t
// although half the bytes go out.  The 4-B stores are not what costs: with 256
// rows per tile (-DMXK_MXFP4_TR_ROWS=256: 128 B per column, 33 KiB of LDS) the
// same calls take 0.064 / 0.189 / 0.059 ms, 6-8 % more.  The kernel is bound by
// vector ALU work: it is straight-line code of 954 VALU instructions per lane
// and tile against the MXFP8 kernel's 710 (271 against 47 of them v_cmp, the
// seven threshold compares per element of mxfp4::f32_to_e2m1), and 4 waves x
// 954 issue cycles x 32 tiles per CU are 51 us of the 59 at [16384, 4096].
#include "mx_gemm_core.h"
#include "mxfp4_format.h"

namespace {

using namespace mxk::mx;

// The element format of the shared quantiser (mx_gemm_core.h), as in
// gemm_mxfp4.hip: one packed dword per lane.
struct E2m1 {
  static constexpr int kBits = 4;
  static constexpr float kMax = mxfp4::kMax;
  __device__ static int block_exp(float amax) { return mxfp4::block_exp(amax); }
  __device__ static float inv_scale(int e) { return mxfp4::block_inv_scale(e); }
  __device__ static uint32_t convert(float v) { return mxfp4::f32_to_e2m1(v); }
};

#ifndef MXK_MXFP4_TR_ROWS
#define MXK_MXFP4_TR_ROWS 128   // 256 measured 6-8 % slower (above)
#endif
constexpr int kTrRows = MXK_MXFP4_TR_ROWS, kTrCols = 64;
static_assert(kTrRows == 128 || kTrRows == 256, "row passes of 64, 16 or 32 lanes per column");
constexpr int kTrLdsRow = kTrRows * 2 + 8;   // bytes
constexpr int kTrLanesPerCol = kTrRows / 8;  // lanes that share a column in the store phase
constexpr int kTrColsPerPass = 256 / kTrLanesPerCol;

template <bool VEC, bool DUAL>
__global__ void __launch_bounds__(256)
quantize_mxfp4_tr_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ q,
                         uint8_t* __restrict__ s, uint8_t* __restrict__ qt, uint8_t* __restrict__ st,
                         long R, long C, long ldx, long ldq, long lds, long ldqt, long ldst) {
  __shared__ __attribute__((aligned(8))) char tile[kTrCols * kTrLdsRow];
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const long r0 = static_cast<long>(blockIdx.x) * kTrRows;
  const long c0 = static_cast<long>(blockIdx.y) * kTrCols;
  const int k = (lane & 3) | ((lane >> 5) << 2);   // 8-column chunk
  const int pair = (lane >> 2) & 7;
  const long col = c0 + k * 8;
#pragma unroll
  for (int pass = 0; pass < kTrRows / 64; ++pass) {
    const int rl = pass * 64 + wave * 16 + pair * 2;   // even row inside the tile
    uint32_t w[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long row = r0 + rl + h;
      const uint16_t* xp = x + row * ldx + col;
      if constexpr (VEC) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (row < R && col < C) v = *reinterpret_cast<const uint4*>(xp);   // C % 8 == 0
        w[h][0] = v.x; w[h][1] = v.y; w[h][2] = v.z; w[h][3] = v.w;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint32_t lo = (row < R && col + 2 * i < C) ? xp[2 * i] : 0u;
          const uint32_t hi = (row < R && col + 2 * i + 1 < C) ? xp[2 * i + 1] : 0u;
          w[h][i] = lo | (hi << 16);
        }
      }
      if constexpr (DUAL) {
        uint32_t out[1];
        const int e = quantize_quarter<E2m1>(w[h], out);
        if (row < R && col < C) {   // C % 32 == 0: whole blocks
          uint8_t* qp = q + row * ldq + (col >> 1);
          if constexpr (VEC) {
            store_quarter<E2m1>(qp, out);
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) qp[i] = static_cast<uint8_t>(out[0] >> (8 * i));
          }
          if ((k & 3) == 0) s[row * lds + (col >> 5)] = static_cast<uint8_t>(e + 127);
        }
      }
    }
    char* tp = tile + (k * 8) * kTrLdsRow + rl * 2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<uint32_t*>(tp + (2 * i) * kTrLdsRow) = (w[0][i] & 0xFFFFu) | (w[1][i] << 16);
      *reinterpret_cast<uint32_t*>(tp + (2 * i + 1) * kTrLdsRow) =
          (w[0][i] >> 16) | (w[1][i] & 0xFFFF0000u);
    }
  }
  __syncthreads();
  const int r8 = t & (kTrLanesPerCol - 1);
  const long row = r0 + r8 * 8;
#pragma unroll
  for (int pass = 0; pass < kTrCols / kTrColsPerPass; ++pass) {
    const int cl = pass * kTrColsPerPass + t / kTrLanesPerCol;
    const char* tp = tile + cl * kTrLdsRow + r8 * 16;
    const uint2 a = *reinterpret_cast<const uint2*>(tp);
    const uint2 b = *reinterpret_cast<const uint2*>(tp + 8);
    const uint32_t w[4] = {a.x, a.y, b.x, b.y};
    uint32_t out[1];
    const int e = quantize_quarter<E2m1>(w, out);
    const long c = c0 + cl;
    if (row < R && c < C) {   // R % 32 == 0: whole blocks
      uint8_t* qp = qt + c * ldqt + (row >> 1);
      if constexpr (VEC) {
        store_quarter<E2m1>(qp, out);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) qp[i] = static_cast<uint8_t>(out[0] >> (8 * i));
      }
      if ((r8 & 3) == 0) st[c * ldst + (row >> 5)] = static_cast<uint8_t>(e + 127);
    }
  }
}

int launch_quantize_tr(bool dual, const void* x, void* q, void* s, void* qt, void* st, long R, long C,
                       long ldx, long ldq, long lds, long ldqt, long ldst, hipStream_t stream) {
  if (!x || !qt || !st || R <= 0 || C <= 0 || R % 32 || ldx < C || ldqt < R / 2 || ldst < R / 32)
    return static_cast<int>(hipErrorInvalidValue);
  if (dual && (!q || !s || C % 32 || ldq < C / 2 || lds < C / 32))
    return static_cast<int>(hipErrorInvalidValue);
  const long gx = (R + kTrRows - 1) / kTrRows, gy = (C + kTrCols - 1) / kTrCols;
  if (gx > 0x7FFFFFFFL || gy > 65535) return static_cast<int>(hipErrorInvalidValue);
  // 16-B row accesses of x, 4-B stores of qt (and q): everything else goes by element and byte
  const bool vec = aligned(x, 16) && ldx % 8 == 0 && C % 8 == 0 && aligned(qt, 4) && ldqt % 4 == 0 &&
                   (!dual || (aligned(q, 4) && ldq % 4 == 0));
  const dim3 grid(static_cast<unsigned>(gx), static_cast<unsigned>(gy));
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, static_cast<const uint16_t*>(x),
                       static_cast<uint8_t*>(q), static_cast<uint8_t*>(s), static_cast<uint8_t*>(qt),
                       static_cast<uint8_t*>(st), R, C, ldx, ldq, lds, ldqt, ldst);
  };
  if (dual) {
    if (vec) go(quantize_mxfp4_tr_kernel<true, true>);
    else go(quantize_mxfp4_tr_kernel<false, true>);
  } else {
    if (vec) go(quantize_mxfp4_tr_kernel<true, false>);
    else go(quantize_mxfp4_tr_kernel<false, false>);
  }
  MXK_RETURN_LAUNCH_STATUS();
}

}  // namespace

// x: bf16 [R][C] (row stride ldx elements), R % 32 == 0, any C > 0, finite
// values only.  qt: packed e2m1 [C][R / 2] bytes (row stride ldqt bytes), st:
// E8M0 bytes [C][R / 32] (row stride ldst): mxk_quantize_mxfp4 of x^T, bit for
// bit, the MX blocks being 32 consecutive rows of x.  Nothing outside the
// [C][R / 2] and [C][R / 32] extents is written.
MXK_API int mxk_quantize_mxfp4_t(const void* x, void* qt, void* st, long R, long C, long ldx,
                                 long ldqt, long ldst, hipStream_t stream) {
  return launch_quantize_tr(false, x, nullptr, nullptr, qt, st, R, C, ldx, 0, 0, ldqt, ldst, stream);
}

// q / s: the image mxk_quantize_mxfp4 writes ([R][C / 2] and [R][C / 32]; C %
// 32 == 0 as well); qt / st: that of mxk_quantize_mxfp4_t; x is read once.
MXK_API int mxk_quantize_mxfp4_dual(const void* x, void* q, void* s, void* qt, void* st, long R,
                                    long C, long ldx, long ldq, long lds, long ldqt, long ldst,
                                    hipStream_t stream) {
  return launch_quantize_tr(true, x, q, s, qt, st, R, C, ldx, ldq, lds, ldqt, ldst, stream);
}
