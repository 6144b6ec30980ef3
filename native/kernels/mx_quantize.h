// The block-scaled (OCP MX) quantisers, written once for both element formats:
// the quarter-block routine, the row and the transposing kernel, and the host
// sides of the entry points.  gemm_mxfp8.hip (struct E4m3) and gemm_mxfp4.hip
// (struct E2m1) keep their format and their entry points.
//
// Fmt: kBits per element, kMax (saturation bound), block_exp(amax),
// inv_scale(e) = 2^-e, convert(v) = the element's code.  A lane quantises 8
// consecutive elements, so everything that differs between the formats follows
// from kBits: the lane's codes are kBits / 4 dwords = kBits bytes, stored at
// byte (element index) >> (kBits == 4) of a row with one kBits-byte store where
// the image is that aligned and byte by byte where it is not; ldq and ldqt
// count bytes.
//
// The kernels are templates, not functions that a kernel of either file calls:
// hipcc optimises a __device__ function before it inlines it, so a kernel body
// moved into a function compiles to another instruction stream
// (profiles/mx_gemm_core/), while every instantiation of a kernel template is
// the code its hand-written copy was (profiles/mx_quantize/).
//
// Rounding is a policy of the format struct.  A stochastic format (E2m1Sr of
// quantize_mxfp4_sr.hip) is launched with one more argument, a uint64_t seed,
// which every kernel and launcher below takes as the pack Seed...:
// empty for the nearest-rounding formats, whose kernels keep their parameter
// lists and instruction streams (profiles/mxfp4_sr/isa_diff.txt), and for them
// quantize_quarter discards the stochastic branch.  A stochastic format has
//   block_exp(amax)       its own (non-clipping) block exponent,
//   random(SrLane, r)     the 4 random words of elements 8 g .. 8 g + 7 of row i
//                         of the OUTPUT image (8 x 16 bits, element j takes
//                         r[j >> 1] >> 16 (j & 1)),
//   convert(v, u16)       the element's code from the scaled value and its bits,
// so an image depends on (seed, element) alone and the transposing kernel's
// image is the row kernel's of the transposed copy.
#pragma once
#include "mx_gemm_core.h"

namespace mxk {
namespace mx {

// The stochastic arguments of quantize_quarter for the lane that converts
// elements 8 g .. 8 g + 7 of row i of the output image; both indices are below
// 2^32 (the launchers' gate), so they are the two counter words.
constexpr long kSrMaxIndex = 0xFFFFFFFFL;
struct SrLane {
  uint32_t g, i;
  uint64_t seed;
};
__device__ __forceinline__ SrLane sr_lane(long g, long i, uint64_t seed) {
  return SrLane{static_cast<uint32_t>(g), static_cast<uint32_t>(i), seed};
}

// 8 consecutive elements of an MX block (4 dwords of two bf16 each, memory
// order) whose other 24 are in the lane's DPP quad: the 8 codes packed in
// memory order; returns the block's exponent.  Every lane of the quad must be
// active.
// sr (stochastic formats only): the SrLane of these 8 elements.
template <class Fmt, class... Sr>
__device__ __forceinline__ int quantize_quarter(const uint32_t (&w)[4],
                                                uint32_t (&out)[Fmt::kBits / 4], Sr... sr) {
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
  const int e = Fmt::block_exp(amax);
  const float inv = Fmt::inv_scale(e);
#pragma unroll
  for (int i = 0; i < Fmt::kBits / 4; ++i) out[i] = 0;
  if constexpr (sizeof...(Sr) != 0) {
    uint32_t r[4];
    Fmt::random(sr..., r);
#pragma unroll
    for (int i = 0; i < 8; ++i)   // |f[i] * inv| <= kMax: the exponent does not clip
      out[i * Fmt::kBits / 32] |= Fmt::convert(f[i] * inv, (r[i >> 1] >> (16 * (i & 1))) & 0xFFFFu)
                                  << (i * Fmt::kBits % 32);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float v = fminf(fmaxf(f[i] * inv, -Fmt::kMax), Fmt::kMax);   // explicit saturation
      out[i * Fmt::kBits / 32] |= Fmt::convert(v) << (i * Fmt::kBits % 32);
    }
  }
  return e;
}

// The packed codes of quantize_quarter to an aligned qp: one 8-B (e4m3) or 4-B
// (e2m1) store.  The by-byte form for an unaligned qp,
//   for (i < Fmt::kBits) qp[i] = out[i >> 2] >> (8 * (i & 3)),
// stays inline in the kernels: as a helper it changes the by-element streams.
template <class Fmt>
__device__ __forceinline__ void store_quarter(uint8_t* qp, const uint32_t (&out)[Fmt::kBits / 4]) {
  if constexpr (Fmt::kBits == 8) *reinterpret_cast<uint2*>(qp) = make_uint2(out[0], out[1]);
  else *reinterpret_cast<uint32_t*>(qp) = out[0];
}

// ---- row quantiser ------------------------------------------------------------
// One lane per 8 consecutive elements, 4 lanes (a DPP quad) per MX block.
template <class Fmt, bool VEC, class... Seed>
__global__ void __launch_bounds__(256)
quantize_rows_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ q,
                     uint8_t* __restrict__ s, long R, int K, long ldx, long ldq, long lds,
                     Seed... seed) {
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
  uint32_t out[Fmt::kBits / 4];
  const int e = quantize_quarter<Fmt>(w, out, sr_lane(c8, row, seed)...);
  uint8_t* qp = q + row * ldq + c8 * Fmt::kBits;
  if constexpr (VEC) {
    store_quarter<Fmt>(qp, out);
  } else {
#pragma unroll
    for (int i = 0; i < Fmt::kBits; ++i) qp[i] = static_cast<uint8_t>(out[i >> 2] >> (8 * (i & 3)));
  }
  if ((c8 & 3) == 0) s[row * lds + (c8 >> 2)] = static_cast<uint8_t>(e + 127);
}

// Host side of a row quantiser: x bf16 [R][K] (row stride ldx elements), K %
// 32 == 0; q packed codes (row stride ldq bytes); s E8M0 bytes [R][K / 32].
// The row kernel with 16-B loads and one packed store per lane, or going by
// element.
template <class Fmt, class... Seed>
int launch_quantize_rows(const void* x, void* q, void* s, long R, int K, long ldx, long ldq, long lds,
                         hipStream_t stream, Seed... seed) {
  if (!x || !q || !s || R <= 0 || K <= 0 || K % 32 || ldx < K || ldq < K * Fmt::kBits / 8 ||
      lds < K / 32)
    return static_cast<int>(hipErrorInvalidValue);
  if (sizeof...(Seed) != 0 && R > kSrMaxIndex) return static_cast<int>(hipErrorInvalidValue);
  const long lanes = R * (K / 8);
  const long blocks = (lanes + 255) / 256;
  if (blocks > 0x7FFFFFFFL) return static_cast<int>(hipErrorInvalidValue);
  // 16-B loads of x, kBits-byte stores of q: everything else goes by element
  const bool vec = aligned(x, 16) && ldx % 8 == 0 && aligned(q, Fmt::kBits) && ldq % Fmt::kBits == 0;
  const auto kernel = vec ? quantize_rows_kernel<Fmt, true, Seed...> : quantize_rows_kernel<Fmt, false, Seed...>;
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream,
                     static_cast<const uint16_t*>(x), static_cast<uint8_t*>(q),
                     static_cast<uint8_t*>(s), R, K, ldx, ldq, lds, seed...);
  MXK_RETURN_LAUNCH_STATUS();
}

// ---- transposing quantiser ----------------------------------------------------
// qt[c][r], st[c][r / 32]: the images of x^T that the backward products of a
// linear layer contract over, without a transposed copy of x; the MX blocks
// are 32 consecutive ROWS of x.  A workgroup takes a kTrRows-row x 64-column
// tile of x (kTrRows = 128):
//   load   lane = (row pair, 8-column chunk): two 16-B row accesses (rows r and
//          r + 1), per wave instruction 8 row pairs x 128 B.  DUAL: the two
//          rows are also quantised along the row (the chunks of a 32-column
//          block sit in one DPP quad) and stored, 8 B (e4m3) or 4 B (e2m1) per
//          lane, the image of quantize_rows_kernel.
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
//          the 8 codes are kBits contiguous bytes of qt per lane: 16 lanes
//          write the 128 B (e4m3) or 64 B (e2m1: a wave instruction 4 such
//          runs) a column has in the tile.
// Rows >= R and columns >= C of a ragged tile load zeros and store nothing.
//
// Measured for e2m1 (profiles/mxfp4_linear/): 0.059 / 0.179 / 0.054 ms at
// [16384, 4096] / [16384, 14336] / [14336, 4096], 1.08-1.21x the time of the
// e4m3 instantiation although half the bytes go out.  The 4-B stores are not
// what costs: with 256 rows per tile (-DMXK_MX_TR_ROWS=256, then named
// MXK_MXFP4_TR_ROWS: 128 B per column, 33 KiB of LDS) the same calls take
// 0.064 / 0.189 / 0.059 ms, 6-8 % more.  The kernel is bound by vector ALU
// work: it is straight-line code of 954 VALU instructions per lane and tile
// against e4m3's 710 (271 against 47 of them v_cmp, the seven threshold
// compares per element of mxfp4::f32_to_e2m1), and 4 waves x 954 issue cycles
// x 32 tiles per CU are 51 us of the 59 at [16384, 4096].
//
// The stochastic e2m1 instantiation (quantize_mxfp4_sr.hip; profiles/mxfp4_sr/):
// 1783 VALU instructions per lane and tile (dual: 3425 against 1769), 467 of
// them v_cmp and 103 (against 36) the 32-bit multiplies that the four Philox
// calls add (v_mul_lo / v_mul_hi_u32, v_mad_u64_u32); the wave-uniform key
// schedule runs on the scalar unit (408 scalar instructions against 86);
// measured 0.093 / 0.281 / 0.083 ms at
// the three shapes, 1.50-1.53x the nearest form of the same run (dual 0.165 /
// 0.522 / 0.147 ms, 1.61-1.68x), less than the static ratio of 1.87 (1.94).
#ifndef MXK_MX_TR_ROWS
#define MXK_MX_TR_ROWS 128   // 256 measured 6-8 % slower for e2m1 (above); e4m3 not measured
#endif
constexpr int kTrRows = MXK_MX_TR_ROWS, kTrCols = 64;
static_assert(kTrRows == 128 || kTrRows == 256, "row passes of 64, 16 or 32 lanes per column");
constexpr int kTrLdsRow = kTrRows * 2 + 8;   // bytes
constexpr int kTrLanesPerCol = kTrRows / 8;  // lanes that share a column in the store phase
constexpr int kTrColsPerPass = 256 / kTrLanesPerCol;

template <class Fmt, bool VEC, bool DUAL, class... Seed>
__global__ void __launch_bounds__(256)
quantize_tr_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ q, uint8_t* __restrict__ s,
                   uint8_t* __restrict__ qt, uint8_t* __restrict__ st, long R, long C, long ldx,
                   long ldq, long lds, long ldqt, long ldst, Seed... seed) {
  constexpr int kPack = Fmt::kBits == 4;   // element index >> kPack = byte of a row
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
        uint32_t out[Fmt::kBits / 4];
        const int e = quantize_quarter<Fmt>(w[h], out, sr_lane(col >> 3, row, seed)...);
        if (row < R && col < C) {   // C % 32 == 0: whole blocks
          uint8_t* qp = q + row * ldq + (col >> kPack);
          if constexpr (VEC) {
            store_quarter<Fmt>(qp, out);
          } else {
#pragma unroll
            for (int i = 0; i < Fmt::kBits; ++i) qp[i] = static_cast<uint8_t>(out[i >> 2] >> (8 * (i & 3)));
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
    uint32_t out[Fmt::kBits / 4];
    // stochastic: the transposed image of a dual call draws with seed + 1
    const int e = quantize_quarter<Fmt>(w, out, sr_lane(row >> 3, c0 + cl, seed + (DUAL ? 1u : 0u))...);
    const long c = c0 + cl;
    if (row < R && c < C) {   // R % 32 == 0: whole blocks
      uint8_t* qp = qt + c * ldqt + (row >> kPack);
      if constexpr (VEC) {
        store_quarter<Fmt>(qp, out);
      } else {
#pragma unroll
        for (int i = 0; i < Fmt::kBits; ++i) qp[i] = static_cast<uint8_t>(out[i >> 2] >> (8 * (i & 3)));
      }
      if ((r8 & 3) == 0) st[c * ldst + (row >> 5)] = static_cast<uint8_t>(e + 127);
    }
  }
}

// Host side of the transposing entry points: x bf16 [R][C] (row stride ldx
// elements), R % 32 == 0; qt packed codes, R kBits / 8 bytes a row (row stride
// ldqt bytes), st
// E8M0 bytes [C][R / 32].  dual: also q / s, the image of launch_quantize_rows
// (C % 32 == 0 as well).
template <class Fmt, class... Seed>
int launch_quantize_tr(bool dual, const void* x, void* q, void* s, void* qt, void* st, long R, long C,
                       long ldx, long ldq, long lds, long ldqt, long ldst, hipStream_t stream,
                       Seed... seed) {
  constexpr int kB = Fmt::kBits;
  if (!x || !qt || !st || R <= 0 || C <= 0 || R % 32 || ldx < C || ldqt < R / (8 / kB) || ldst < R / 32)
    return static_cast<int>(hipErrorInvalidValue);
  if (dual && (!q || !s || C % 32 || ldq < C / (8 / kB) || lds < C / 32))
    return static_cast<int>(hipErrorInvalidValue);
  if (sizeof...(Seed) != 0 && (R > kSrMaxIndex || C > kSrMaxIndex))
    return static_cast<int>(hipErrorInvalidValue);
  const long gx = (R + kTrRows - 1) / kTrRows, gy = (C + kTrCols - 1) / kTrCols;
  if (gx > 0x7FFFFFFFL || gy > 65535) return static_cast<int>(hipErrorInvalidValue);
  // 16-B row accesses of x, kBits-byte stores of qt (and q): everything else goes by element and byte
  const bool vec = aligned(x, 16) && ldx % 8 == 0 && C % 8 == 0 && aligned(qt, kB) && ldqt % kB == 0 &&
                   (!dual || (aligned(q, kB) && ldq % kB == 0));
  const dim3 grid(static_cast<unsigned>(gx), static_cast<unsigned>(gy));
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, static_cast<const uint16_t*>(x),
                       static_cast<uint8_t*>(q), static_cast<uint8_t*>(s), static_cast<uint8_t*>(qt),
                       static_cast<uint8_t*>(st), R, C, ldx, ldq, lds, ldqt, ldst, seed...);
  };
  if (dual) {
    if (vec) go(quantize_tr_kernel<Fmt, true, true, Seed...>);
    else go(quantize_tr_kernel<Fmt, false, true, Seed...>);
  } else {
    if (vec) go(quantize_tr_kernel<Fmt, true, false, Seed...>);
    else go(quantize_tr_kernel<Fmt, false, false, Seed...>);
  }
  MXK_RETURN_LAUNCH_STATUS();
}

}  // namespace mx
}  // namespace mxk
