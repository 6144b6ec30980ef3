// SwiGLU computed inside the block-scaled quantisers, for the MLP of the MX
// training routes (mxk8s.ops.linear.swiglu_mlp_mx): between the two MX GEMMs of
// an MLP only quantised images are read, so h = silu(g) * u and dgu = [dg | du]
// need not go to memory as bf16 at all.
//
//   swiglu_rows_kernel      quantize_rows_kernel of h            (gu read once)
//   swiglu_tr_kernel        quantize_tr_kernel (not DUAL) of h   (gu read once)
//   swiglu_bwd_dual_kernel  quantize_tr_kernel (DUAL) of dgu     (gu, dh read once)
//
// gu = [g (F) | u (F)] per row, as mxk_swiglu_fwd / mxk_swiglu_bwd take it
// (fused_ops.hip).  The arithmetic is those kernels', expression for expression,
// and the result is rounded to bf16 (v_cvt_pk_bf16_f32, as store8 there) before
// quantize_quarter sees it, so every image equals, bit for bit, the image the
// stand-alone quantiser makes of the stand-alone SwiGLU kernel's output
// (tests/test_gpu_swiglu_mx.py).  quantize_quarter, store_quarter, sr_lane and
// the tile constants are mx_quantize.h's, unchanged; so are the LDS image and
// the store phase of the transposing kernels, whose comment there explains the
// padding.  Only the 16-B / packed-store forms exist: the entry points refuse
// what is not aligned for them.
//
// swiglu_bwd_dual_kernel: a workgroup takes 128 rows x 64 F-columns and makes
// the dg tile (output columns c) and the du tile (output columns F + c) of it,
// so the sigmoid is computed once per element.  It keeps two LDS tile images
// and one barrier.  hipcc reports for E4m3 / E2m1 / E2m1Sr 74 / 51 / 88 VGPRs
// and 33 792 B of LDS, no scratch: the LDS allows 4 workgroups per CU, 4 waves
// per SIMD, the registers 6 / 8 / 5.  The other form, one image reused for du
// after the dg store phase (du held in registers meanwhile, two more
// barriers), compiles to 84 / 62 / 95 VGPRs and 16 896 B, no scratch: 5 / 8 /
// 5 waves per SIMD by registers, not limited by LDS.  So the one-image form
// could keep 1 / 4 / 1 more waves resident; this one has a third of the
// barriers.  The code is straight-line and bound by vector ALU issue, which 4
// waves per SIMD already fill, so the two-image form was built and measured;
// the one-image form was compiled for these figures and not timed.
// (profiles/mx_swiglu/README.md has the figures.)  With a stochastic format
// the SrLane indices are those of dgu's images ([T, 2F] and [2F, T]): the row
// image draws with seed, the transposed one with seed + 1.
#pragma once
#include "mx_quantize.h"

namespace mxk {
namespace mx {

__device__ __forceinline__ void unpack8(const uint4& v, float (&f)[8]) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(w[i] << 16);
    f[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u);
  }
}

__device__ __forceinline__ void pack8(const float (&f)[8], uint32_t (&w)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = mxk::pack2bf(f[2 * i], f[2 * i + 1]);
}

// 8 elements of h = silu(g) * u as 4 dwords of bf16: mxk_swiglu_fwd_kernel's expression
__device__ __forceinline__ void swiglu_fwd8(const uint4& gv, const uint4& uv, uint32_t (&w)[4]) {
  float g[8], u[8], o[8];
  unpack8(gv, g);
  unpack8(uv, u);
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = g[e] / (1.f + __expf(-g[e])) * u[e];
  pack8(o, w);
}

// 8 elements of dg and of du: mxk_swiglu_bwd_kernel's expressions
__device__ __forceinline__ void swiglu_bwd8(const uint4& gv, const uint4& uv, const uint4& dv,
                                            uint32_t (&wg)[4], uint32_t (&wu)[4]) {
  float g[8], u[8], d[8], dg[8], du[8];
  unpack8(gv, g);
  unpack8(uv, u);
  unpack8(dv, d);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float s = 1.f / (1.f + __expf(-g[e]));
    du[e] = d[e] * g[e] * s;
    dg[e] = d[e] * u[e] * s * (1.f + g[e] * (1.f - s));
  }
  pack8(dg, wg);
  pack8(du, wu);
}

// ---- row image of h -----------------------------------------------------------
// quantize_rows_kernel<Fmt, true> with the lane's 8 elements computed from two
// 16-B loads.
template <class Fmt>
__global__ void __launch_bounds__(256)
swiglu_rows_kernel(const uint16_t* __restrict__ gu, uint8_t* __restrict__ q, uint8_t* __restrict__ s,
                   long T, long F, long ldgu, long ldq, long lds) {
  const long per_row = F >> 3;
  const long gid = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  // F % 32 == 0, so a quad never straddles a row and leaves the grid whole
  if (gid >= T * per_row) return;
  const long row = gid / per_row;
  const long c8 = gid - row * per_row;
  const uint16_t* gp = gu + row * ldgu + c8 * 8;
  uint32_t w[4];
  swiglu_fwd8(*reinterpret_cast<const uint4*>(gp), *reinterpret_cast<const uint4*>(gp + F), w);
  uint32_t out[Fmt::kBits / 4];
  const int e = quantize_quarter<Fmt>(w, out);
  store_quarter<Fmt>(q + row * ldq + c8 * Fmt::kBits, out);
  if ((c8 & 3) == 0) s[row * lds + (c8 >> 2)] = static_cast<uint8_t>(e + 127);
}

// The lane's transposed hand-off of quantize_tr_kernel: rows rl, rl + 1 of
// chunk k (8 columns) into the image T[c][r] of bf16.
__device__ __forceinline__ void tr_lds_store(char* tile, int k, int rl, const uint32_t (&w)[2][4]) {
  char* tp = tile + (k * 8) * kTrLdsRow + rl * 2;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    *reinterpret_cast<uint32_t*>(tp + (2 * i) * kTrLdsRow) = (w[0][i] & 0xFFFFu) | (w[1][i] << 16);
    *reinterpret_cast<uint32_t*>(tp + (2 * i + 1) * kTrLdsRow) =
        (w[0][i] >> 16) | (w[1][i] & 0xFFFF0000u);
  }
}

// The store phase of quantize_tr_kernel for one tile image: column c0 + cl of
// the tile is row crow0 + cl of the output image, whose rows are R elements.
template <class Fmt, class... Seed>
__device__ __forceinline__ void tr_store_phase(const char* tile, uint8_t* __restrict__ qt,
                                               uint8_t* __restrict__ st, long R, long C, long r0,
                                               long c0, long crow0, long ldqt, long ldst,
                                               Seed... seed) {
  constexpr int kPack = Fmt::kBits == 4;
  const int t = threadIdx.x;
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
    const long orow = crow0 + cl;
    const int e = quantize_quarter<Fmt>(w, out, sr_lane(row >> 3, orow, seed)...);
    if (row < R && c0 + cl < C) {   // R % 32 == 0: whole blocks
      store_quarter<Fmt>(qt + orow * ldqt + (row >> kPack), out);
      if ((r8 & 3) == 0) st[orow * ldst + (row >> 5)] = static_cast<uint8_t>(e + 127);
    }
  }
}

// ---- transposed image of h ----------------------------------------------------
// quantize_tr_kernel<Fmt, true, false>: 128 rows x 64 columns of h per
// workgroup; rows >= T and columns >= F of a ragged tile load zeros (h = 0)
// and store nothing, so every lane of a DPP quad stays active.
template <class Fmt>
__global__ void __launch_bounds__(256)
swiglu_tr_kernel(const uint16_t* __restrict__ gu, uint8_t* __restrict__ qt, uint8_t* __restrict__ st,
                 long T, long F, long ldgu, long ldqt, long ldst) {
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
      const uint16_t* gp = gu + row * ldgu + col;
      uint4 gv = make_uint4(0, 0, 0, 0), uv = gv;
      if (row < T && col < F) {   // F % 8 == 0
        gv = *reinterpret_cast<const uint4*>(gp);
        uv = *reinterpret_cast<const uint4*>(gp + F);
      }
      swiglu_fwd8(gv, uv, w[h]);
    }
    tr_lds_store(tile, k, rl, w);
  }
  __syncthreads();
  tr_store_phase<Fmt>(tile, qt, st, T, F, r0, c0, c0, ldqt, ldst);
}

// ---- both images of dgu -------------------------------------------------------
template <class Fmt, class... Seed>
__global__ void __launch_bounds__(256)
swiglu_bwd_dual_kernel(const uint16_t* __restrict__ gu, const uint16_t* __restrict__ dh,
                       uint8_t* __restrict__ q, uint8_t* __restrict__ s, uint8_t* __restrict__ qt,
                       uint8_t* __restrict__ st, long T, long F, long ldgu, long lddh, long ldq,
                       long lds, long ldqt, long ldst, Seed... seed) {
  constexpr int kPack = Fmt::kBits == 4;   // element index >> kPack = byte of a row
  __shared__ __attribute__((aligned(8))) char tile[2][kTrCols * kTrLdsRow];   // dg, du
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
    uint32_t wg[2][4], wu[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long row = r0 + rl + h;
      const bool in = row < T && col < F;   // F % 32 == 0: whole blocks
      const uint16_t* gp = gu + row * ldgu + col;
      uint4 gv = make_uint4(0, 0, 0, 0), uv = gv, dv = gv;
      if (in) {
        gv = *reinterpret_cast<const uint4*>(gp);
        uv = *reinterpret_cast<const uint4*>(gp + F);
        dv = *reinterpret_cast<const uint4*>(dh + row * lddh + col);
      }
      swiglu_bwd8(gv, uv, dv, wg[h], wu[h]);
      // the row images, as DUAL does: dg at output column col, du at F + col
      uint32_t og[Fmt::kBits / 4], ou[Fmt::kBits / 4];
      const int eg = quantize_quarter<Fmt>(wg[h], og, sr_lane(col >> 3, row, seed)...);
      const int eu = quantize_quarter<Fmt>(wu[h], ou, sr_lane((F + col) >> 3, row, seed)...);
      if (in) {
        store_quarter<Fmt>(q + row * ldq + (col >> kPack), og);
        store_quarter<Fmt>(q + row * ldq + ((F + col) >> kPack), ou);
        if ((k & 3) == 0) {
          s[row * lds + (col >> 5)] = static_cast<uint8_t>(eg + 127);
          s[row * lds + ((F + col) >> 5)] = static_cast<uint8_t>(eu + 127);
        }
      }
    }
    tr_lds_store(tile[0], k, rl, wg);
    tr_lds_store(tile[1], k, rl, wu);
  }
  __syncthreads();
  // stochastic: the transposed image of a dual call draws with seed + 1
  tr_store_phase<Fmt>(tile[0], qt, st, T, F, r0, c0, c0, ldqt, ldst, (seed + 1u)...);
  tr_store_phase<Fmt>(tile[1], qt, st, T, F, r0, c0, F + c0, ldqt, ldst, (seed + 1u)...);
}

// ---- host sides ---------------------------------------------------------------
// gu bf16 [T][2F] (row stride ldgu elements), dh bf16 [T][F] (lddh); the images
// as launch_quantize_rows / launch_quantize_tr lay them out, of h [T][F] or of
// dgu [T][2F].  Only what the 16-B loads and packed stores take is accepted.
inline bool swiglu_in_ok(const void* p, long ld, long width) {
  return p && aligned(p, 16) && ld >= width && ld % 8 == 0;
}
template <class Fmt>
inline bool swiglu_codes_ok(const void* qp, const void* sp, long ldq, long lds, long width) {
  constexpr int kB = Fmt::kBits;
  return qp && sp && aligned(qp, kB) && ldq % kB == 0 && ldq >= width / (8 / kB) && lds >= width / 32;
}

template <class Fmt>
int launch_swiglu_rows(const void* gu, void* q, void* s, long T, long F, long ldgu, long ldq, long lds,
                       hipStream_t stream) {
  if (T <= 0 || F <= 0 || F % 32 || !swiglu_in_ok(gu, ldgu, 2 * F) ||
      !swiglu_codes_ok<Fmt>(q, s, ldq, lds, F))
    return static_cast<int>(hipErrorInvalidValue);
  if (T > 0x7FFFFFFFFFFFL / F) return static_cast<int>(hipErrorInvalidValue);
  const long blocks = (T * (F / 8) + 255) / 256;
  if (blocks > 0x7FFFFFFFL) return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(swiglu_rows_kernel<Fmt>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream,
                     static_cast<const uint16_t*>(gu), static_cast<uint8_t*>(q),
                     static_cast<uint8_t*>(s), T, F, ldgu, ldq, lds);
  MXK_RETURN_LAUNCH_STATUS();
}

// The grid of the transposing forms (launch_quantize_tr's limits); false: refuse.
inline bool swiglu_tr_grid(long T, long F, dim3* grid) {
  const long gx = (T + kTrRows - 1) / kTrRows, gy = (F + kTrCols - 1) / kTrCols;
  if (gx > 0x7FFFFFFFL || gy > 65535) return false;
  *grid = dim3(static_cast<unsigned>(gx), static_cast<unsigned>(gy));
  return true;
}

template <class Fmt>
int launch_swiglu_tr(const void* gu, void* qt, void* st, long T, long F, long ldgu, long ldqt,
                     long ldst, hipStream_t stream) {
  dim3 grid;
  if (T <= 0 || F <= 0 || F % 32 || T % 32 || !swiglu_in_ok(gu, ldgu, 2 * F) ||
      !swiglu_codes_ok<Fmt>(qt, st, ldqt, ldst, T) || !swiglu_tr_grid(T, F, &grid))
    return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(swiglu_tr_kernel<Fmt>, grid, dim3(256), 0, stream,
                     static_cast<const uint16_t*>(gu), static_cast<uint8_t*>(qt),
                     static_cast<uint8_t*>(st), T, F, ldgu, ldqt, ldst);
  MXK_RETURN_LAUNCH_STATUS();
}

template <class Fmt, class... Seed>
int launch_swiglu_bwd_dual(const void* gu, const void* dh, void* q, void* s, void* qt, void* st, long T,
                           long F, long ldgu, long lddh, long ldq, long lds, long ldqt, long ldst,
                           hipStream_t stream, Seed... seed) {
  dim3 grid;
  if (T <= 0 || F <= 0 || F % 32 || T % 32 || !swiglu_in_ok(gu, ldgu, 2 * F) ||
      !swiglu_in_ok(dh, lddh, F) || !swiglu_codes_ok<Fmt>(q, s, ldq, lds, 2 * F) ||
      !swiglu_codes_ok<Fmt>(qt, st, ldqt, ldst, T) || !swiglu_tr_grid(T, F, &grid))
    return static_cast<int>(hipErrorInvalidValue);
  if (sizeof...(Seed) != 0 && (T > kSrMaxIndex || 2 * F > kSrMaxIndex))
    return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL((swiglu_bwd_dual_kernel<Fmt, Seed...>), grid, dim3(256), 0, stream,
                     static_cast<const uint16_t*>(gu), static_cast<const uint16_t*>(dh),
                     static_cast<uint8_t*>(q), static_cast<uint8_t*>(s), static_cast<uint8_t*>(qt),
                     static_cast<uint8_t*>(st), T, F, ldgu, lddh, ldq, lds, ldqt, ldst, seed...);
  MXK_RETURN_LAUNCH_STATUS();
}

}  // namespace mx
}  // namespace mxk
