// SwiGLU fused into the MXFP8 / MXFP4 quantisers (mx_swiglu_quantize.h has the
// kernels): what the MX MLP node (mxk8s.ops.linear.swiglu_mlp_mx) puts between
// its GEMMs instead of mxk_swiglu_fwd / mxk_swiglu_bwd and a quantiser each.
//
//   mxk_swiglu_quantize_<fmt>           row image of h = silu(g) * u
//   mxk_swiglu_quantize_<fmt>_t         transposed image of h (blocks of 32 tokens)
//   mxk_swiglu_bwd_quantize_<fmt>_dual  both images of dgu = [dg | du]
//   mxk_swiglu_bwd_quantize_mxfp4_sr_dual   the same with stochastic rounding
//
// Each image equals, bit for bit, mxk_quantize_<fmt>{,_t,_dual} of the bf16
// tensor that mxk_swiglu_fwd / mxk_swiglu_bwd writes.
//
// Contract (any violation returns hipErrorInvalidValue and launches nothing):
// T > 0 tokens, F > 0 with F % 32 == 0, T % 32 == 0 for the transposing and
// dual forms; gu bf16 [T][2F] and dh bf16 [T][F], 16-B aligned, row strides
// (elements) >= the width and multiples of 8; code images aligned to 8 B (e4m3)
// or 4 B (e2m1) with row strides (bytes) that are multiples of that and >= the
// row, scale rows >= the blocks of a row; F <= 64 * 65535 for the transposing
// and dual forms; T and 2F below 2^32 for the stochastic form.  T need not be a
// multiple of 128, nor F of 64.
#include "mx_gemm_core.h"
#include "mx_swiglu_quantize.h"
#include "mx_formats.h"

using namespace mxk::mx;

#define MXK_SWIGLU_QUANTIZE(NAME, FMT)                                                              \
  MXK_API int mxk_swiglu_quantize_##NAME(const void* gu, void* q, void* s, long T, long F,          \
                                         long ldgu, long ldq, long lds, hipStream_t stream) {       \
    return launch_swiglu_rows<FMT>(gu, q, s, T, F, ldgu, ldq, lds, stream);                         \
  }                                                                                                 \
  MXK_API int mxk_swiglu_quantize_##NAME##_t(const void* gu, void* qt, void* st, long T, long F,    \
                                             long ldgu, long ldqt, long ldst, hipStream_t stream) { \
    return launch_swiglu_tr<FMT>(gu, qt, st, T, F, ldgu, ldqt, ldst, stream);                       \
  }                                                                                                 \
  MXK_API int mxk_swiglu_bwd_quantize_##NAME##_dual(                                                \
      const void* gu, const void* dh, void* q, void* s, void* qt, void* st, long T, long F,         \
      long ldgu, long lddh, long ldq, long lds, long ldqt, long ldst, hipStream_t stream) {         \
    return launch_swiglu_bwd_dual<FMT>(gu, dh, q, s, qt, st, T, F, ldgu, lddh, ldq, lds, ldqt,      \
                                       ldst, stream);                                               \
  }

MXK_SWIGLU_QUANTIZE(mxfp8, E4m3)
MXK_SWIGLU_QUANTIZE(mxfp4, E2m1)

MXK_API int mxk_swiglu_bwd_quantize_mxfp4_sr_dual(const void* gu, const void* dh, void* q, void* s,
                                                  void* qt, void* st, long T, long F, long ldgu,
                                                  long lddh, long ldq, long lds, long ldqt, long ldst,
                                                  uint64_t seed, hipStream_t stream) {
  return launch_swiglu_bwd_dual<E2m1Sr>(gu, dh, q, s, qt, st, T, F, ldgu, lddh, ldq, lds, ldqt, ldst,
                                        stream, seed);
}
