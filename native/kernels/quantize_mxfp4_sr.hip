// MXFP4 quantisers with stochastic rounding, for the gradient operand of the
// MXFP4 training route (mxk8s.ops.linear.linear_mxfp4, grad_rounding =
// "stochastic").  The images are ordinary MXFP4 (gemm_mxfp4.hip has the
// storage, mxk_gemm_mxfp4_tn consumes them); what differs is the rounding:
//
//   mxk_quantize_mxfp4_sr       bf16 rows -> packed e2m1 nibbles + E8M0 bytes
//   mxk_quantize_mxfp4_sr_t     the same of x^T (blocks of 32 rows), stored transposed
//   mxk_quantize_mxfp4_sr_dual  both images from one read of x; the transposed
//                               one draws with seed + 1 (mod 2^64)
//
// Definition (mxfp4_format.h, mx_philox.h; mxk8s.ops.mxfp4.quantize_mxfp4_ref
// with rounding="stochastic" is the same, bit for bit):
//   * block exponent block_exp_noclip: scaled block maxima in (3, 6], nothing
//     is clamped (round-to-nearest's [4, 8) with its clamp at 6 shrinks every
//     block, which random rounding alone cannot repair);
//   * element 8 g + j of row i of the OUTPUT image rounds to one of its two
//     e2m1 neighbours with the 16 bits (word[j >> 1] >> 16 (j & 1)) & 0xffff of
//     Philox4x32-10(counter (g, i, 0, 0), key (seed & 0xffffffff, seed >> 32)),
//     the upper one with probability (|x| - lo) / gap: E[dequant] = x to
//     within gap 2^(e - 16).
// One Philox call per lane and quarter block: a lane converts exactly these 8
// elements in every kernel of mx_quantize.h (row kernel (row, c8), DUAL load
// phase (row, col / 8), store phase (c, (r0 + 8 r8) / 8)), so the kernels are
// those templates on the format below and the transposing forms equal the row
// form of the transposed copy.  Counter-based, hence stateless: the same
// (seed, element) always gets the same bits, whatever the launch order.  The
// key words come from the kernel argument and are wave-uniform: they and their
// ten Weyl increments stay in scalar registers.
//
// Follow-up, deliberately not used here: gfx950 has a hardware path
// (v_cvt_scalef32_sr_pk_fp4_bf16 fed by v_prng_b32).  It is stateful and
// cannot be checked bit for bit against a CPU reference.
#include "mx_gemm_core.h"
#include "mx_quantize.h"
#include "mx_philox.h"
#include "mxfp4_format.h"
#include "mx_formats.h"   // struct E2m1Sr

namespace {

using namespace mxk::mx;

}  // namespace

// The contracts of mxk_quantize_mxfp4, _t and _dual (gemm_mxfp4.hip), R, K and
// C below 2^32, and the seed of the definition above.
MXK_API int mxk_quantize_mxfp4_sr(const void* x, void* q, void* s, long R, int K, long ldx, long ldq,
                                  long lds, uint64_t seed, hipStream_t stream) {
  return launch_quantize_rows<E2m1Sr>(x, q, s, R, K, ldx, ldq, lds, stream, seed);
}

MXK_API int mxk_quantize_mxfp4_sr_t(const void* x, void* qt, void* st, long R, long C, long ldx,
                                    long ldqt, long ldst, uint64_t seed, hipStream_t stream) {
  return launch_quantize_tr<E2m1Sr>(false, x, nullptr, nullptr, qt, st, R, C, ldx, 0, 0, ldqt, ldst,
                                    stream, seed);
}

MXK_API int mxk_quantize_mxfp4_sr_dual(const void* x, void* q, void* s, void* qt, void* st, long R,
                                       long C, long ldx, long ldq, long lds, long ldqt, long ldst,
                                       uint64_t seed, hipStream_t stream) {
  return launch_quantize_tr<E2m1Sr>(true, x, q, s, qt, st, R, C, ldx, ldq, lds, ldqt, ldst, stream, seed);
}
