"""The GEMM K-tiles with bare LDS-DMA pieces (``mxk::dma16q``) and their M0
writes in MFMA gaps of their own (``mxk::m0_put``): outputs against the K-tile
they replace and against fp64.

1. TN schedule 52 against schedule 59, the same K-tile with its pieces through
   the builtin (the form 52 had; experiments library only, so this part skips
   on the production library): ``torch.equal`` on the bits.  The same MFMAs
   run in the same order on the same fragments, so nothing may differ.
   256 x 256 x 64 ns for ns = 1, 2, 3, 7, 8, 9, 14: the two DMA-free tail
   K-tiles alone (1, 2), every remainder of the unroll by six (ns - 2 = 1, 5,
   0, 1 after one trip) and two trips (14); 512 x 768 x 576 with lda and ldb
   padded by 64.
2. Against the fp64 reference and bound of ``tests/kernel_refs.py``
   (``gemm_plain``: 2^-8 |d| + K 2^-23 S + atol; ``gemm_rope`` for the rotary
   epilogue; ``test_gpu_gemm_numerics.py`` derives both), inputs uniform in
   [-1, 1): schedule 52 on the shapes of part 1, the RoPE-epilogue GEMM at
   256 x 256 x 448, and the four operand layouts of ``mxk_gemm_bf16_ex`` at
   256 x 512 x 128 and x 1152 (the layout K-tile's DMA-free tails alone, and
   eight trips of its loop).  This part never skips.
"""
import functools

import pytest
import torch

import kernel_refs as R
from mxk8s.ops import _lib
from test_gpu_fused_numerics import _bits
from test_gpu_gemm_numerics import LAYOUTS, _Buf, _Tally, _operands, _run_tn_variant, _stream

pytestmark = pytest.mark.gpu

RECORD = 59
TN_CASES = [(256, 256, 64 * ns, 0) for ns in (1, 2, 3, 7, 8, 9, 14)] + [(512, 768, 576, 64)]
EX_KS = (128, 1152)
ROPE_SHAPE = (256, 256, 448)
ROPE_S, ROPE_COLS = 256, 128


@functools.lru_cache(maxsize=None)
def _uniform(M, N, K):
    """a [M][K], b [K][N] bf16, uniform in [-1, 1), and the fp64 (d, bound)."""
    gen = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    top = 1.0 - 2.0 ** -8           # the largest bf16 below 1: rounding never reaches 1
    a = (torch.rand((M, K), generator=gen) * 2 - 1).bfloat16().clamp(max=top)
    b = (torch.rand((K, N), generator=gen) * 2 - 1).bfloat16().clamp(max=top)
    d, bound, _ = R.gemm_plain(a, b)
    return a, b, d, bound


def _record_built():
    L = _lib.lib()
    return L.mxk_gemm_bf16_tn_num_variants() > RECORD and bool(L.mxk_gemm_bf16_tn_variant_built(RECORD))


@pytest.mark.parametrize("M,N,K,pad", TN_CASES)
def test_schedule_52_bit_equal_to_the_builtin_dma_record(cuda_device, M, N, K, pad):
    if not _record_built():
        pytest.skip("schedule 59 is an A/B record of the experiments library")
    assert _lib.lib().mxk_gemm_bf16_tn_variant_name(RECORD) == b"w4k_border_builtin_dma"
    a, b, _, _ = _uniform(M, N, K)
    A, B = _operands(a, b, "tn", cuda_device, K + pad, K + pad)
    new, old = _Buf(M, N, cuda_device), _Buf(M, N, cuda_device)
    _run_tn_variant(A, B, new, M, N, K, 52)
    _run_tn_variant(A, B, old, M, N, K, RECORD)
    assert torch.equal(_bits(new.t), _bits(old.t))
    assert new.pads_intact() and old.pads_intact() and A.pads_intact() and B.pads_intact()


@pytest.mark.parametrize("M,N,K,pad", TN_CASES)
def test_schedule_52_against_fp64(cuda_device, M, N, K, pad):
    a, b, d, bound = _uniform(M, N, K)
    tally = _Tally(f"dma_gaps tn52[{M}x{N}x{K},ld+{pad}]", d, bound, cuda_device)
    A, B = _operands(a, b, "tn", cuda_device, K + pad, K + pad)
    C = _Buf(M, N, cuda_device)
    _run_tn_variant(A, B, C, M, N, K, 52)
    tally.check("schedule 52", C.t)
    if not (A.pads_intact() and B.pads_intact() and C.pads_intact()):
        tally.fail("schedule 52", "padding overwritten")
    tally.done()


def test_rope_epilogue_gemm_against_fp64(cuda_device):
    from mxk8s.ops.fused import rope_tables
    M, N, K = ROPE_SHAPE
    a, b, _, _ = _uniform(M, N, K)
    cos, sin = rope_tables(ROPE_S, 128)
    ref, bound = R.gemm_rope(a, b, cos, sin, ROPE_S, ROPE_COLS)
    tally = _Tally(f"dma_gaps rope[{M}x{N}/{ROPE_COLS}x{K}]", ref, bound, cuda_device)
    A, B = _operands(a, b, "tn", cuda_device)
    C = _Buf(M, N, cuda_device)
    cos_d, sin_d = cos.to(cuda_device), sin.to(cuda_device)
    assert cos_d.shape == (ROPE_S, 64) and cos_d.dtype == torch.float32 and cos_d.is_contiguous()
    st = _lib.lib().mxk_gemm_bf16_rope(A.ptr, B.ptr, C.ptr, M, N, K, A.ld, B.ld, C.ld, cos_d.data_ptr(),
                                       sin_d.data_ptr(), ROPE_S, ROPE_COLS, _stream(cuda_device))
    _lib.check(st, "mxk_gemm_bf16_rope")
    torch.cuda.synchronize()
    tally.check("rope", C.t)
    if not C.pads_intact():
        tally.fail("rope", "padding overwritten")
    tally.done()


@pytest.mark.parametrize("K", EX_KS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layout_gemm_against_fp64(cuda_device, layout, K):
    M, N = 256, 512
    ak, bk = LAYOUTS[layout]
    a, b, d, bound = _uniform(M, N, K)
    tally = _Tally(f"dma_gaps ex[{layout},{M}x{N}x{K}]", d, bound, cuda_device)
    A, B = _operands(a, b, layout, cuda_device)
    C = _Buf(M, N, cuda_device)
    st = _lib.lib().mxk_gemm_bf16_ex(A.ptr, B.ptr, C.ptr, M, N, K, A.ld, B.ld, C.ld, ak, bk,
                                     _stream(cuda_device))
    _lib.check(st, f"mxk_gemm_bf16_ex {layout}")
    torch.cuda.synchronize()
    tally.check("ex", C.t)
    if not (A.pads_intact() and B.pads_intact() and C.pads_intact()):
        tally.fail("ex", "padding overwritten")
    tally.done()
