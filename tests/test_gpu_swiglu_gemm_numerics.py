"""Elementwise fp64 checks of the two bf16 GEMMs with a SwiGLU epilogue:
``mxk_gemm_bf16_dgrad_swiglu`` (``gemm_bf16_layouts.hip``; epilogues EPI 2, 3
and 4 of the layout kernel, ``mx_common.h`` ``swiglu_bwd_block``, ``_wide``,
``_lds``) and ``mxk_gemm_bf16_w13_swiglu`` (``gemm_bf16.hip``), called through
``_lib`` into poisoned outputs.  The references are fp64 on the CPU
(``tests/kernel_refs.py``), so no GPU BLAS is trusted.

The GEMM term.  Products of two bf16 values are exact in fp32, so a dot
product of depth K only rounds in its K - 1 additions: in any order, with
round-to-nearest, |acc - d| <= (K - 1) 2^-24 S with S = sum |a| |b|.  MFMA's
internal adds are not documented to round to nearest, hence a factor 2:

    delta = K 2^-23 S.

The sigmoid chain.  The kernels compute s = rcp(1 + exp2(g * -1.44269504f)).
The product carries a relative error of 2^-24 (and the constant one of
2^-25), which exp2 turns into a relative error of about |g| 2^-24; exp2 and
rcp add an ulp each, and every fp32 multiply after them 2^-24.  All of it is
inside

    c(g) = (|g| + 8) 2^-23     (relative, twice what the steps add up to).

dgrad-SwiGLU, from d = dy W2 (fp32 accumulators), s = sigmoid(g) and
f = 1 + g sigmoid(-g):  dg = d u s f,  du = d g s.  The kernel evaluates f as
(g + 1) - g s, which cancels for g > 0 and next to g = -1.2785 (f = 0), so
the chain's error is weighed with the terms |1 + g| and |g| s, not with |f|:

    bound_dg = 2^-8 |dg| + delta |u s f| + c(g) |d u s| (|1 + g| + |g| s) + atol
    bound_du = 2^-8 |du| + delta |g s|   + c(g) |du|                      + atol

Up-projection: gu = x W13^T rounded to bf16, and h = silu(g) u computed from
the fp32 accumulators (so the reference of h uses the unrounded g, u), with
silu'(g) = s f carrying the accumulation error of g into h:

    bound_gu = 2^-8 |gu| + delta                                          + atol
    bound_h  = 2^-8 |h| + delta_g |u silu'(g)| + delta_u |silu(g)| + c(g) |h| + atol

2^-8 is round-to-nearest bf16 just above a power of two (rounding alone
reaches 0.996 of it); atol = 1e-30 only matters next to zero.  No product of
two operands is below 2^-60, so flush-to-zero in MFMA or v_rcp_f32 cannot
matter; for g below -87 the true s d u is under atol.

Inputs (``kernel_refs.dgrad_inputs`` / ``w13_inputs``) tell rows and columns
apart: power-of-two scales per row and per column with different periods,
zero rows and columns, and for the dgrad whole columns of g at 0, 2^-20,
-1.2785, +-17, -30, -87, -88.5, -100, -126, 100 and 128.  The *tight*
family adds terms of one sign in every dot product (S = |d|: the bound is
bf16 rounding and little else, asserted from the reference alone as
``loose_fraction <= 10 %``), the *signed* family lets d cancel so that delta
carries weight.  ``tests/test_kernel_refs_cpu.py`` shows that a float32
emulation of each epilogue stays inside these bounds and that planted defects
(g / u of the wrong 4-row group, a wrong u offset, gate and up exchanged in
half a wave pair, a dropped K-tile, a wrong sigmoid branch) leave them.

Every check prints one RATIO line (largest error / bound).
"""
import ctypes
import functools

import pytest
import torch

import kernel_refs as R
from mxk8s.ops import _lib
from test_gpu_fused_numerics import _bits, _poison

pytestmark = pytest.mark.gpu

FAMILIES = ["tight", "signed"]


def _check(what, got, ref, bound):
    ratio = R.bound_ratio(got, ref, bound)
    print(f"RATIO {what} {ratio:.3g}")
    assert ratio <= 1, f"{what}: largest error / bound = {ratio:.3g}"


def _check_sharp(what, ref, bound):
    loose = R.loose_fraction(ref, bound)
    assert loose <= 0.10, f"{what}: {loose:.3f} of the bounds are not bf16 rounding alone"


def _at_offset(t, dev, nbytes):
    """A copy of ``t`` on ``dev`` whose first byte sits ``nbytes`` past a 16-B
    boundary (rows of 2F bf16 keep that phase)."""
    skip = nbytes // 2
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[skip:skip + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == nbytes
    return view


# ---- dgrad-SwiGLU -----------------------------------------------------------
def _planned_epi(dy, w2, gu, dgu, M, F, K, mode):
    L = _lib.lib()
    out = (ctypes.c_long * 5)()
    st = L.mxk_gemm_bf16_dgrad_swiglu_plan(
        M, F, K, K, F, *(t.data_ptr() % 16 for t in (dy, w2, gu, dgu)), mode, 0,
        int(bool(L.mxk_gemm_bf16_tn_variant_built(54))), L.mxk_gemm_available_cus(), 1, out)
    assert st == 0
    assert (out[1], out[2]) == (0, 0)
    return out[0]


def _run_dgrad(dy, w2, gu, dgu, mode, expect_epi):
    """One launch under epilogue mode ``mode``, after asserting the epilogue
    the plan resolves this very call to."""
    L = _lib.lib()
    M, K = dy.shape
    F = w2.shape[1]
    assert _planned_epi(dy, w2, gu, dgu, M, F, K, mode) == expect_epi
    try:
        L.mxk_gemm_swiglu_set_epi(mode)
        st = L.mxk_gemm_bf16_dgrad_swiglu(dy.data_ptr(), w2.data_ptr(), gu.data_ptr(), dgu.data_ptr(),
                                          M, F, K, K, F, _lib.stream_ptr(dy.device))
    finally:
        L.mxk_gemm_swiglu_set_epi(4)
    _lib.check(st, f"dgrad_swiglu mode {mode}")
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _dgrad_case(M, F, K, family):
    inputs = R.dgrad_inputs(M, F, K, family)
    return inputs, R.dgrad_swiglu(*inputs)


# (name, mode, gu phase, dgu phase, EPI for K >= 2 K-tiles); one K-tile is EPI 2 always
DGRAD_MODES = [("mode4", 4, 0, 0, 4), ("mode3", 3, 0, 0, 3), ("mode0", 0, 0, 0, 2),
               ("mode4-gu8", 4, 8, 0, 2), ("mode4-dgu8", 4, 0, 8, 2)]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("K", [64, 128, 192, 256, 320])
@pytest.mark.parametrize("M,F", [(256, 256), (512, 512)])
def test_dgrad_swiglu_elementwise(cuda_device, M, F, K, family):
    """EPI 4, 3 and 2 over 1-5 K-tiles (both parities of the stage the g / u
    prefetch lands in), EPI 2 also as the route of a gu or dgu at 8 mod 16."""
    (dy, w2, gu), (dg, bound_dg, du, bound_du) = _dgrad_case(M, F, K, family)
    if family == "tight":
        _check_sharp("dg", dg, bound_dg)
        _check_sharp("du", du, bound_du)
    dev = cuda_device
    dy_d, w2_d = dy.to(dev), w2.to(dev)
    bits = {}
    for name, mode, gu_off, dgu_off, epi in DGRAD_MODES:
        gu_d = _at_offset(gu, dev, gu_off)
        dgu = _at_offset(_poison((M, 2 * F), torch.bfloat16, "cpu"), dev, dgu_off)
        _run_dgrad(dy_d, w2_d, gu_d, dgu, mode, epi if K >= 128 else 2)
        tag = f"dgrad[{M}x{F}x{K},{family},{name}]"
        _check(f"{tag} dg", dgu[:, :F], dg, bound_dg)
        _check(f"{tag} du", dgu[:, F:], du, bound_du)
        bits[name] = _bits(dgu)
    # EPI 3 and 4 share their arithmetic; so do the three routes to EPI 2
    assert torch.equal(bits["mode4"], bits["mode3"]), "modes 4 and 3 differ in bits"
    assert torch.equal(bits["mode0"], bits["mode4-gu8"]) and torch.equal(bits["mode0"], bits["mode4-dgu8"])


def test_dgrad_swiglu_through_autograd(cuda_device):
    """SwiGLULinear's backward reaches the same kernel: gu.grad within the
    bound and bit-equal to the direct call."""
    from mxk8s.ops.linear import SwiGLULinear
    M, F, K = 512, 512, 256
    (dy, w2, gu), (dg, bound_dg, du, bound_du) = _dgrad_case(M, F, K, "signed")
    dev = cuda_device
    lin = SwiGLULinear(F, K).to(dev).bfloat16()
    with torch.no_grad():
        lin.weight.copy_(w2.to(dev))
    gu_d = gu.to(dev).requires_grad_()
    lin(gu_d).backward(dy.to(dev))
    _check("dgrad[autograd] dg", gu_d.grad[:, :F], dg, bound_dg)
    _check("dgrad[autograd] du", gu_d.grad[:, F:], du, bound_du)
    dgu = _poison((M, 2 * F), torch.bfloat16, dev)
    _run_dgrad(dy.to(dev), lin.weight.detach(), gu_d.detach(), dgu, 4, 4)
    assert torch.equal(_bits(dgu), _bits(gu_d.grad))


def test_dgrad_swiglu_gu_past_4gib(cuda_device):
    """gu and dgu of 4 GiB + 256 KiB.  The g / u prefetch of EPI 4 addresses gu
    with a 32-bit byte offset from its first row; past 4 GiB that wraps to
    rows 2^32 / (4F) further up, silently (the wrapped rows exist).  Such a
    call must run without the prefetch (EPI 3).  Only the first and the last
    256-row tile carry data, different in the two, so a wrapped read in the
    last tile combines d with g / u of the first."""
    F, K = 256, 128
    M = (1 << 22) + 256
    dev = cuda_device
    if torch.cuda.mem_get_info(dev)[0] < 12 << 30:
        pytest.skip("needs 12 GiB of free device memory")
    dy0, w2, gu0 = R.dgrad_inputs(256, F, K, "tight")
    dy1, _, gu1 = R.dgrad_inputs(256, F, K, "tight", seed=1, row0=3)
    assert not torch.equal(gu0, gu1) and not torch.equal(dy0, dy1)
    dy = gu = dgu = None
    try:
        dy = torch.zeros((M, K), dtype=torch.bfloat16, device=dev)
        gu = torch.zeros((M, 2 * F), dtype=torch.bfloat16, device=dev)
        dy[:256], dy[M - 256:] = dy0.to(dev), dy1.to(dev)
        gu[:256], gu[M - 256:] = gu0.to(dev), gu1.to(dev)
        dgu = _poison((M, 2 * F), torch.bfloat16, dev)
        assert gu.numel() * 2 > 0xFFFFFFF0
        _run_dgrad(dy, w2.to(dev), gu, dgu, 4, 3)
        for name, rows, dy_t, gu_t in (("first", slice(0, 256), dy0, gu0),
                                       ("last", slice(M - 256, M), dy1, gu1)):
            dg, bound_dg, du, bound_du = R.dgrad_swiglu(dy_t, w2, gu_t)
            _check(f"dgrad[4GiB,{name} tile] dg", dgu[rows, :F], dg, bound_dg)
            _check(f"dgrad[4GiB,{name} tile] du", dgu[rows, F:], du, bound_du)
        assert torch.count_nonzero(dgu[256:M - 256]).item() == 0
    finally:
        del dy, gu, dgu
        torch.cuda.empty_cache()


# ---- up-projection with SwiGLU ----------------------------------------------
@functools.lru_cache(maxsize=None)
def _w13_case(M, F, K, family):
    inputs = R.w13_inputs(M, F, K, family)
    return inputs, R.w13_swiglu(*inputs)


def _run_w13(x, w13, sched):
    L = _lib.lib()
    M, K = x.shape
    F = w13.shape[0] // 2
    gu = _poison((M, 2 * F), torch.bfloat16, x.device)
    h = _poison((M, F), torch.bfloat16, x.device)
    try:
        L.mxk_gemm_w13_set_sched(sched)
        st = L.mxk_gemm_bf16_w13_swiglu(x.data_ptr(), w13.data_ptr(), gu.data_ptr(), h.data_ptr(), M, F,
                                        K, K, K, 2 * F, F, _lib.stream_ptr(x.device))
    finally:
        L.mxk_gemm_w13_set_sched(0)
    _lib.check(st, f"w13_swiglu sched {sched}")
    torch.cuda.synchronize()
    return gu, h


@pytest.mark.parametrize("sched", [0, 1, 2, 3])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("K", [64, 128, 192, 256, 320, 448])
@pytest.mark.parametrize("M,F", [(256, 128), (512, 384)])
def test_w13_swiglu_elementwise(cuda_device, M, F, K, family, sched):
    """gu and h of every K loop (0 the default; 1-3 the experiments
    library's records) over 1-7 K-tiles; gu of schedules 1 and 2 bit-equal to
    the default's (the same accumulation order)."""
    if sched and not _lib.lib().mxk_gemm_bf16_tn_variant_built(54):
        pytest.skip("A/B record: experiments library only")
    (x, w13), (gu, bound_gu, h, bound_h) = _w13_case(M, F, K, family)
    if family == "tight":
        _check_sharp("gu", gu, bound_gu)
        _check_sharp("h", h, bound_h)
    x_d, w_d = x.to(cuda_device), w13.to(cuda_device)
    got_gu, got_h = _run_w13(x_d, w_d, sched)
    tag = f"w13[{M}x{F}x{K},{family},sched{sched}]"
    _check(f"{tag} gu", got_gu, gu, bound_gu)
    _check(f"{tag} h", got_h, h, bound_h)
    if sched in (1, 2):
        assert torch.equal(_bits(got_gu), _bits(_run_w13(x_d, w_d, 0)[0])), f"{tag}: gu bits"
