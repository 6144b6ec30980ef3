"""SwiGLU fused into the MX quantisers and the one-node MX MLP, everything that
needs no GPU: the wrappers' CPU definition (the composition of the reference
ops), their argument checks, the library signatures, the kernel set of
``native/kernels/swiglu_quantize_mx.hip``, the node on CPU tensors against its
products written out by hand, and the routing of ``MLP.forward``."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest
import torch

import mx_gemm_checks as mx
import mx_linear_checks as lc
from mx_linear_checks import no_library  # noqa: F401  (fixture)
import mxk8s.models.llama as LLAMA
import mxk8s.ops.linear as LIN
from mxk8s.models.llama import LlamaConfig, MLP
from mxk8s.ops import _lib
from mxk8s.ops.fused import swiglu_bwd_ref, swiglu_ref

REPO = mx.REPO
FORMATS = [lc.MXFP8, lc.MXFP4]
IDS = [f.name for f in FORMATS]


def _gu_dh(T, F, seed):
    g = torch.Generator().manual_seed(seed)
    gu = (torch.randn((T, 2 * F), generator=g) * 3).bfloat16()
    dh = torch.ldexp(torch.randn((T, F), generator=g),
                     torch.randint(-8, 8, (T, F), generator=g)).bfloat16()
    return gu, dh


def _same(a, b):
    return all(lc._same(x, y) for x, y in zip(a, b)) and len(a) == len(b)


# ---- the wrappers on CPU tensors -------------------------------------------------------
@pytest.mark.parametrize("f", FORMATS, ids=IDS)
def test_cpu_wrappers_are_the_reference_composition(f, no_library):  # noqa: F811
    gu, dh = _gu_dh(96, 64, 1)
    h, dgu = swiglu_ref(gu), swiglu_bwd_ref(gu, dh)
    ref = f.base.quantize_ref
    assert _same(f.op("swiglu_quantize_%s")(gu), ref(h))
    assert _same(f.op("swiglu_quantize_%s_t")(gu), ref(h.t().contiguous()))
    assert _same(f.op("swiglu_bwd_quantize_%s_dual")(gu, dh), ref(dgu) + ref(dgu.t().contiguous()))
    wide = torch.zeros((96, 128 + 24), dtype=torch.bfloat16)
    wide[:, 8:136] = gu
    assert _same(f.op("swiglu_quantize_%s")(wide[:, 8:136]), ref(h))   # a row stride larger than 2F


def test_cpu_stochastic_dual_is_the_stochastic_reference(no_library):  # noqa: F811
    gu, dh = _gu_dh(64, 32, 2)
    dgu = swiglu_bwd_ref(gu, dh)
    ref = lc.MXFP4.base.quantize_ref
    for seed in (0, 2 ** 64 - 1):
        got = lc.MX4.swiglu_bwd_quantize_mxfp4_dual(gu, dh, "stochastic", seed)
        want = ref(dgu, "stochastic", seed) + ref(dgu.t().contiguous(), "stochastic", (seed + 1) % 2 ** 64)
        assert _same(got, want)
    assert not _same(lc.MX4.swiglu_bwd_quantize_mxfp4_dual(gu, dh, "stochastic", 3)[:1],
                     lc.MX4.swiglu_bwd_quantize_mxfp4_dual(gu, dh, "stochastic", 5)[:1])


def test_swiglu_bwd_ref_is_the_gradient_of_swiglu_ref():
    gu, dh = _gu_dh(32, 32, 3)
    x = gu.double().requires_grad_()
    g, u = x.chunk(2, dim=-1)
    (torch.nn.functional.silu(g) * u).backward(dh.double())
    got = swiglu_bwd_ref(gu, dh).double()
    # fp32 arithmetic and one bf16 rounding (2^-9 relative) against fp64
    assert ((got - x.grad).abs() <= 2 ** -8 * x.grad.abs() + 1e-30).all()


@pytest.mark.parametrize("f", FORMATS, ids=IDS)
def test_contract_violations_raise_before_the_library(f, no_library):  # noqa: F811
    bf = dict(dtype=torch.bfloat16)
    rows, tr, dual = (f.op("swiglu_quantize_%s"), f.op("swiglu_quantize_%s_t"),
                      f.op("swiglu_bwd_quantize_%s_dual"))
    ok_dh = torch.zeros((32, 32), **bf)
    for fn in (rows, tr, lambda gu: dual(gu, ok_dh)):
        with pytest.raises(TypeError):
            fn(torch.zeros((32, 64)))                                # fp32
        with pytest.raises(TypeError):
            fn([[0.0] * 64] * 32)
        with pytest.raises(ValueError):
            fn(torch.zeros((32, 96), **bf))                          # F % 32
        with pytest.raises(ValueError):
            fn(torch.zeros((64,), **bf))                             # rank
        with pytest.raises(ValueError):
            fn(torch.zeros((32, 128), **bf)[:, ::2])                 # inner stride
        with pytest.raises(ValueError):
            fn(torch.zeros((0, 64), **bf))
        with pytest.raises(ValueError):
            fn(torch.zeros((32, 0), **bf))
    for fn in (tr, lambda gu: dual(gu, torch.zeros((48, 32), **bf))):
        with pytest.raises(ValueError):
            fn(torch.zeros((48, 64), **bf))                          # T % 32
    assert rows(torch.zeros((48, 64), **bf))[0].shape[0] == 48       # the row form takes any T
    gu = torch.zeros((32, 64), **bf)
    with pytest.raises(TypeError):
        dual(gu, torch.zeros((32, 32)))                              # dh fp32
    with pytest.raises(TypeError):
        dual(gu, None)
    with pytest.raises(ValueError):
        dual(gu, torch.zeros((32, 64), **bf))                        # dh is [T, F]
    with pytest.raises(ValueError):
        dual(gu, torch.zeros((32, 64), **bf)[:, ::2])
    if f.name == "mxfp4":
        with pytest.raises(ValueError):
            dual(gu, ok_dh, "stochastic")                            # no seed
        with pytest.raises(ValueError):
            dual(gu, ok_dh, "nearest", 1)
        with pytest.raises(ValueError):
            dual(gu, ok_dh, "up", 1)
        with pytest.raises(ValueError):
            dual(gu, ok_dh, "stochastic", 2 ** 64)


# ---- library signatures ------------------------------------------------------------------
def test_library_signatures():
    S = _lib._SIGNATURES
    vp, lg = ctypes.c_void_p, ctypes.c_long
    for name in ("mxfp8", "mxfp4"):
        assert S["mxk_swiglu_quantize_" + name] == (ctypes.c_int, [vp] * 3 + [lg] * 5 + [vp])
        assert S["mxk_swiglu_quantize_%s_t" % name] == (ctypes.c_int, [vp] * 3 + [lg] * 5 + [vp])
        assert S["mxk_swiglu_bwd_quantize_%s_dual" % name] == (ctypes.c_int, [vp] * 6 + [lg] * 8 + [vp])
    res, args = S["mxk_swiglu_bwd_quantize_mxfp4_sr_dual"]
    rne = S["mxk_swiglu_bwd_quantize_mxfp4_dual"][1]
    assert res is ctypes.c_int and args == rne[:-1] + [ctypes.c_uint64, vp]   # the seed before the stream
    assert "mxk_swiglu_quantize_mxfp4_sr" not in S and "mxk_swiglu_bwd_quantize_mxfp8_sr_dual" not in S


# ---- build hygiene -------------------------------------------------------------------------
@pytest.mark.skipif(not mx.HIPCC, reason="no hipcc")
def test_kernels_are_seven_without_scratch_or_spills():
    """swiglu_quantize_mx.hip compiles to the row and the transposing kernel on
    E4m3 and E2m1 and the backward dual kernel on E4m3, E2m1 and E2m1Sr, and to
    nothing else; zero scratch and zero spills, read from the kernel metadata as
    mx_gemm_checks.kernel_listing reads it."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "m.s")
        subprocess.run([mx.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17",
                        "-I" + os.path.join(REPO, "native", "kernels"), "--cuda-device-only", "-S",
                        os.path.join(REPO, "native", "kernels", "swiglu_quantize_mx.hip"), "-o", out],
                       check=True, capture_output=True)
        with open(out) as fh:
            asm = fh.read()
    by = {}
    kernels = asm[asm.index("amdhsa.kernels:"):]
    for entry in kernels[:kernels.index("\namdhsa.")].split("\n  - ")[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", entry).group(1)
        by[name] = {k: int(re.search(r"\n    \.%s:\s+(\d+)" % k, entry).group(1)) for k in mx._META}
    assert len(by) == 7, sorted(by)
    # "4E4m3E" etc.: the struct's length-prefixed name, so E2m1 does not count E2m1Sr
    count = lambda kernel, fmt: sum(kernel in n and fmt in n for n in by)   # noqa: E731
    for kernel in ("swiglu_rows_kernel", "swiglu_tr_kernel", "swiglu_bwd_dual_kernel"):
        assert count(kernel, "4E4m3E") == 1 and count(kernel, "4E2m1E") == 1, sorted(by)
    assert count("swiglu_bwd_dual_kernel", "6E2m1SrE") == 1
    assert all(v == 0 for m in by.values() for v in m.values()), by


# ---- the node on CPU tensors -------------------------------------------------------------------
def _mlp_by_hand(f, x, w13, w2, dy, sr=None):
    """y, dx, dW13, dW2 of the node from the reference ops: the GEMM's CPU
    definition on reference-quantised operands, SwiGLU by swiglu_ref and
    swiglu_bwd_ref.  sr: (w13's, w2's) seeds of the stochastic gradient images."""
    def mm(a, b):
        return (f.base.dequantize(*a) @ f.base.dequantize(*b).t()).bfloat16()
    q = lambda m, *a: f.base.quantize_ref(m.contiguous(), *a)               # noqa: E731
    rows = lambda m, s: q(m) if sr is None else q(m, "stochastic", s)         # noqa: E731
    cols = lambda m, s: q(m.t()) if sr is None else q(m.t(), "stochastic", (s + 1) % 2 ** 64)  # noqa: E731
    s13, s2 = sr or (None, None)
    gu = mm(q(x), q(w13))
    h = swiglu_ref(gu)
    y = mm(q(h), q(w2))
    dh = mm(rows(dy, s2), q(w2.t()))
    dw2 = mm(cols(dy, s2), q(h.t()))
    dgu = swiglu_bwd_ref(gu, dh)
    return y, mm(rows(dgu, s13), q(w13.t())), mm(cols(dgu, s13), q(x.t())), dw2


def _mlp_operands(seed, T=256, D=256, F=256):
    x, w13, _ = lc.operands(T, D, 2 * F, seed)
    _, w2, dy = lc.operands(T, F, D, seed + 1)
    return x, w13, w2, dy


@pytest.mark.parametrize("f,rounding", [(lc.MXFP8, "nearest"), (lc.MXFP4, "nearest"),
                                        (lc.MXFP4, "stochastic")],
                         ids=["mxfp8", "mxfp4", "mxfp4-stochastic"])
def test_node_on_the_cpu_equals_its_products_by_hand(f, rounding, monkeypatch, no_library):  # noqa: F811
    x, w13, w2, dy = _mlp_operands(71)
    calls = []
    lc._counting(monkeypatch, f, lambda a, k: calls.append(1))
    xg = x.reshape(2, 128, 256).clone().requires_grad_()
    w13g, w2g = w13.clone().requires_grad_(), w2.clone().requires_grad_()
    sr = None
    if rounding == "stochastic":
        lc.MX4.sr_reseed(9, 1, 2)
        sr = (lc.MX4.sr_next(), lc.MX4.sr_next())        # w13's first
        lc.MX4.sr_reseed(9, 1, 2)
    y = LIN.swiglu_mlp_mx(xg, w13g, w2g, f.name, rounding)
    assert y.shape == (2, 128, 256) and y.dtype == torch.bfloat16 and len(calls) == 2
    y.backward(dy.reshape(2, 128, 256))
    assert len(calls) == 6
    ry, rdx, rdw13, rdw2 = _mlp_by_hand(f, x, w13, w2, dy, sr)
    assert torch.equal(y.detach().reshape(256, 256), ry)
    assert torch.equal(xg.grad.reshape(256, 256), rdx)
    assert torch.equal(w13g.grad, rdw13) and torch.equal(w2g.grad, rdw2)
    if sr is not None:                                   # explicit seeds: the same node
        xg2 = x.clone().requires_grad_()
        LIN.swiglu_mlp_mx(xg2, w13, w2, f.name, rounding, seeds=sr).backward(dy)
        assert torch.equal(xg2.grad, rdx)


@pytest.mark.parametrize("f", FORMATS, ids=IDS)
def test_node_computes_only_the_needed_products_and_keeps_main_grad(f, monkeypatch, no_library):  # noqa: F811
    x, w13, w2, dy = _mlp_operands(73)
    _, rdx, rdw13, rdw2 = _mlp_by_hand(f, x, w13, w2, dy)
    calls = []
    lc._counting(monkeypatch, f, lambda a, k: calls.append(1))
    xg = x.clone().requires_grad_()
    LIN.swiglu_mlp_mx(xg, w13, w2, f.name).backward(dy)
    assert torch.equal(xg.grad, rdx) and len(calls) == 4            # 2 forward, dh, dx
    del calls[:]
    p13, buf13, ready13 = lc.main_grad_weight(w13, 256, 512)
    p2, buf2, ready2 = lc.main_grad_weight(w2, 256, 256)
    order = []
    p13._mxk_grad_ready = lambda: order.append("w13") or ready13.append(1)
    p2._mxk_grad_ready = lambda: order.append("w2") or ready2.append(1)
    LIN.swiglu_mlp_mx(x, p13, p2, f.name).backward(dy)
    assert len(calls) == 5 and order == ["w2", "w13"]               # 2 forward, dh, dW2, dW13
    assert p13.grad is None and p2.grad is None
    assert p13._mxk_grad_fresh is False and p2._mxk_grad_fresh is False
    assert torch.equal(p13.main_grad, rdw13) and torch.equal(p2.main_grad, rdw2)
    assert torch.isnan(buf13[:, 256:]).all() and torch.isnan(buf2[:, 256:]).all()
    LIN.swiglu_mlp_mx(x, p13, p2, f.name).backward(dy)              # second micro-batch: accumulate
    assert torch.equal(p13.main_grad, rdw13 + rdw13) and torch.equal(p2.main_grad, rdw2 + rdw2)
    del calls[:]
    w2g = w2.clone().requires_grad_()
    LIN.swiglu_mlp_mx(x, w13, w2g, f.name).backward(dy)
    assert torch.equal(w2g.grad, rdw2) and len(calls) == 3          # no dh, no dgu


def test_node_saves_no_T_by_F_tensor_on_the_cpu(no_library):  # noqa: F811
    x, w13, w2, dy = _mlp_operands(75, F=512)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(tuple(t.shape)) or t, lambda t: t):
        LIN.swiglu_mlp_mx(x.clone().requires_grad_(), w13, w2, "mxfp8")
    assert sorted(saved) == sorted([(256, 256), (256, 1024), (1024, 256), (256, 512)])


def test_node_argument_checks(no_library):  # noqa: F811
    x, w13, w2, _ = _mlp_operands(77)
    with pytest.raises(ValueError):
        LIN.swiglu_mlp_mx(x, w13, w2, "bf16")
    with pytest.raises(ValueError):
        LIN.swiglu_mlp_mx(x, w13, w2, "mxfp8", "stochastic")
    with pytest.raises(ValueError):
        LIN.swiglu_mlp_mx(x, w13, w2, "mxfp4", "nearest", seeds=(2, 4))
    with pytest.raises(ValueError):
        LIN.swiglu_mlp_mx(x, w13, w2, "mxfp4", "stochastic", seeds=(2,))
    with pytest.raises(ValueError):
        LIN.swiglu_mlp_mx(x, w13, w2, "mxfp4", "stochastic", seeds=(2, -1))
    with pytest.raises(ValueError):
        LIN.swiglu_mlp_mx(x, w13[:256], w2, "mxfp8")                 # w13 is [2F, in]
    with pytest.raises(ValueError, match="multiples of 256"):
        LIN.swiglu_mlp_mx(x[:100], w13, w2, "mxfp8")


# ---- routing ---------------------------------------------------------------------------------
@pytest.mark.parametrize("f", FORMATS, ids=IDS)
def test_mlp_forward_on_the_cpu_still_runs_the_two_linears(f, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the one-node MX MLP ran on CPU tensors")
    monkeypatch.setattr(LLAMA, "swiglu_mlp_mx", boom)
    monkeypatch.setattr(LIN, "_USE_MX_FUSED_SWIGLU", True)
    cfg = LlamaConfig(dim=256, ffn_dim=256, linear_dtype=f.name)
    torch.manual_seed(5)
    mlp = MLP(cfg).bfloat16()
    x = torch.randn(256, 256).bfloat16()
    assert torch.equal(mlp(x), mlp.w2(mlp.w13(x)))


def test_the_switch_parses():
    env = LIN._mx_fused_swiglu_env
    assert env({"MXK_MX_FUSED_SWIGLU": "0"}) is False
    assert env({"MXK_MX_FUSED_SWIGLU": "1"}) is True
    assert env({}) is (LIN.MX_FUSED_SWIGLU_DEFAULT != "0")
    assert LIN.MX_FUSED_SWIGLU_DEFAULT in ("0", "1")
    assert isinstance(LIN._USE_MX_FUSED_SWIGLU, bool)
