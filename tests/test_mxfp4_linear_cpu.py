"""MXFP4 linear layers, everything that needs no GPU: the transposing
quantiser's reference path, nibble order and contract, ``linear_mxfp4`` against
its three products written out by hand, the ``main_grad`` protocol, the shape
fallback of ``Linear(compute="mxfp4")``, the model and trainer wiring, build
hygiene of the new kernels."""
import json
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

import mxk8s.ops.mxfp4 as MX4
import mxk8s.ops.mxfp8 as MX8
from mxk8s.models.llama import Llama, LlamaConfig
from mxk8s.ops import (_lib, dequantize_mxfp4, is_mxfp4_linear_shape, linear_mxfp4,
                       quantize_mxfp4_dual, quantize_mxfp4_ref, quantize_mxfp4_t)
from mxk8s.ops.linear import Linear, SwiGLULinear

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _wide(rows, cols, seed, lo=-40, hi=40):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, cols), generator=g)
    e = torch.randint(lo, hi, (rows, cols), generator=g)
    return torch.ldexp(x, e).bfloat16()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the kernel library was loaded")
    monkeypatch.setattr(_lib, "lib", boom)


# ---- transposed quantiser: reference path and contract -----------------------------
@pytest.mark.parametrize("R,C", [(32, 1), (96, 3), (64, 100), (256, 32)])
def test_cpu_quantize_t_is_the_reference_of_the_transposed_copy(no_library, R, C):
    x = _wide(R, C, 11 + R + C)
    qt, st = quantize_mxfp4_t(x)
    qr, sr = quantize_mxfp4_ref(x.t().contiguous())
    assert qt.dtype == torch.uint8 and st.dtype == torch.uint8
    assert qt.shape == (C, R // 2) and st.shape == (C, R // 32)
    assert _same(qt, qr) and _same(st, sr)
    wide = torch.zeros((R, C + 5), dtype=torch.bfloat16)
    wide[:, 2:C + 2] = x
    qt2, st2 = quantize_mxfp4_t(wide[:, 2:C + 2])            # a row stride larger than C
    assert _same(qt2, qr) and _same(st2, sr)


def test_cpu_quantize_dual_is_both_references(no_library):
    x = _wide(96, 64, 12)
    q, s, qt, st = quantize_mxfp4_dual(x)
    qr, sr = quantize_mxfp4_ref(x)
    qtr, str_ = quantize_mxfp4_ref(x.t().contiguous())
    assert all(t.dtype == torch.uint8 for t in (q, s, qt, st))
    assert _same(q, qr) and _same(s, sr) and _same(qt, qtr) and _same(st, str_)


def test_nibble_order_of_the_transposed_image(no_library):
    """Byte i of row c holds x[2i][c] in bits 3:0 and x[2i+1][c] in bits 7:4.
    Column 0 counts through the e2m1 magnitudes twice with the block maximum 6
    (scale 2^0), column 1 is its negative times 4 (scale 2^2)."""
    mags = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    col = torch.tensor(mags + mags[::-1] + mags + mags[::-1])
    x = torch.stack((col, -4 * col), dim=1).bfloat16()       # [32, 2]
    codes = list(range(8)) + list(range(7, -1, -1))
    codes = codes + codes                                    # code of row r in column 0
    neg = [c | 8 if c else 0 for c in codes]                 # -0 is never produced
    want = torch.tensor([[codes[2 * i] | (codes[2 * i + 1] << 4) for i in range(16)],
                         [neg[2 * i] | (neg[2 * i + 1] << 4) for i in range(16)]], dtype=torch.uint8)
    for qt, st in (quantize_mxfp4_t(x), quantize_mxfp4_dual(x.repeat(1, 16))[2:]):
        assert torch.equal(qt[:2], want)
        assert st[:2].tolist() == [[127], [129]]
    assert qt.shape == (32, 16) and torch.equal(qt[2:4], want)   # the dual input repeats the pair


@pytest.mark.parametrize("dev", ["cpu", "meta"])
def test_quantize_t_contract_raises_before_the_library(no_library, dev):
    bf = dict(dtype=torch.bfloat16, device=dev)
    for fn in (quantize_mxfp4_t, quantize_mxfp4_dual):
        with pytest.raises(TypeError):
            fn(torch.zeros((32, 32), device=dev))                        # fp32
        with pytest.raises(TypeError):
            fn([[0.0] * 32] * 32)
        with pytest.raises(ValueError):
            fn(torch.zeros((48, 32), **bf))                              # R % 32
        with pytest.raises(ValueError):
            fn(torch.zeros((32,), **bf))                                 # rank
        with pytest.raises(ValueError):
            fn(torch.zeros((2, 32, 32), **bf))
        with pytest.raises(ValueError):
            fn(torch.zeros((32, 64), **bf)[:, ::2])                      # inner stride
        with pytest.raises(ValueError):
            fn(torch.zeros((0, 32), **bf))
    with pytest.raises(ValueError):
        quantize_mxfp4_dual(torch.zeros((32, 48), **bf))                 # C % 32, dual only
    with pytest.raises(ValueError):
        quantize_mxfp4_t(torch.zeros((32, 0), **bf))


# ---- linear_mxfp4 on the CPU ------------------------------------------------------
def _by_hand(x2, w, dy2):
    """The three products from the reference quantiser, the fp32 product of the
    dequantised operands rounded to bf16 (the GEMM's CPU definition)."""
    def mm(a, b):
        return (dequantize_mxfp4(*a) @ dequantize_mxfp4(*b).t()).bfloat16()
    t = lambda m: m.t().contiguous()                                     # noqa: E731
    y = mm(quantize_mxfp4_ref(x2), quantize_mxfp4_ref(w))
    dx = mm(quantize_mxfp4_ref(dy2), quantize_mxfp4_ref(t(w)))
    dw = mm(quantize_mxfp4_ref(t(dy2)), quantize_mxfp4_ref(t(x2)))
    return y, dx, dw


def _operands(T, i, o, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand((T, i), generator=g) * 2 - 1).bfloat16()
    w = (torch.randn((o, i), generator=g) * 0.05).bfloat16()
    e = torch.randint(-6, 7, (T // 32, o // 32), generator=g).float()
    dy = (torch.rand((T, o), generator=g) * 2 - 1) * \
        torch.exp2(e).repeat_interleave(32, 0).repeat_interleave(32, 1)
    return x, w, dy.bfloat16()


@pytest.mark.parametrize("T,i,o", [(256, 256, 256), (256, 512, 256), (512, 256, 768)])
def test_linear_mxfp4_cpu_equals_the_products_by_hand(no_library, T, i, o):
    x, w, dy = _operands(T, i, o, 21)
    x3 = x.reshape(2, T // 2, i).clone().requires_grad_()
    wp = w.clone().requires_grad_()
    y = linear_mxfp4(x3, wp)
    assert y.shape == (2, T // 2, o) and y.dtype == torch.bfloat16
    y.backward(dy.reshape(2, T // 2, o))
    ry, rdx, rdw = _by_hand(x, w, dy)
    assert torch.equal(y.detach().reshape(T, o), ry)
    assert torch.equal(x3.grad.reshape(T, i), rdx)
    assert torch.equal(wp.grad, rdw)


def test_linear_mxfp4_casts_other_dtypes_and_strided_dy(no_library):
    T, i, o = 256, 256, 256
    x, w, dy = _operands(T, i, o, 22)
    xf = x.float().requires_grad_()
    wf = w.float().requires_grad_()
    y = linear_mxfp4(xf, wf)
    assert y.dtype == torch.float32
    # dy with a non-unit last stride (made contiguous) through a transposed consumer
    y.t().backward(dy.float().t().contiguous())
    ry, rdx, rdw = _by_hand(x, w, dy)
    assert torch.equal(y.detach(), ry.float())
    assert xf.grad.dtype == torch.float32 and torch.equal(xf.grad, rdx.float())
    assert wf.grad.dtype == torch.float32 and torch.equal(wf.grad, rdw.float())


def test_only_the_needed_gradients_are_computed(no_library, monkeypatch):
    T, i, o = 256, 256, 256
    x, w, dy = _operands(T, i, o, 23)
    calls = []
    real = MX4.gemm_mxfp4_tn
    monkeypatch.setattr(MX4, "gemm_mxfp4_tn", lambda *a, **k: calls.append(1) or real(*a, **k))
    _, rdx, rdw = _by_hand(x, w, dy)
    xg = x.clone().requires_grad_()
    linear_mxfp4(xg, w).backward(dy)
    assert torch.equal(xg.grad, rdx) and len(calls) == 2
    wg = w.clone().requires_grad_()
    linear_mxfp4(x, wg).backward(dy)
    assert torch.equal(wg.grad, rdw) and len(calls) == 4


def test_dy_is_read_once_when_both_gradients_are_needed(no_library, monkeypatch):
    T, i, o = 256, 256, 256
    x, w, dy = _operands(T, i, o, 27)
    seen = []
    for name in ("quantize_mxfp4", "quantize_mxfp4_t", "quantize_mxfp4_dual"):
        real = getattr(MX4, name)
        monkeypatch.setattr(MX4, name, lambda t, _n=name, _r=real: seen.append((_n, t.shape)) or _r(t))
    y = linear_mxfp4(x.clone().requires_grad_(), w.clone().requires_grad_())
    del seen[:]
    y.backward(dy)
    assert sorted(seen) == sorted([("quantize_mxfp4_dual", (T, o)), ("quantize_mxfp4_t", (o, i)),
                                   ("quantize_mxfp4_t", (T, i))])


# ---- main_grad protocol -----------------------------------------------------------
def test_main_grad_fresh_overwrites_then_accumulates(no_library):
    T, i, o = 256, 256, 256
    x, w, dy = _operands(T, i, o, 24)
    x2, _, dy2 = _operands(T, i, o, 25)
    wp = w.clone().requires_grad_()
    buf = torch.full((o, i + 8), float("nan"), dtype=torch.bfloat16)
    wp.main_grad = buf[:, :i]
    wp._mxk_grad_fresh = True
    ready = []
    wp._mxk_grad_ready = lambda: ready.append(1)
    xg = x.clone().requires_grad_()
    linear_mxfp4(xg, wp).backward(dy)
    _, rdx, rdw = _by_hand(x, w, dy)
    assert wp.grad is None and ready == [1] and wp._mxk_grad_fresh is False
    assert torch.equal(wp.main_grad, rdw)                    # the NaNs are overwritten
    assert torch.isnan(buf[:, i:]).all()                     # the padding is not
    assert torch.equal(xg.grad, rdx)
    linear_mxfp4(x2, wp).backward(dy2)
    _, _, rdw2 = _by_hand(x2, w, dy2)
    assert wp.grad is None and ready == [1, 1]
    assert torch.equal(wp.main_grad, rdw + rdw2)             # bf16 add_, as the op does


def test_without_main_grad_the_weight_gradient_is_returned(no_library):
    T, i, o = 256, 256, 256
    x, w, dy = _operands(T, i, o, 26)
    wp = w.clone().requires_grad_()
    linear_mxfp4(x, wp).backward(dy)
    assert torch.equal(wp.grad, _by_hand(x, w, dy)[2])


# ---- shape fallback ---------------------------------------------------------------
def test_is_mxfp4_linear_shape():
    assert is_mxfp4_linear_shape(256, 256, 256) and is_mxfp4_linear_shape(16384, 4096, 28672)
    for bad in [(100, 256, 256), (256, 384, 256), (256, 256, 128), (0, 256, 256), (256, 0, 256)]:
        assert not is_mxfp4_linear_shape(*bad), bad


@pytest.mark.parametrize("T,i", [(100, 256), (256, 384)])
def test_linear_falls_back_to_bf16_on_other_shapes(no_library, monkeypatch, T, i):
    def boom(*a, **k):
        raise AssertionError("the MXFP4 GEMM ran")
    monkeypatch.setattr(MX4, "gemm_mxfp4_tn", boom)
    torch.manual_seed(3)
    mx = Linear(i, 256, compute="mxfp4").bfloat16()
    bf = Linear(i, 256).bfloat16()
    bf.load_state_dict(mx.state_dict())
    x = torch.randn(T, i).bfloat16()
    dy = torch.randn(T, 256).bfloat16()
    outs = []
    for m in (mx, bf):
        xg = x.clone().requires_grad_()
        y = m(xg)
        y.backward(dy)
        outs.append((y.detach(), xg.grad, m.weight.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="multiples of 256"):
        linear_mxfp4(x, mx.weight)


def test_linear_compute_argument():
    assert Linear(256, 256, compute="mxfp4").compute == "mxfp4"
    assert SwiGLULinear(256, 256, compute="mxfp4").compute == "mxfp4"
    assert LlamaConfig(linear_dtype="mxfp4").linear_dtype == "mxfp4"
    with pytest.raises(ValueError):
        Linear(256, 256, compute="fp4")
    with pytest.raises(ValueError):
        linear_mxfp4(torch.zeros(256, 512), torch.zeros(256, 256))       # in mismatch


def test_swiglu_linear_mxfp4_is_the_plain_composition(no_library):
    from mxk8s.ops.fused import swiglu
    torch.manual_seed(4)
    m = SwiGLULinear(256, 256, compute="mxfp4").bfloat16()
    gu = torch.randn(256, 512).bfloat16()
    assert torch.equal(m(gu), linear_mxfp4(swiglu(gu), m.weight))


# ---- model wiring -----------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_pair():
    """fp32 tiny Llama with bf16 linears and its MXFP4 twin on the same weights
    and tokens, after one forward + backward each; the GEMM calls of both MX
    formats counted."""
    torch.manual_seed(0)
    ref = Llama(LlamaConfig.tiny())
    cfg = LlamaConfig.tiny()
    cfg.linear_dtype = "mxfp4"
    mx = Llama(cfg)
    mx.load_state_dict(ref.state_dict())
    tok = torch.randint(0, cfg.vocab_size, (2, 129))                     # T = 256
    calls = {"ref": [], "mx": []}
    fp8_calls = []
    state = {"key": None, "in_lm_head": False}
    real4, real8 = MX4.gemm_mxfp4_tn, MX8.gemm_mxfp8_tn

    def spy(*a, **k):
        calls[state["key"]].append(state["in_lm_head"])
        return real4(*a, **k)

    def spy8(*a, **k):
        fp8_calls.append(state["key"])
        return real8(*a, **k)

    MX4.gemm_mxfp4_tn, MX8.gemm_mxfp8_tn = spy, spy8
    try:
        losses = {}
        for key, m in (("ref", ref), ("mx", mx)):
            state["key"] = key
            h1 = m.lm_head.register_forward_pre_hook(lambda *_: state.update(in_lm_head=True))
            h2 = m.lm_head.register_forward_hook(lambda *_: state.update(in_lm_head=False))
            loss = m.loss(tok)
            loss.backward()
            losses[key] = loss.item()
            h1.remove()
            h2.remove()
    finally:
        MX4.gemm_mxfp4_tn, MX8.gemm_mxfp8_tn = real4, real8
    return ref, mx, losses, calls, fp8_calls


def test_model_routes_24_products_and_none_by_default(tiny_pair):
    ref, mx, _, calls, fp8_calls = tiny_pair
    assert len(calls["mx"]) == 24                            # 2 layers x 4 linears x 3 products
    assert not any(calls["mx"])                              # none inside lm_head's forward
    assert calls["ref"] == [] and fp8_calls == []
    assert mx.lm_head.compute == "bf16" and ref.layers[0].attn.wqkv.compute == "bf16"
    for layer in mx.layers:
        assert [m.compute for m in (layer.attn.wqkv, layer.attn.wo, layer.mlp.w13,
                                    layer.mlp.w2)] == ["mxfp4"] * 4


def test_model_loss_and_gradients_against_the_fp32_model(tiny_pair):
    """Plumbing conditions, not accuracy claims: |loss - loss_fp32| < 0.1, every
    gradient finite with a cosine >= 0.7 against the fp32 model.  The reference
    emulation alone, measured on the CPU over seeds 0-3, gives loss differences
    of 0.001-0.030 and worst cosines of 0.844-0.867 (e2m1 has one mantissa bit),
    while a dropped or garbage product gives a cosine near 0."""
    ref, mx, losses, _, _ = tiny_pair
    print("loss", losses)
    assert abs(losses["ref"] - losses["mx"]) < 0.1, losses
    for (n, pr), (_, pm) in zip(ref.named_parameters(), mx.named_parameters()):
        a, b = pr.grad.double().flatten(), pm.grad.double().flatten()
        cos = (a @ b / (a.norm() * b.norm())).item()
        print(n, round(cos, 5))
        assert torch.isfinite(b).all() and cos >= 0.7, (n, cos)


# ---- trainer switch -----------------------------------------------------------------
def _trainer_cfg(monkeypatch, argv=None, env=None, ns=None):
    """cfg.linear_dtype as the trainer's build() receives it (CPU, one rank)."""
    import mxk8s.train.ddp_llama as D
    seen = {}

    class Stop(Exception):
        pass

    def fake_build(cfg, *a, **k):
        seen["cfg"] = cfg
        raise Stop

    monkeypatch.setattr(D, "build", fake_build)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MXK_LINEAR_DTYPE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    with pytest.raises(Stop):
        if ns is not None:
            D.run_ddp_bench(ns)
        else:
            D.main(argv)
    return seen["cfg"].linear_dtype


def test_trainer_switch_reaches_the_config(monkeypatch):
    tiny = ["--tiny", "--steps", "1", "--warmup", "0", "--seq-len", "128", "--micro-batch", "2"]
    assert _trainer_cfg(monkeypatch, tiny + ["--linear-dtype", "mxfp4"]) == "mxfp4"
    assert _trainer_cfg(monkeypatch, tiny, env={"MXK_LINEAR_DTYPE": "mxfp4"}) == "mxfp4"
    # the flag wins over the environment, in both directions
    assert _trainer_cfg(monkeypatch, tiny + ["--linear-dtype", "bf16"],
                        env={"MXK_LINEAR_DTYPE": "mxfp4"}) == "bf16"
    assert _trainer_cfg(monkeypatch, tiny + ["--linear-dtype", "mxfp4"],
                        env={"MXK_LINEAR_DTYPE": "mxfp8"}) == "mxfp4"
    # bench.py's namespace has no linear_dtype attribute: the environment decides
    ns = types.SimpleNamespace(steps=1, warmup=0, seq_len=128, micro_batch=2, layers=None, tiny=True)
    assert _trainer_cfg(monkeypatch, ns=ns, env={"MXK_LINEAR_DTYPE": "mxfp4"}) == "mxfp4"
    assert _trainer_cfg(monkeypatch, ns=ns) == "bf16"


def test_trainer_tiny_step_on_the_cpu_reports_linear_dtype(monkeypatch, capsys):
    """One CPU step of the tiny model through FlatDDP with MXFP4 linears: the
    weight gradients go into the flat buffer through out=."""
    import mxk8s.train.ddp_llama as D
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MXK_LINEAR_DTYPE"):
        monkeypatch.delenv(k, raising=False)
    calls = []
    real = MX4.gemm_mxfp4_tn
    monkeypatch.setattr(MX4, "gemm_mxfp4_tn", lambda *a, **k: calls.append(k.get("out")) or real(*a, **k))
    assert D.main(["--tiny", "--steps", "1", "--warmup", "0", "--seq-len", "128", "--micro-batch", "2",
                   "--bucket-mb", "1", "--linear-dtype", "mxfp4"]) == 0
    out = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    assert out["linear_dtype"] == "mxfp4" and out["mean_loss"] == out["mean_loss"]
    assert len(calls) == 24 and sum(o is not None for o in calls) == 8   # 8 weight gradients


# ---- build hygiene ------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC) and not shutil.which("hipcc"), reason="no hipcc")
def test_transposing_quantiser_kernels_have_no_scratch(tmp_path):
    out = str(tmp_path / "m.s")
    subprocess.run([HIPCC if os.path.exists(HIPCC) else "hipcc", "--offload-arch=gfx950", "-O3",
                    "-std=c++17", "-I" + os.path.join(REPO, "native", "kernels"),
                    "--cuda-device-only", "-S",
                    os.path.join(REPO, "native", "kernels", "quantize_mxfp4_tr.hip"), "-o", out],
                   check=True, capture_output=True)
    with open(out) as f:
        asm = f.read()
    meta = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", asm)
    by = {n: int(v) for n, v in meta}
    assert len(by) == 4 and all("quantize_mxfp4_tr_kernel" in n for n in by), by
    assert all(v == 0 for v in by.values()), by              # {vector, element-wise} x {t, dual}
    spills = re.findall(r"\.(?:vgpr|sgpr)_spill_count:\s+(\d+)", asm)
    assert len(spills) == 8 and all(int(x) == 0 for x in spills), spills
