"""What the MXFP8 and MXFP4 linear-layer tests share (``test_mxfp8_linear_cpu.py``,
``test_mxfp4_linear_cpu.py``, ``test_gpu_mxfp8_linear.py``,
``test_gpu_mxfp4_linear.py``): one description per format and the check bodies
written once against it.  Test names, parametrisations and the docstrings that
justify a format's thresholds stay in the test files.  A plain helper module,
not collected.
"""
import json
import types
from dataclasses import dataclass

import pytest
import torch

import mx_gemm_checks as mx
import mxk8s.ops.linear as LIN
import mxk8s.ops.mxfp4 as MX4
import mxk8s.ops.mxfp8 as MX8
from mxk8s.models.llama import Llama, LlamaConfig
from mxk8s.ops import _lib
from mxk8s.ops.linear import Linear, SwiGLULinear


@dataclass(frozen=True)
class LinearFormat:
    base: mx.Format           # name, reference quantiser, dequantiser, q dtype, codes per byte
    ops: types.ModuleType     # the ops module; its functions are looked up at every call, as
    other: types.ModuleType   # mxk8s.ops.linear does, so that a monkeypatch is seen; the other format's
    store_bytes: int          # a lane's packed store: q and qt rows aligned to less go by byte
    # paddings (bytes) that leave rows unaligned to store_bytes: qt alone, then
    # (x | its contiguous copy "xa", qt padding, q padding) for the dual kernel
    unaligned_qtpad: int
    unaligned_dual: tuple
    short_ldqt: int           # a qt row stride below that of 32 rows of x
    loss_tol: float           # tiny model against the fp32 model: |loss difference| below this,
    min_cos: float            # every gradient's cosine at least this (the test files say why)

    @property
    def name(self):
        return self.base.name

    @property
    def other_name(self):
        return "mxfp4" if self.name == "mxfp8" else "mxfp8"

    def op(self, pattern):
        return getattr(self.ops, pattern % self.name)

    quantize = property(lambda self: self.op("quantize_%s"))
    quantize_t = property(lambda self: self.op("quantize_%s_t"))
    quantize_dual = property(lambda self: self.op("quantize_%s_dual"))
    gemm_name = property(lambda self: "gemm_%s_tn" % self.name)
    linear = property(lambda self: getattr(LIN, "linear_" + self.name))
    is_linear_shape = property(lambda self: getattr(LIN, "is_%s_linear_shape" % self.name))

    def entry(self, suffix):
        return getattr(_lib.lib(), "mxk_quantize_%s%s" % (self.name, suffix))

    def code_bytes(self, n):
        return n // self.base.per_byte


MXFP8 = LinearFormat(mx.MXFP8, MX8, MX4, 8, 3, (("x", 16, 16), ("x", 5, 5), ("xa", 5, 5)), 16,
                     loss_tol=0.05, min_cos=0.9)
MXFP4 = LinearFormat(mx.MXFP4, MX4, MX8, 4, 3,
                     (("x", 16, 16), ("x", 3, 16), ("xa", 3, 16), ("xa", 16, 5), ("xa", 3, 5)), 8,
                     loss_tol=0.1, min_cos=0.7)


def _bytes(t):
    return t.contiguous().view(torch.uint8).cpu()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bytes(a), _bytes(b))


@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the kernel library was loaded")
    monkeypatch.setattr(_lib, "lib", boom)


def _counting(monkeypatch, f, record):
    """The format's GEMM op with record(args, kwargs) before every call."""
    real = getattr(f.ops, f.gemm_name)
    monkeypatch.setattr(f.ops, f.gemm_name, lambda *a, **k: record(a, k) or real(*a, **k))


def operands(T, i, o, seed, dev="cpu"):
    """bf16 x, W and a gradient whose 32 x 32 blocks carry exponents 2^-6 .. 2^6,
    so its scales differ along both axes."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand((T, i), generator=g) * 2 - 1).bfloat16()
    w = (torch.randn((o, i), generator=g) * 0.05).bfloat16()
    e = torch.randint(-6, 7, (T // 32, o // 32), generator=g).float()
    dy = (torch.rand((T, o), generator=g) * 2 - 1) * \
        torch.exp2(e).repeat_interleave(32, 0).repeat_interleave(32, 1)
    return x.to(dev), w.to(dev), dy.bfloat16().to(dev)


def main_grad_weight(w, i, o):
    """w as a parameter with the trainer's main_grad protocol: a view into a
    wider NaN buffer, marked fresh; returns (parameter, buffer, ready calls)."""
    wp = w.clone().requires_grad_()
    buf = torch.full((o, i + 8), float("nan"), dtype=torch.bfloat16, device=w.device)
    wp.main_grad = buf[:, :i]
    wp._mxk_grad_fresh = True
    ready = []
    wp._mxk_grad_ready = lambda: ready.append(1)
    return wp, buf, ready


# ---- CPU: transposed quantiser, reference path and contract --------------------------
def _wide(rows, cols, seed, lo=-40, hi=40):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, cols), generator=g)
    e = torch.randint(lo, hi, (rows, cols), generator=g)
    return torch.ldexp(x, e).bfloat16()


def cpu_quantize_t_is_the_reference_of_the_transposed_copy(f, R, C):
    x = _wide(R, C, 11 + R + C)
    qt, st = f.quantize_t(x)
    qr, sr = f.base.quantize_ref(x.t().contiguous())
    assert qt.dtype == f.base.q_dtype and st.dtype == torch.uint8
    assert qt.shape == (C, f.code_bytes(R)) and st.shape == (C, R // 32)
    assert _same(qt, qr) and _same(st, sr)
    wide = torch.zeros((R, C + 5), dtype=torch.bfloat16)
    wide[:, 2:C + 2] = x
    qt2, st2 = f.quantize_t(wide[:, 2:C + 2])               # a row stride larger than C
    assert _same(qt2, qr) and _same(st2, sr)


def cpu_quantize_dual_is_both_references(f):
    x = _wide(96, 64, 12)
    q, s, qt, st = f.quantize_dual(x)
    qr, sr = f.base.quantize_ref(x)
    qtr, str_ = f.base.quantize_ref(x.t().contiguous())
    assert q.dtype == qt.dtype == f.base.q_dtype and s.dtype == st.dtype == torch.uint8
    assert _same(q, qr) and _same(s, sr) and _same(qt, qtr) and _same(st, str_)


def quantize_t_contract_raises_before_the_library(f, dev):
    bf = dict(dtype=torch.bfloat16, device=dev)
    for fn in (f.quantize_t, f.quantize_dual):
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
        f.quantize_dual(torch.zeros((32, 48), **bf))                     # C % 32, dual only
    with pytest.raises(ValueError):
        f.quantize_t(torch.zeros((32, 0), **bf))


# ---- CPU: linear_<format> --------------------------------------------------------------
def by_hand(f, x2, w, dy2):
    """The three products from the reference quantiser, the fp32 product of the
    dequantised operands rounded to bf16 (the GEMM's CPU definition)."""
    def mm(a, b):
        return (f.base.dequantize(*a) @ f.base.dequantize(*b).t()).bfloat16()
    q = lambda m: f.base.quantize_ref(m.contiguous())                    # noqa: E731
    return mm(q(x2), q(w)), mm(q(dy2), q(w.t())), mm(q(dy2.t()), q(x2.t()))


def linear_cpu_equals_the_products_by_hand(f, T, i, o):
    x, w, dy = operands(T, i, o, 21)
    x3 = x.reshape(2, T // 2, i).clone().requires_grad_()
    wp = w.clone().requires_grad_()
    y = f.linear(x3, wp)
    assert y.shape == (2, T // 2, o) and y.dtype == torch.bfloat16
    y.backward(dy.reshape(2, T // 2, o))
    ry, rdx, rdw = by_hand(f, x, w, dy)
    assert torch.equal(y.detach().reshape(T, o), ry)
    assert torch.equal(x3.grad.reshape(T, i), rdx)
    assert torch.equal(wp.grad, rdw)


def linear_casts_other_dtypes_and_strided_dy(f):
    T, i, o = 256, 256, 256
    x, w, dy = operands(T, i, o, 22)
    xf = x.float().requires_grad_()
    wf = w.float().requires_grad_()
    y = f.linear(xf, wf)
    assert y.dtype == torch.float32
    # dy with a non-unit last stride (made contiguous) through a transposed consumer
    y.t().backward(dy.float().t().contiguous())
    ry, rdx, rdw = by_hand(f, x, w, dy)
    assert torch.equal(y.detach(), ry.float())
    assert xf.grad.dtype == torch.float32 and torch.equal(xf.grad, rdx.float())
    assert wf.grad.dtype == torch.float32 and torch.equal(wf.grad, rdw.float())


def only_the_needed_gradients_are_computed(f, monkeypatch):
    T, i, o = 256, 256, 256
    x, w, dy = operands(T, i, o, 23)
    calls = []
    _counting(monkeypatch, f, lambda a, k: calls.append(1))
    _, rdx, rdw = by_hand(f, x, w, dy)
    xg = x.clone().requires_grad_()
    f.linear(xg, w).backward(dy)
    assert torch.equal(xg.grad, rdx) and len(calls) == 2
    wg = w.clone().requires_grad_()
    f.linear(x, wg).backward(dy)
    assert torch.equal(wg.grad, rdw) and len(calls) == 4


def dy_is_read_once_when_both_gradients_are_needed(f, monkeypatch):
    T, i, o = 256, 256, 256
    x, w, dy = operands(T, i, o, 27)
    seen = []
    names = ["quantize_" + f.name + sfx for sfx in ("", "_t", "_dual")]
    for name in names:
        real = getattr(f.ops, name)
        monkeypatch.setattr(f.ops, name, lambda t, _n=name, _r=real: seen.append((_n, t.shape)) or _r(t))
    y = f.linear(x.clone().requires_grad_(), w.clone().requires_grad_())
    del seen[:]
    y.backward(dy)
    assert sorted(seen) == sorted([(names[2], (T, o)), (names[1], (o, i)), (names[1], (T, i))])


def main_grad_fresh_overwrites_then_accumulates(f):
    T, i, o = 256, 256, 256
    x, w, dy = operands(T, i, o, 24)
    x2, _, dy2 = operands(T, i, o, 25)
    wp, buf, ready = main_grad_weight(w, i, o)
    xg = x.clone().requires_grad_()
    f.linear(xg, wp).backward(dy)
    _, rdx, rdw = by_hand(f, x, w, dy)
    assert wp.grad is None and ready == [1] and wp._mxk_grad_fresh is False
    assert torch.equal(wp.main_grad, rdw)                    # the NaNs are overwritten
    assert torch.isnan(buf[:, i:]).all()                     # the padding is not
    assert torch.equal(xg.grad, rdx)
    f.linear(x2, wp).backward(dy2)
    _, _, rdw2 = by_hand(f, x2, w, dy2)
    assert wp.grad is None and ready == [1, 1]
    assert torch.equal(wp.main_grad, rdw + rdw2)             # bf16 add_, as the op does


def without_main_grad_the_weight_gradient_is_returned(f):
    T, i, o = 256, 256, 256
    x, w, dy = operands(T, i, o, 26)
    wp = w.clone().requires_grad_()
    f.linear(x, wp).backward(dy)
    assert torch.equal(wp.grad, by_hand(f, x, w, dy)[2])


# ---- CPU: shape fallback -----------------------------------------------------------------
def is_linear_shape(f):
    assert f.is_linear_shape(256, 256, 256) and f.is_linear_shape(16384, 4096, 28672)
    for bad in [(100, 256, 256), (256, 384, 256), (256, 256, 128), (0, 256, 256), (256, 0, 256)]:
        assert not f.is_linear_shape(*bad), bad


def linear_falls_back_to_bf16_on_other_shapes(f, monkeypatch, T, i):
    def boom(*a, **k):
        raise AssertionError("the %s GEMM ran" % f.name)
    monkeypatch.setattr(f.ops, f.gemm_name, boom)
    torch.manual_seed(3)
    mxl = Linear(i, 256, compute=f.name).bfloat16()
    bf = Linear(i, 256).bfloat16()
    bf.load_state_dict(mxl.state_dict())
    x = torch.randn(T, i).bfloat16()
    dy = torch.randn(T, 256).bfloat16()
    outs = []
    for m in (mxl, bf):
        xg = x.clone().requires_grad_()
        y = m(xg)
        y.backward(dy)
        outs.append((y.detach(), xg.grad, m.weight.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="multiples of 256"):
        f.linear(x, mxl.weight)


def linear_compute_argument(f):
    assert Linear(256, 256).compute == "bf16"
    assert Linear(256, 256, compute=f.name).compute == f.name
    assert SwiGLULinear(256, 256, compute=f.name).compute == f.name
    assert LlamaConfig(linear_dtype=f.name).linear_dtype == f.name
    with pytest.raises(ValueError):
        Linear(256, 256, compute="fp4")
    with pytest.raises(ValueError):
        LlamaConfig(linear_dtype="fp4")
    with pytest.raises(ValueError):
        f.linear(torch.zeros(256, 512), torch.zeros(256, 256))           # in mismatch


def swiglu_linear_is_the_plain_composition(f):
    from mxk8s.ops.fused import swiglu
    torch.manual_seed(4)
    m = SwiGLULinear(256, 256, compute=f.name).bfloat16()
    gu = torch.randn(256, 512).bfloat16()
    assert torch.equal(m(gu), f.linear(swiglu(gu), m.weight))


# ---- CPU: model wiring -------------------------------------------------------------------
def tiny_pair(f):
    """fp32 tiny Llama with bf16 linears and its MX twin on the same weights and
    tokens, after one forward + backward each; the GEMM calls of both MX formats
    counted: (ref, mx, losses, this format's calls, the other format's)."""
    torch.manual_seed(0)
    ref = Llama(LlamaConfig.tiny())
    cfg = LlamaConfig.tiny()
    cfg.linear_dtype = f.name
    mxm = Llama(cfg)
    mxm.load_state_dict(ref.state_dict())
    tok = torch.randint(0, cfg.vocab_size, (2, 129))                     # T = 256
    calls = {"ref": [], "mx": []}
    other_calls = []
    state = {"key": None, "in_lm_head": False}
    other_name = "gemm_%s_tn" % f.other_name
    real, real_other = getattr(f.ops, f.gemm_name), getattr(f.other, other_name)

    def spy(*a, **k):
        calls[state["key"]].append(state["in_lm_head"])
        return real(*a, **k)

    def spy_other(*a, **k):
        other_calls.append(state["key"])
        return real_other(*a, **k)

    setattr(f.ops, f.gemm_name, spy)
    setattr(f.other, other_name, spy_other)
    try:
        losses = {}
        for key, m in (("ref", ref), ("mx", mxm)):
            state["key"] = key
            h1 = m.lm_head.register_forward_pre_hook(lambda *_: state.update(in_lm_head=True))
            h2 = m.lm_head.register_forward_hook(lambda *_: state.update(in_lm_head=False))
            loss = m.loss(tok)
            loss.backward()
            losses[key] = loss.item()
            h1.remove()
            h2.remove()
    finally:
        setattr(f.ops, f.gemm_name, real)
        setattr(f.other, other_name, real_other)
    return ref, mxm, losses, calls, other_calls


def model_routes_24_products_and_none_by_default(f, pair):
    ref, mxm, _, calls, other_calls = pair
    assert len(calls["mx"]) == 24                            # 2 layers x 4 linears x 3 products
    assert not any(calls["mx"])                              # none inside lm_head's forward
    assert calls["ref"] == [] and other_calls == []
    assert mxm.lm_head.compute == "bf16" and ref.layers[0].attn.wqkv.compute == "bf16"
    for layer in mxm.layers:
        assert [m.compute for m in (layer.attn.wqkv, layer.attn.wo, layer.mlp.w13,
                                    layer.mlp.w2)] == [f.name] * 4


def assert_gradients_close(f, ref, model):
    """Every gradient finite with a cosine >= f.min_cos against the fp32 model's."""
    for (n, pr), (_, pm) in zip(ref.named_parameters(), model.named_parameters()):
        a, b = pr.grad.double().flatten(), pm.grad.double().cpu().flatten()
        assert torch.isfinite(b).all(), n
        cos = (a @ b / (a.norm() * b.norm())).item()
        print(n, round(cos, 5))
        assert cos >= f.min_cos, (n, cos)


def model_loss_and_gradients_against_the_fp32_model(f, pair):
    ref, mxm, losses, _, _ = pair
    print("loss", losses)
    assert abs(losses["ref"] - losses["mx"]) < f.loss_tol, losses
    assert_gradients_close(f, ref, mxm)


# ---- CPU: trainer switch -----------------------------------------------------------------
TINY_ARGV = ["--tiny", "--steps", "1", "--warmup", "0", "--seq-len", "128", "--micro-batch", "2"]


def bench_namespace():
    """bench.py's namespace: no linear_dtype attribute."""
    return types.SimpleNamespace(steps=1, warmup=0, seq_len=128, micro_batch=2, layers=None, tiny=True)


def _trainer_env(monkeypatch, env=None):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MXK_LINEAR_DTYPE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


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
    _trainer_env(monkeypatch, env)
    with pytest.raises(Stop):
        if ns is not None:
            D.run_ddp_bench(ns)
        else:
            D.main(argv)
    return seen["cfg"].linear_dtype


def trainer_switch_reaches_the_config(f, monkeypatch):
    name, other = f.name, f.other_name
    assert _trainer_cfg(monkeypatch, TINY_ARGV) == "bf16"
    assert _trainer_cfg(monkeypatch, TINY_ARGV + ["--linear-dtype", name]) == name
    assert _trainer_cfg(monkeypatch, TINY_ARGV, env={"MXK_LINEAR_DTYPE": name}) == name
    # the flag wins over the environment, in both directions
    assert _trainer_cfg(monkeypatch, TINY_ARGV + ["--linear-dtype", "bf16"],
                        env={"MXK_LINEAR_DTYPE": name}) == "bf16"
    assert _trainer_cfg(monkeypatch, TINY_ARGV + ["--linear-dtype", name],
                        env={"MXK_LINEAR_DTYPE": other}) == name
    # bench.py's namespace has no linear_dtype attribute: the environment decides
    assert _trainer_cfg(monkeypatch, ns=bench_namespace(), env={"MXK_LINEAR_DTYPE": name}) == name
    assert _trainer_cfg(monkeypatch, ns=bench_namespace()) == "bf16"


def trainer_tiny_step_on_the_cpu_reports_linear_dtype(f, monkeypatch, capsys):
    import mxk8s.train.ddp_llama as D
    _trainer_env(monkeypatch)
    calls = []
    _counting(monkeypatch, f, lambda a, k: calls.append(k.get("out")))
    assert D.main(TINY_ARGV + ["--bucket-mb", "1", "--linear-dtype", f.name]) == 0
    out = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    assert out["linear_dtype"] == f.name and out["mean_loss"] == out["mean_loss"]
    assert len(calls) == 24 and sum(o is not None for o in calls) == 8   # 8 weight gradients


# ---- CPU: build hygiene ------------------------------------------------------------------
def transposing_quantiser_kernels_have_no_scratch(f):
    _, by = mx.kernel_listing(f.base)
    mx.check_quantiser_kernels(f.base, by, "quantize_tr_kernel", 4)   # {vector, element-wise} x {t, dual}


# ---- GPU: quantisers ---------------------------------------------------------------------
def _rand(shape, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.rand(shape, device=dev, generator=g) * 2 - 1


def check(c, ref):
    """max |C - ref| <= 2^-7 max |ref| (mx_gemm_checks._check), the figures printed first."""
    c = c.detach().cpu()
    print("err", (c.double() - ref).abs().max().item(), "bound", 2 ** -7 * ref.abs().max().item())
    mx._check(c, ref)


def _quant_inputs(R, C, kind, dev):
    x = _rand((R, C), dev, 41 + R + C)
    if kind == "uniform":
        return x.bfloat16()
    if kind == "wide":
        g = torch.Generator(device=dev)
        g.manual_seed(R * 7 + C)
        e = torch.randint(-130, 125, (R, C), device=dev, generator=g)
        return torch.ldexp(x, e).bfloat16()                 # bf16 subnormals to ~2^124
    if kind == "zero_blocks":                               # along the rows and along the columns
        x = x.reshape(R // 32, 32, C).clone()
        x[::2] = 0
        x[-1, 5, 0] = -0.0
        x = x.reshape(R, C)
        x[:, :32][1::2] = 0
        return x.bfloat16()
    assert kind == "strided"
    buf = torch.zeros((R, C + 24), device=dev, dtype=torch.bfloat16)
    buf[:, 8:C + 8] = x.bfloat16()
    return buf[:, 8:C + 8]                                  # row stride C + 24


def _poisoned(rows, cols, pad, fill, dev):
    buf = torch.full((rows, cols + pad), fill, dtype=torch.uint8, device=dev)
    return buf, buf[:, :cols]


def _run(f, x, dual, qtpad=16, qpad=16, spad=3):
    """The C entry point on views of wider poisoned buffers (0x7f in the code
    bytes, a NaN of e4m3, 0xff in the scales); returns the logical outputs as
    bytes after checking that the padding is unchanged."""
    R, C = x.shape
    dev = x.device
    qtb, qt = _poisoned(C, f.code_bytes(R), qtpad, 0x7f, dev)
    stb, st = _poisoned(C, R // 32, spad, 0xff, dev)
    if dual:
        qb, q = _poisoned(R, f.code_bytes(C), qpad, 0x7f, dev)
        sb, s = _poisoned(R, C // 32, spad, 0xff, dev)
        rc = f.entry("_dual")(x.data_ptr(), q.data_ptr(), s.data_ptr(), qt.data_ptr(), st.data_ptr(),
                              R, C, x.stride(0), q.stride(0), s.stride(0), qt.stride(0), st.stride(0),
                              _lib.stream_ptr(dev))
    else:
        rc = f.entry("_t")(x.data_ptr(), qt.data_ptr(), st.data_ptr(), R, C, x.stride(0),
                           qt.stride(0), st.stride(0), _lib.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.all(qtb[:, f.code_bytes(R):] == 0x7f) and torch.all(stb[:, R // 32:] == 0xff)
    if not dual:
        return qt, st
    assert torch.all(qb[:, f.code_bytes(C):] == 0x7f) and torch.all(sb[:, C // 32:] == 0xff)
    return q, s, qt, st


def _assert_rows(f, x, q, s):
    qr, sr = f.base.quantize_ref(x.cpu().contiguous())
    assert torch.equal(_bytes(s), sr)
    assert torch.equal(_bytes(q), _bytes(qr))


def _assert_t(f, x, qt, st):
    _assert_rows(f, x.t(), qt, st)


def quantize_t_bit_equal_to_reference(f, dev, R, C, kind):
    x = _quant_inputs(R, C, kind, dev)
    _assert_t(f, x, *_run(f, x, dual=False))
    qt, st = f.quantize_t(x)                                # the op: fresh outputs
    assert qt.dtype == f.base.q_dtype and st.dtype == torch.uint8
    assert qt.shape == (C, f.code_bytes(R)) and st.shape == (C, R // 32)
    _assert_t(f, x, qt, st)


def quantize_dual_bit_equal_to_reference(f, dev, R, C, kind):
    x = _quant_inputs(R, C, kind, dev)
    q0, s0 = f.quantize(x)
    for q, s, qt, st in (_run(f, x, dual=True), f.quantize_dual(x)):
        assert q.shape == (R, f.code_bytes(C)) and s.shape == (R, C // 32)
        _assert_t(f, x, qt, st)
        assert torch.equal(_bytes(q), _bytes(q0)) and torch.equal(_bytes(s), _bytes(s0))
        _assert_rows(f, x, q, s)


def _unaligned(f, n, pad):
    """Rows of n codes and pad bytes: pad 16 keeps the packed stores, another must not."""
    assert ((f.code_bytes(n) + pad) % f.store_bytes == 0) == (pad == 16)
    return pad


def quantisers_unaligned_views(f, dev, R, C):
    buf = torch.zeros((R, C + 3), device=dev, dtype=torch.bfloat16)
    buf[:, 1:C + 1] = _rand((R, C), dev, 43).bfloat16()
    x = buf[:, 1:C + 1]
    _assert_t(f, x, *_run(f, x, dual=False))
    qtpad = _unaligned(f, R, f.unaligned_qtpad)
    _assert_t(f, x, *_run(f, x, dual=False, qtpad=qtpad))
    xa = x.contiguous()
    _assert_t(f, xa, *_run(f, xa, dual=False, qtpad=qtpad))   # aligned x, unaligned qt rows
    if C % 32 == 0:
        for which, qtpad, qpad in f.unaligned_dual:
            q, s, qt, st = _run(f, {"x": x, "xa": xa}[which], dual=True, qtpad=_unaligned(f, R, qtpad),
                                qpad=_unaligned(f, C, qpad))
            _assert_t(f, x, qt, st)
            _assert_rows(f, x, q, s)


def contract_violation_launches_nothing(f, dev):
    x = torch.ones((48, 32), dtype=torch.bfloat16, device=dev)
    out = torch.full((64, 64), 0x7f, dtype=torch.uint8, device=dev)
    sc = torch.full((64, 4), 0xff, dtype=torch.uint8, device=dev)
    sp = _lib.stream_ptr(dev)
    t, dual = f.entry("_t"), f.entry("_dual")
    assert t(x.data_ptr(), out.data_ptr(), sc.data_ptr(), 48, 32, 32, 64, 4, sp) == 1   # R % 32
    assert t(x.data_ptr(), out.data_ptr(), sc.data_ptr(), 32, 32, 32, f.short_ldqt, 4, sp) == 1
    assert dual(x.data_ptr(), out.data_ptr(), sc.data_ptr(), out.data_ptr(), sc.data_ptr(), 32, 16,
                32, 64, 4, 64, 4, sp) == 1                                              # C % 32
    torch.cuda.synchronize()
    assert torch.all(out == 0x7f) and torch.all(sc == 0xff)


# ---- GPU: the three products ---------------------------------------------------------------
def _ref_products(f, x, w, dy):
    """fp64 products of the dequantised reference-quantised operands (CPU)."""
    x, w, dy = x.cpu(), w.cpu(), dy.cpu()
    d = lambda m: f.base.dequantize(*f.base.quantize_ref(m.contiguous())).double()   # noqa: E731
    return (d(x) @ d(w).t(), d(dy) @ d(w.t()).t(), d(dy.t()) @ d(x.t()).t())


def products_against_dequantised_fp64(f, dev, T, i, o):
    x, w, dy = operands(T, i, o, 61, dev)
    xg = x.reshape(2, T // 2, i).clone().requires_grad_()
    wg = w.clone().requires_grad_()
    y = f.linear(xg, wg)
    y.backward(dy.reshape(2, T // 2, o))
    ry, rdx, rdw = _ref_products(f, x, w, dy)
    assert y.shape == (2, T // 2, o) and y.dtype == torch.bfloat16
    check(y.reshape(T, o), ry)
    check(xg.grad.reshape(T, i), rdx)
    check(wg.grad, rdw)


def main_grad_fresh_then_accumulate(f, dev):
    T, i, o = 256, 512, 256
    x1, w, dy1 = operands(T, i, o, 62, dev)
    x2, _, dy2 = operands(T, i, o, 63, dev)
    wp, buf, ready = main_grad_weight(w, i, o)
    f.linear(x1.clone().requires_grad_(), wp).backward(dy1)
    r1 = _ref_products(f, x1, w, dy1)[2]
    assert wp.grad is None and ready == [1] and wp._mxk_grad_fresh is False
    check(wp.main_grad, r1)
    assert torch.isnan(buf[:, i:]).all()                    # the padding is untouched
    f.linear(x2, wp).backward(dy2)
    r2 = _ref_products(f, x2, w, dy2)[2]
    assert wp.grad is None and ready == [1, 1]
    # two bf16 products and one bf16 sum: three roundings of <= 2^-9 each
    check(wp.main_grad, r1 + r2)
    assert torch.isnan(buf[:, i:]).all()


def run_to_run_identity(f, dev):
    T, i, o = 512, 256, 768
    x, w, dy = operands(T, i, o, 64, dev)
    runs = []
    for _ in range(2):
        xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
        y = f.linear(xg, wg)
        y.backward(dy)
        runs.append([_bytes(t) for t in (y.detach(), xg.grad, wg.grad)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)                            # no atomics: bit-identical


# ---- GPU: model ----------------------------------------------------------------------------
def fp32_reference():
    torch.manual_seed(0)
    cfg = LlamaConfig.tiny()
    ref = Llama(cfg)                                        # fp32 CPU, bf16-free pure torch
    tok = torch.randint(0, cfg.vocab_size, (2, 129))        # T = 256
    loss = ref.loss(tok)
    loss.backward()
    return ref, tok, loss.item()


def _mx_model_run(f, ref, tok, dev):
    cfg = LlamaConfig.tiny()
    cfg.linear_dtype = f.name
    m = Llama(cfg)
    m.load_state_dict(ref.state_dict())
    m = m.to(dev, torch.bfloat16)
    loss = m.loss(tok.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    return m, loss


def tiny_llama_against_fp32_cpu(f, dev, reference, monkeypatch):
    ref, tok, ref_loss = reference
    calls = []
    _counting(monkeypatch, f, lambda a, k: calls.append(1))
    m, loss = _mx_model_run(f, ref, tok, dev)
    assert len(calls) == 24                                 # 2 layers x 4 linears x 3 products
    print("loss", loss.item(), "fp32", ref_loss)
    assert torch.isfinite(loss).item() and abs(loss.item() - ref_loss) < f.loss_tol
    assert_gradients_close(f, ref, m)
    _, loss2 = _mx_model_run(f, ref, tok, dev)
    assert torch.equal(loss.cpu(), loss2.cpu())             # bit for bit


def three_train_steps_leave_finite_parameters(f, dev):
    from mxk8s.train.ddp_llama import build, train_step
    cfg = LlamaConfig.tiny()
    cfg.linear_dtype = f.name
    torch.manual_seed(0)
    model, ddp, opt = build(cfg, dev, bucket_mb=1.0)
    tok = torch.randint(0, cfg.vocab_size, (2, 129), device=dev,
                        generator=torch.Generator(device=dev).manual_seed(1))
    losses = [train_step(model, ddp, opt, tok) for _ in range(3)]
    torch.cuda.synchronize()
    assert all(torch.isfinite(l).item() for l in losses)
    for n, p in model.named_parameters():
        assert torch.isfinite(p).all(), n
