"""SwiGLU fused into the MX quantisers (``native/kernels/swiglu_quantize_mx.hip``)
and the one-node MX MLP (``mxk8s.ops.linear.swiglu_mlp_mx``) on the GPU.

Every check is bit for bit against the unfused composition running on the same
GPU: the stand-alone SwiGLU kernels (``mxk_swiglu_fwd`` / ``mxk_swiglu_bwd``)
followed by the stand-alone quantisers, and ``Linear`` followed by
``SwiGLULinear``.  No tolerance appears anywhere in this file.
"""
import pytest
import torch

import mx_linear_checks as lc
import mxk8s.models.llama as LLAMA
import mxk8s.ops.linear as LIN
from mxk8s.models.llama import Llama, LlamaConfig
from mxk8s.ops import _lib
from mxk8s.ops.fused import swiglu_bwd, swiglu_fwd
from mxk8s.ops.linear import Linear, SwiGLULinear, swiglu_mlp_mx

pytestmark = pytest.mark.gpu

FORMATS = [lc.MXFP8, lc.MXFP4]
IDS = [f.name for f in FORMATS]
SHAPES = [(32, 32), (160, 96), (256, 256), (384, 320)]   # one block, ragged both ways, whole tiles
KINDS = ["uniform", "wide", "zero_blocks", "strided"]
SEEDS = [0x0123456789ABCDEE, 2 ** 64 - 1]               # the second: seed + 1 wraps to 0


# ---- inputs ----------------------------------------------------------------------------
def _gen(dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return g


def _uniform(shape, dev, seed):
    return torch.rand(shape, device=dev, generator=_gen(dev, seed)) * 2 - 1


def _wide(shape, dev, seed, lo, hi, span):
    """Half of the elements uniform in [-span, span], the other half with bf16
    exponents lo .. hi."""
    g = _gen(dev, seed)
    x = torch.rand(shape, device=dev, generator=g) * 2 - 1
    e = torch.randint(lo, hi + 1, shape, device=dev, generator=g)
    pick = torch.rand(shape, device=dev, generator=g) < 0.5
    return torch.where(pick, x * span, torch.ldexp(x, e))


def _inputs(T, F, kind, dev):
    """bf16 gu [T, 2F] and dh [T, F], finite."""
    seed = 1000 * T + F
    if kind == "wide":
        # exp(-g) overflows (g < -89) and underflows, h and dgu reach +-0 and ~2^60
        gu = _wide((T, 2 * F), dev, seed, -60, 30, 100.0).bfloat16()
        dh = _wide((T, F), dev, seed + 1, -20, 20, 4.0).bfloat16()
    else:
        gu = (_uniform((T, 2 * F), dev, seed)).bfloat16()
        dh = (_uniform((T, F), dev, seed + 1)).bfloat16()
    if kind == "zero_blocks":                                # along the rows and along the columns
        gu = gu.reshape(T // 32, 32, 2 * F).clone()
        gu[::2, :, :32] = 0                                  # g of the first block of every other row block
        gu[:, 1::2, F:F + 32] = 0                            # u: every other row
        gu[-1, 5, 0] = -0.0
        gu[0, 3, F + 1] = -0.0
        gu = gu.reshape(T, 2 * F)
        dh = dh.reshape(T // 32, 32, F).clone()
        dh[1::2] = 0
        dh[0, :, F - 32:] = 0
        dh[-1, 7, 2] = -0.0
        dh = dh.reshape(T, F)
    if kind == "strided":                                    # row strides 2F + 24 and F + 8
        gb = torch.zeros((T, 2 * F + 24), device=dev, dtype=torch.bfloat16)
        gb[:, 8:2 * F + 8] = gu
        hb = torch.zeros((T, F + 8), device=dev, dtype=torch.bfloat16)
        hb[:, :F] = dh
        gu, dh = gb[:, 8:2 * F + 8], hb[:, :F]
    assert torch.isfinite(gu).all() and torch.isfinite(dh).all()
    return gu, dh


def _composition(f, gu, dh, sr=()):
    """The images of the unfused ops on the GPU: ((q, s), (qt, st), (q, s, qt, st))."""
    h = swiglu_fwd(gu)
    dgu = swiglu_bwd(gu, dh)
    assert torch.isfinite(h).all() and torch.isfinite(dgu).all()
    return f.quantize(h), f.quantize_t(h), f.quantize_dual(dgu, *sr)


# ---- the entry points on views of poisoned buffers ---------------------------------------
def _entry(f, what):
    return getattr(_lib.lib(), what % f.name)


def _outputs(f, rows, cols, dev):
    """(code buffer, code view, scale buffer, scale view) of an image of a
    [rows, cols] tensor: 16 bytes of 0x7f behind every code row, 3 of 0xff
    behind every scale row."""
    qb, q = lc._poisoned(rows, f.code_bytes(cols), 16, 0x7f, dev)
    sb, s = lc._poisoned(rows, cols // 32, 3, 0xff, dev)
    return qb, q, sb, s


def _padding_unchanged(f, bufs, cols):
    qb, _, sb, _ = bufs
    return bool(torch.all(qb[:, f.code_bytes(cols):] == 0x7f) and torch.all(sb[:, cols // 32:] == 0xff))


def _equal(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.shape[0] == b.shape[0] and torch.equal(lc._bytes(a), lc._bytes(b))


def _run_entries(f, gu, dh, seed=None):
    """The three C entry points; returns the images after checking the padding."""
    T, F = dh.shape
    dev = gu.device
    sp = _lib.stream_ptr(dev)
    rows, tr = _outputs(f, T, F, dev), _outputs(f, F, T, dev)
    drows, dtr = _outputs(f, T, 2 * F, dev), _outputs(f, 2 * F, T, dev)
    rc = _entry(f, "mxk_swiglu_quantize_%s")(gu.data_ptr(), rows[1].data_ptr(), rows[3].data_ptr(), T, F,
                                             gu.stride(0), rows[1].stride(0), rows[3].stride(0), sp)
    assert rc == 0
    rc = _entry(f, "mxk_swiglu_quantize_%s_t")(gu.data_ptr(), tr[1].data_ptr(), tr[3].data_ptr(), T, F,
                                               gu.stride(0), tr[1].stride(0), tr[3].stride(0), sp)
    assert rc == 0
    dual = _entry(f, "mxk_swiglu_bwd_quantize_%s_dual" if seed is None
                  else "mxk_swiglu_bwd_quantize_%s_sr_dual")
    rc = dual(gu.data_ptr(), dh.data_ptr(), drows[1].data_ptr(), drows[3].data_ptr(), dtr[1].data_ptr(),
              dtr[3].data_ptr(), T, F, gu.stride(0), dh.stride(0), drows[1].stride(0),
              drows[3].stride(0), dtr[1].stride(0), dtr[3].stride(0), *(() if seed is None else (seed,)), sp)
    assert rc == 0
    torch.cuda.synchronize()
    assert _padding_unchanged(f, rows, F) and _padding_unchanged(f, tr, T)
    assert _padding_unchanged(f, drows, 2 * F) and _padding_unchanged(f, dtr, T)
    return (rows[1], rows[3]), (tr[1], tr[3]), (drows[1], drows[3], dtr[1], dtr[3])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,F", SHAPES)
@pytest.mark.parametrize("f", FORMATS, ids=IDS)
def test_entry_points_bit_equal_to_the_composition(cuda_device, f, T, F, kind):
    gu, dh = _inputs(T, F, kind, cuda_device)
    want = _composition(f, gu, dh)
    for got, ref in zip(_run_entries(f, gu, dh), want):
        _equal(got, ref)
    # the ops: fresh outputs, the same images
    _equal(f.op("swiglu_quantize_%s")(gu), want[0])
    _equal(f.op("swiglu_quantize_%s_t")(gu), want[1])
    _equal(f.op("swiglu_bwd_quantize_%s_dual")(gu, dh), want[2])


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T,F", SHAPES)
def test_stochastic_dual_bit_equal_to_the_composition(cuda_device, T, F, kind, seed):
    f = lc.MXFP4
    gu, dh = _inputs(T, F, kind, cuda_device)
    want = _composition(f, gu, dh, ("stochastic", seed))[2]
    _equal(_run_entries(f, gu, dh, seed)[2], want)
    _equal(f.ops.swiglu_bwd_quantize_mxfp4_dual(gu, dh, "stochastic", seed), want)


def test_stochastic_seeds_give_different_images(cuda_device):
    gu, dh = _inputs(256, 256, "uniform", cuda_device)
    a, b = (lc.MXFP4.ops.swiglu_bwd_quantize_mxfp4_dual(gu, dh, "stochastic", s) for s in SEEDS)
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[2], b[2])


def test_ops_take_the_composition_for_rows_the_kernels_refuse(cuda_device):
    """Rows that are not 16-byte aligned: the wrappers stay total and bit-equal."""
    f = lc.MXFP8
    T, F = 64, 32
    gb = torch.zeros((T, 2 * F + 3), device=cuda_device, dtype=torch.bfloat16)
    gb[:, 1:2 * F + 1] = _uniform((T, 2 * F), cuda_device, 5).bfloat16()
    gu = gb[:, 1:2 * F + 1]
    dh = _uniform((T, F), cuda_device, 6).bfloat16()
    want = _composition(f, gu, dh)
    _equal(f.ops.swiglu_quantize_mxfp8(gu), want[0])
    _equal(f.ops.swiglu_quantize_mxfp8_t(gu), want[1])
    _equal(f.ops.swiglu_bwd_quantize_mxfp8_dual(gu, dh), want[2])


def test_ops_take_overlapping_rows_and_a_single_row(cuda_device):
    """Row stride 0 (an expanded row), which the entry points refuse, takes the
    composition; one row fits the kernel whatever stride torch reports for it."""
    f = lc.MXFP8
    F = 32
    row = _uniform((1, 2 * F), cuda_device, 7).bfloat16()
    drow = _uniform((1, F), cuda_device, 8).bfloat16()
    gu, dh = row.expand(64, 2 * F), drow.expand(64, F)
    assert gu.stride(0) == 0
    want = _composition(f, gu.contiguous(), dh.contiguous())
    _equal(f.ops.swiglu_quantize_mxfp8(gu), want[0])
    _equal(f.ops.swiglu_quantize_mxfp8_t(gu), want[1])
    _equal(f.ops.swiglu_bwd_quantize_mxfp8_dual(gu, dh), want[2])
    one = gu[:1]                                             # [1, 2F] with stride 0
    _equal(f.ops.swiglu_quantize_mxfp8(one), f.quantize(swiglu_fwd(row)))


@pytest.mark.parametrize("f", FORMATS, ids=IDS)
def test_contract_violation_launches_nothing(cuda_device, f):
    dev = cuda_device
    sp = _lib.stream_ptr(dev)
    gu = torch.ones((64, 136), dtype=torch.bfloat16, device=dev)      # room for F = 64 and odd strides
    dh = torch.ones((64, 72), dtype=torch.bfloat16, device=dev)
    out = torch.full((128, 128), 0x7f, dtype=torch.uint8, device=dev)
    sc = torch.full((128, 8), 0xff, dtype=torch.uint8, device=dev)
    g, d, o, s = gu.data_ptr(), dh.data_ptr(), out.data_ptr(), sc.data_ptr()
    rows, tr, dual = (_entry(f, "mxk_swiglu_quantize_%s"), _entry(f, "mxk_swiglu_quantize_%s_t"),
                      _entry(f, "mxk_swiglu_bwd_quantize_%s_dual"))
    kb = f.store_bytes
    bad = [
        rows(g, o, s, 64, 16, 136, 128, 8, sp),                       # F % 32
        rows(g, o, s, 0, 32, 136, 128, 8, sp),                        # T == 0
        rows(g, o, s, 64, 0, 136, 128, 8, sp),                        # F == 0
        rows(g + 2, o, s, 64, 32, 136, 128, 8, sp),                   # gu not 16-B aligned
        rows(g, o, s, 64, 32, 132, 128, 8, sp),                       # ldgu % 8
        rows(g, o, s, 64, 64, 120, 128, 8, sp),                       # ldgu < 2F
        rows(g, o + 1, s, 64, 32, 136, 128, 8, sp),                   # q not aligned to a lane's store
        rows(g, o, s, 64, 32, 136, 128 - kb // 2, 8, sp),             # ldq not a multiple of it
        rows(g, o, s, 64, 64, 136, f.code_bytes(64) - kb, 8, sp),     # ldq < a row
        rows(g, o, s, 64, 64, 136, 128, 1, sp),                       # lds < F / 32
        rows(None, o, s, 64, 32, 136, 128, 8, sp), rows(g, None, s, 64, 32, 136, 128, 8, sp),
        rows(g, o, None, 64, 32, 136, 128, 8, sp),
        tr(g, o, s, 48, 32, 136, 128, 8, sp),                         # T % 32
        tr(g, o, s, 64, 16, 136, 128, 8, sp),                         # F % 32
        tr(g, o, s, 64, 32, 136, f.code_bytes(64) - kb, 8, sp),       # ldqt < T codes
        tr(g, o, s, 64, 32, 136, 128, 1, sp),                         # ldst < T / 32
        tr(g, o, s, 64, 64 * 65536, 2 * 64 * 65536, 128, 8, sp),      # grid.y
        dual(g, d, o, s, o, s, 48, 32, 136, 72, 128, 8, 128, 8, sp),  # T % 32
        dual(g, d, o, s, o, s, 64, 16, 136, 72, 128, 8, 128, 8, sp),  # F % 32
        dual(g, d + 2, o, s, o, s, 64, 32, 136, 72, 128, 8, 128, 8, sp),   # dh not aligned
        dual(g, d, o, s, o, s, 64, 32, 136, 36, 128, 8, 128, 8, sp),  # lddh % 8
        dual(g, d, o, s, o, s, 64, 64, 136, 56, 128, 8, 128, 8, sp),  # lddh < F
        dual(g, d, o, s, o, s, 64, 64, 136, 72, f.code_bytes(128) - kb, 8, 128, 8, sp),   # ldq < 2F codes
        dual(g, d, o, s, o, s, 64, 64, 136, 72, 128, 3, 128, 8, sp),  # lds < 2F / 32
        dual(g, None, o, s, o, s, 64, 32, 136, 72, 128, 8, 128, 8, sp),
        dual(g, d, o, s, None, s, 64, 32, 136, 72, 128, 8, 128, 8, sp),
    ]
    if f.name == "mxfp4":
        sr = _entry(f, "mxk_swiglu_bwd_quantize_%s_sr_dual")
        bad.append(sr(g, d, o, s, o, s, 48, 32, 136, 72, 128, 8, 128, 8, 7, sp))
        # T = 2^32: a stochastic index would not fit its counter word (2F >= 2^32 is
        # already beyond the grid limit)
        bad.append(sr(g, d, o, s, o, s, 2 ** 32, 32, 136, 72, 128, 8, 2 ** 31, 2 ** 27, 7, sp))
    torch.cuda.synchronize()
    assert bad == [1] * len(bad), bad
    assert torch.all(out == 0x7f) and torch.all(sc == 0xff)


# ---- the MLP node against Linear -> SwiGLULinear ------------------------------------------
T_, DIM, FFN = 256, 256, 512
CONFIGS = [(lc.MXFP8, "nearest"), (lc.MXFP4, "nearest"), (lc.MXFP4, "stochastic")]
CONFIG_IDS = ["mxfp8", "mxfp4", "mxfp4-stochastic"]


def _layers(f, rounding, dev):
    torch.manual_seed(7)
    w13 = Linear(DIM, 2 * FFN, compute=f.name, grad_rounding=rounding).to(dev, torch.bfloat16)
    w2 = SwiGLULinear(FFN, DIM, compute=f.name, grad_rounding=rounding).to(dev, torch.bfloat16)
    return w13, w2


def _mlp_io(dev, seed, T=T_):
    x, _, _ = lc.operands(T, DIM, DIM, seed, dev)
    _, _, dy = lc.operands(T, DIM, DIM, seed + 1, dev)
    return x, dy


def _step(fused, f, rounding, w13, w2, x, dy, need_x=True):
    """One forward + backward after the same reseed: (y, dx)."""
    lc.MX4.sr_reseed(11, 0, 3)
    xg = x.reshape(2, T_ // 2, DIM).clone().requires_grad_(need_x)
    if fused:
        y = swiglu_mlp_mx(xg, w13.weight, w2.weight, f.name, rounding)
    else:
        y = w2(w13(xg))
    y.backward(dy.reshape(2, T_ // 2, DIM))
    return y.detach().clone(), None if xg.grad is None else xg.grad.clone()


def _attach_main_grad(layer):
    o, i = layer.weight.shape
    buf = torch.full((o, i + 8), float("nan"), dtype=torch.bfloat16, device=layer.weight.device)
    layer.weight.main_grad = buf[:, :i]
    layer.weight._mxk_grad_fresh = True
    return buf


@pytest.mark.parametrize("f,rounding", CONFIGS, ids=CONFIG_IDS)
def test_mlp_node_bit_equal_to_the_two_linears(cuda_device, f, rounding, monkeypatch):
    dev = cuda_device
    w13, w2 = _layers(f, rounding, dev)
    x, dy = _mlp_io(dev, 81)
    x2, dy2 = _mlp_io(dev, 83)
    calls = []
    lc._counting(monkeypatch, f, lambda a, k: calls.append(1))
    runs = {}
    for fused in (False, True):
        for layer in (w13, w2):
            layer.weight.grad = None
        del calls[:]
        y, dx = _step(fused, f, rounding, w13, w2, x, dy)
        assert len(calls) == 6                                # 2 forward, dh, dW2, dx, dW13
        runs[fused] = [y, dx, w13.weight.grad.clone(), w2.weight.grad.clone()]
        # the trainer's protocol: overwrite a fresh main_grad, then accumulate
        bufs = [_attach_main_grad(w13), _attach_main_grad(w2)]
        ready = []
        w13.weight._mxk_grad_ready = lambda: ready.append("w13")
        w2.weight._mxk_grad_ready = lambda: ready.append("w2")
        for layer in (w13, w2):
            layer.weight.grad = None
        _step(fused, f, rounding, w13, w2, x, dy)
        assert ready == ["w2", "w13"] and w13.weight.grad is None and w2.weight.grad is None
        runs[fused] += [b.clone() for b in bufs]
        _step(fused, f, rounding, w13, w2, x2, dy2)
        assert ready == ["w2", "w13"] * 2
        runs[fused] += [b.clone() for b in bufs]
        for layer in (w13, w2):
            del layer.weight.main_grad, layer.weight._mxk_grad_fresh, layer.weight._mxk_grad_ready
    for a, b in zip(runs[False], runs[True]):
        assert torch.equal(lc._bytes(a), lc._bytes(b))        # NaN padding included
    # the first main_grad equals the returned gradient, and the second call changed it
    assert torch.equal(runs[True][4][:, :DIM], runs[True][2])
    assert torch.isnan(runs[True][4][:, DIM:]).all() and torch.isnan(runs[True][7][:, FFN:]).all()
    assert not torch.equal(runs[True][4][:, :DIM], runs[True][6][:, :DIM])


@pytest.mark.parametrize("f,rounding", CONFIGS, ids=CONFIG_IDS)
def test_mlp_node_computes_only_the_needed_products(cuda_device, f, rounding, monkeypatch):
    dev = cuda_device
    w13, w2 = _layers(f, rounding, dev)
    x, dy = _mlp_io(dev, 85)
    calls = []
    lc._counting(monkeypatch, f, lambda a, k: calls.append(1))
    out = {}
    for fused in (False, True):
        for layer in (w13, w2):                                # only x
            layer.weight.requires_grad_(False)
        del calls[:]
        y, dx = _step(fused, f, rounding, w13, w2, x, dy)
        assert len(calls) == 4                                 # 2 forward, dh, dx
        for layer in (w13, w2):                                # only the weights
            layer.weight.requires_grad_(True)
            layer.weight.grad = None
        del calls[:]
        _, none = _step(fused, f, rounding, w13, w2, x, dy, need_x=False)
        assert none is None and len(calls) == 5                # 2 forward, dh, dW2, dW13
        out[fused] = [y, dx, w13.weight.grad.clone(), w2.weight.grad.clone()]
    for a, b in zip(out[False], out[True]):
        assert torch.equal(lc._bytes(a), lc._bytes(b))


def test_mlp_node_saves_no_T_by_F_tensor(cuda_device):
    f, dev, T = lc.MXFP8, cuda_device, 512                     # no weight is [T, FFN]
    w13, w2 = _layers(f, "nearest", dev)
    x, _ = _mlp_io(dev, 87, T)
    saved = {}
    for fused in (False, True):
        shapes = saved.setdefault(fused, [])
        with torch.autograd.graph.saved_tensors_hooks(lambda t: shapes.append(tuple(t.shape)) or t,
                                                      lambda t: t):
            xg = x.clone().requires_grad_()
            if fused:
                swiglu_mlp_mx(xg, w13.weight, w2.weight, f.name)
            else:
                w2(w13(xg))
    assert (T, FFN) in saved[False]                            # the composition keeps h
    assert (T, FFN) not in saved[True]
    assert sorted(saved[True]) == sorted([(T, DIM), (T, 2 * FFN), (2 * FFN, DIM), (DIM, FFN)])


# ---- tiny Llama: the switch changes nothing ---------------------------------------------------
@pytest.fixture(scope="module")
def tiny_weights():
    torch.manual_seed(0)
    cfg = LlamaConfig.tiny()
    return Llama(cfg).state_dict(), torch.randint(0, cfg.vocab_size, (2, 129))   # T = 256


def _tiny_run(f, rounding, dev, weights, tok, fused, monkeypatch):
    monkeypatch.setattr(LIN, "_USE_MX_FUSED_SWIGLU", fused)
    nodes = []
    real = LLAMA.swiglu_mlp_mx
    monkeypatch.setattr(LLAMA, "swiglu_mlp_mx", lambda *a, **k: nodes.append(1) or real(*a, **k))
    cfg = LlamaConfig.tiny()
    cfg.linear_dtype, cfg.grad_rounding = f.name, rounding
    m = Llama(cfg)
    m.load_state_dict(weights)
    m = m.to(dev, torch.bfloat16)
    lc.MX4.sr_reseed(3, 0, 1)
    loss = m.loss(tok.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    assert len(nodes) == (cfg.n_layers if fused else 0)
    return loss.detach().reshape(1), {n: p.grad for n, p in m.named_parameters()}


@pytest.mark.parametrize("f,rounding", CONFIGS, ids=CONFIG_IDS)
def test_tiny_llama_bit_identical_with_the_switch_on_and_off(cuda_device, f, rounding, tiny_weights,
                                                             monkeypatch):
    weights, tok = tiny_weights
    calls = []
    lc._counting(monkeypatch, f, lambda a, k: calls.append(1))
    loss_off, grads_off = _tiny_run(f, rounding, cuda_device, weights, tok, False, monkeypatch)
    assert len(calls) == 24
    loss_on, grads_on = _tiny_run(f, rounding, cuda_device, weights, tok, True, monkeypatch)
    assert len(calls) == 48                                    # 24 products either way
    assert torch.isfinite(loss_on).all() and torch.equal(lc._bytes(loss_on), lc._bytes(loss_off))
    assert grads_on.keys() == grads_off.keys()
    for n in grads_on:
        assert torch.equal(lc._bytes(grads_on[n]), lc._bytes(grads_off[n])), n
