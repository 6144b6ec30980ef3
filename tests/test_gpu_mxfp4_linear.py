"""Transposing MXFP4 quantiser and ``linear_mxfp4`` on the GPU
(``native/kernels/quantize_mxfp4_tr.hip``, ``mxk8s/ops/linear.py``).

The quantisers are bit-equal to the reference, so the products are compared
with the fp64 product of the dequantised *reference-quantised* operands under
the project's bf16-output criterion (``mx_gemm_checks._check``).
"""
import pytest
import torch

import mx_gemm_checks as mx
import mxk8s.ops.mxfp4 as MX
from mxk8s.models.llama import Llama, LlamaConfig
from mxk8s.ops import (_lib, dequantize_mxfp4, linear_mxfp4, quantize_mxfp4, quantize_mxfp4_dual,
                       quantize_mxfp4_ref, quantize_mxfp4_t)

pytestmark = pytest.mark.gpu


def _rand(shape, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.rand(shape, device=dev, generator=g) * 2 - 1


def _bytes(t):
    assert t.dtype == torch.uint8
    return t.contiguous().cpu()


def _check(c, ref):
    """max |C - ref| <= 2^-7 max |ref|, the figures printed first."""
    c = c.detach().cpu()
    print("err", (c.double() - ref).abs().max().item(), "bound", 2 ** -7 * ref.abs().max().item())
    mx._check(c, ref)


# ---- 1. quantisers ------------------------------------------------------------
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


def _run(x, dual, qtpad=16, qpad=16, spad=3):
    """The C entry point on views of wider poisoned buffers (0x7f in the code
    bytes, 0xff in the scales); returns the logical outputs after checking that
    the padding is unchanged."""
    R, C = x.shape
    dev = x.device
    L = _lib.lib()
    qtb, qt = _poisoned(C, R // 2, qtpad, 0x7f, dev)
    stb, st = _poisoned(C, R // 32, spad, 0xff, dev)
    if dual:
        qb, q = _poisoned(R, C // 2, qpad, 0x7f, dev)
        sb, s = _poisoned(R, C // 32, spad, 0xff, dev)
        rc = L.mxk_quantize_mxfp4_dual(x.data_ptr(), q.data_ptr(), s.data_ptr(), qt.data_ptr(),
                                       st.data_ptr(), R, C, x.stride(0), q.stride(0), s.stride(0),
                                       qt.stride(0), st.stride(0), _lib.stream_ptr(dev))
    else:
        rc = L.mxk_quantize_mxfp4_t(x.data_ptr(), qt.data_ptr(), st.data_ptr(), R, C, x.stride(0),
                                    qt.stride(0), st.stride(0), _lib.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.all(qtb[:, R // 2:] == 0x7f) and torch.all(stb[:, R // 32:] == 0xff)
    if not dual:
        return qt, st
    assert torch.all(qb[:, C // 2:] == 0x7f) and torch.all(sb[:, C // 32:] == 0xff)
    return q, s, qt, st


def _assert_t(x, qt, st):
    qr, sr = quantize_mxfp4_ref(x.cpu().t().contiguous())
    assert torch.equal(_bytes(st), sr)
    assert torch.equal(_bytes(qt), qr)


KINDS = ["uniform", "wide", "zero_blocks", "strided"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [1, 3, 32, 100, 256])
@pytest.mark.parametrize("R", [32, 96, 256, 1152])
def test_quantize_t_bit_equal_to_reference(cuda_device, R, C, kind):
    x = _quant_inputs(R, C, kind, cuda_device)
    _assert_t(x, *_run(x, dual=False))
    qt, st = quantize_mxfp4_t(x)                            # the op: fresh outputs
    assert qt.dtype == torch.uint8 and st.dtype == torch.uint8
    assert qt.shape == (C, R // 2) and st.shape == (C, R // 32)
    _assert_t(x, qt, st)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [32, 256])
@pytest.mark.parametrize("R", [32, 96, 256, 1152])
def test_quantize_dual_bit_equal_to_reference(cuda_device, R, C, kind):
    x = _quant_inputs(R, C, kind, cuda_device)
    q0, s0 = quantize_mxfp4(x)
    qr, sr = quantize_mxfp4_ref(x.cpu())
    for q, s, qt, st in (_run(x, dual=True), quantize_mxfp4_dual(x)):
        assert q.shape == (R, C // 2) and s.shape == (R, C // 32)
        _assert_t(x, qt, st)
        assert torch.equal(_bytes(q), _bytes(q0)) and torch.equal(_bytes(s), _bytes(s0))
        assert torch.equal(_bytes(q), qr) and torch.equal(_bytes(s), sr)


@pytest.mark.parametrize("R,C", [(32, 1), (160, 72), (96, 64)])
def test_quantisers_unaligned_views(cuda_device, R, C):
    """Rows of x that are not 16-byte aligned, and output rows that are not
    4-byte aligned (qt rows with 3 bytes of padding, q rows with 5), take the
    path that goes by element and by byte."""
    buf = torch.zeros((R, C + 3), device=cuda_device, dtype=torch.bfloat16)
    buf[:, 1:C + 1] = _rand((R, C), cuda_device, 43).bfloat16()
    x = buf[:, 1:C + 1]
    _assert_t(x, *_run(x, dual=False))
    _assert_t(x, *_run(x, dual=False, qtpad=3))
    xa = x.contiguous()
    _assert_t(xa, *_run(xa, dual=False, qtpad=3))           # aligned x, unaligned qt rows
    if C % 32 == 0:
        qr, sr = quantize_mxfp4_ref(x.cpu())
        for xx, qtpad, qpad in ((x, 16, 16), (x, 3, 16), (xa, 3, 16), (xa, 16, 5), (xa, 3, 5)):
            q, s, qt, st = _run(xx, dual=True, qtpad=qtpad, qpad=qpad)
            _assert_t(x, qt, st)
            assert torch.equal(_bytes(q), qr) and torch.equal(_bytes(s), sr)


def test_contract_violation_launches_nothing(cuda_device):
    L = _lib.lib()
    x = torch.ones((48, 32), dtype=torch.bfloat16, device=cuda_device)
    out = torch.full((64, 64), 0x7f, dtype=torch.uint8, device=cuda_device)
    sc = torch.full((64, 4), 0xff, dtype=torch.uint8, device=cuda_device)
    sp = _lib.stream_ptr(cuda_device)
    # R % 32
    assert L.mxk_quantize_mxfp4_t(x.data_ptr(), out.data_ptr(), sc.data_ptr(), 48, 32, 32, 64, 4, sp) == 1
    # ldqt < R / 2
    assert L.mxk_quantize_mxfp4_t(x.data_ptr(), out.data_ptr(), sc.data_ptr(), 32, 32, 32, 8, 4, sp) == 1
    # dual: C % 32
    assert L.mxk_quantize_mxfp4_dual(x.data_ptr(), out.data_ptr(), sc.data_ptr(), out.data_ptr(),
                                     sc.data_ptr(), 32, 16, 32, 64, 4, 64, 4, sp) == 1
    torch.cuda.synchronize()
    assert torch.all(out == 0x7f) and torch.all(sc == 0xff)


# ---- 2. the three products -------------------------------------------------------
def _operands(T, i, o, seed, dev):
    """bf16 x, W and a gradient whose 32 x 32 blocks carry exponents 2^-6 .. 2^6,
    so its scales differ along both axes."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand((T, i), generator=g) * 2 - 1).bfloat16()
    w = (torch.randn((o, i), generator=g) * 0.05).bfloat16()
    e = torch.randint(-6, 7, (T // 32, o // 32), generator=g).float()
    dy = (torch.rand((T, o), generator=g) * 2 - 1) * \
        torch.exp2(e).repeat_interleave(32, 0).repeat_interleave(32, 1)
    return x.to(dev), w.to(dev), dy.bfloat16().to(dev)


def _ref_products(x, w, dy):
    """fp64 products of the dequantised reference-quantised operands (CPU)."""
    x, w, dy = x.cpu(), w.cpu(), dy.cpu()
    d = lambda m: dequantize_mxfp4(*quantize_mxfp4_ref(m.contiguous())).double()   # noqa: E731
    return (d(x) @ d(w).t(), d(dy) @ d(w.t()).t(), d(dy.t()) @ d(x.t()).t())


SHAPES = [(256, 256, 256), (512, 256, 768), (256, 1024, 512), (256, 512, 1024)]


@pytest.mark.parametrize("T,i,o", SHAPES)
def test_products_against_dequantised_fp64(cuda_device, T, i, o):
    x, w, dy = _operands(T, i, o, 61, cuda_device)
    xg = x.reshape(2, T // 2, i).clone().requires_grad_()
    wg = w.clone().requires_grad_()
    y = linear_mxfp4(xg, wg)
    y.backward(dy.reshape(2, T // 2, o))
    ry, rdx, rdw = _ref_products(x, w, dy)
    assert y.shape == (2, T // 2, o) and y.dtype == torch.bfloat16
    _check(y.reshape(T, o), ry)
    _check(xg.grad.reshape(T, i), rdx)
    _check(wg.grad, rdw)


def test_main_grad_fresh_then_accumulate(cuda_device):
    T, i, o = 256, 512, 256
    x1, w, dy1 = _operands(T, i, o, 62, cuda_device)
    x2, _, dy2 = _operands(T, i, o, 63, cuda_device)
    wp = w.clone().requires_grad_()
    buf = torch.full((o, i + 8), float("nan"), dtype=torch.bfloat16, device=cuda_device)
    wp.main_grad = buf[:, :i]
    wp._mxk_grad_fresh = True
    ready = []
    wp._mxk_grad_ready = lambda: ready.append(1)
    linear_mxfp4(x1.clone().requires_grad_(), wp).backward(dy1)
    r1 = _ref_products(x1, w, dy1)[2]
    assert wp.grad is None and ready == [1] and wp._mxk_grad_fresh is False
    _check(wp.main_grad, r1)
    assert torch.isnan(buf[:, i:]).all()                    # the padding is untouched
    linear_mxfp4(x2, wp).backward(dy2)
    r2 = _ref_products(x2, w, dy2)[2]
    assert wp.grad is None and ready == [1, 1]
    # two bf16 products and one bf16 sum: three roundings of <= 2^-9 each
    _check(wp.main_grad, r1 + r2)
    assert torch.isnan(buf[:, i:]).all()


def test_run_to_run_identity(cuda_device):
    T, i, o = 512, 256, 768
    x, w, dy = _operands(T, i, o, 64, cuda_device)
    runs = []
    for _ in range(2):
        xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
        y = linear_mxfp4(xg, wg)
        y.backward(dy)
        runs.append([t.contiguous().view(torch.int16).cpu() for t in (y.detach(), xg.grad, wg.grad)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)                            # no atomics: bit-identical


# ---- 3. model ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def fp32_reference():
    torch.manual_seed(0)
    cfg = LlamaConfig.tiny()
    ref = Llama(cfg)                                        # fp32 CPU, bf16-free pure torch
    tok = torch.randint(0, cfg.vocab_size, (2, 129))        # T = 256
    loss = ref.loss(tok)
    loss.backward()
    return ref, tok, loss.item()


def _mx_model_run(ref, tok, dev):
    cfg = LlamaConfig.tiny()
    cfg.linear_dtype = "mxfp4"
    m = Llama(cfg)
    m.load_state_dict(ref.state_dict())
    m = m.to(dev, torch.bfloat16)
    loss = m.loss(tok.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    return m, loss


def test_tiny_llama_mxfp4_against_fp32_cpu(cuda_device, fp32_reference, monkeypatch):
    """Plumbing conditions, not accuracy claims (the CPU file's docstring has the
    figures of the reference emulation alone): |loss - loss_fp32| < 0.1, every
    gradient finite with a cosine >= 0.7 against the fp32 model."""
    ref, tok, ref_loss = fp32_reference
    calls = []
    real = MX.gemm_mxfp4_tn
    monkeypatch.setattr(MX, "gemm_mxfp4_tn", lambda *a, **k: calls.append(1) or real(*a, **k))
    m, loss = _mx_model_run(ref, tok, cuda_device)
    assert len(calls) == 24                                 # 2 layers x 4 linears x 3 products
    print("loss", loss.item(), "fp32", ref_loss)
    assert torch.isfinite(loss).item() and abs(loss.item() - ref_loss) < 0.1
    for (n, pr), (_, pm) in zip(ref.named_parameters(), m.named_parameters()):
        a, b = pr.grad.double().flatten(), pm.grad.double().cpu().flatten()
        assert torch.isfinite(b).all(), n
        cos = (a @ b / (a.norm() * b.norm())).item()
        print(n, round(cos, 5))
        assert cos >= 0.7, (n, cos)
    _, loss2 = _mx_model_run(ref, tok, cuda_device)
    assert torch.equal(loss.cpu(), loss2.cpu())             # bit for bit


def test_three_train_steps_leave_finite_parameters(cuda_device):
    from mxk8s.train.ddp_llama import build, train_step
    cfg = LlamaConfig.tiny()
    cfg.linear_dtype = "mxfp4"
    torch.manual_seed(0)
    model, ddp, opt = build(cfg, cuda_device, bucket_mb=1.0)
    tok = torch.randint(0, cfg.vocab_size, (2, 129), device=cuda_device,
                        generator=torch.Generator(device=cuda_device).manual_seed(1))
    losses = [train_step(model, ddp, opt, tok) for _ in range(3)]
    torch.cuda.synchronize()
    assert all(torch.isfinite(l).item() for l in losses)
    for n, p in model.named_parameters():
        assert torch.isfinite(p).all(), n
