"""Stochastic-rounding MXFP4 quantisers and ``linear_mxfp4(.., "stochastic")`` on
the GPU (``native/kernels/quantize_mxfp4_sr.hip``: the templates of
``mx_quantize.h`` on the stochastic format; ``mxk8s/ops/linear.py``).

The generator is counter-based, so the kernels are bit-equal to the reference
quantiser for every seed, and the products are compared with the fp64 product
of the dequantised *reference* images of the same seeds under the project's
bf16-output criterion (``mx_gemm_checks._check``).
"""
import pytest
import torch

import mx_gemm_checks as mx
import mx_linear_checks as lc
import mx_sr_checks as sr
from mxk8s.ops import _lib
from mxk8s.ops.linear import linear_mxfp4
from mxk8s.ops.mxfp4 import quantize_mxfp4, quantize_mxfp4_dual, quantize_mxfp4_t

pytestmark = pytest.mark.gpu

F = lc.MXFP4
M64 = sr.M64
KINDS = ["uniform", "wide", "zero_blocks", "strided"]
TR_SEEDS = [M64 - 1, 0x9E3779B97F4A7C15]       # the first makes the dual's seed + 1 wrap to 0


def _entry(suffix):
    return getattr(_lib.lib(), "mxk_quantize_mxfp4_sr" + suffix)


def _assert_image(x, seed, q, s):
    qr, s_r = sr.ref(x, seed)
    assert torch.equal(lc._bytes(s), s_r)
    assert torch.equal(lc._bytes(q), qr)


# ---- 1. rows kernel ----------------------------------------------------------------
@pytest.mark.parametrize("seed", sr.SEEDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", [32, 96, 256])
@pytest.mark.parametrize("R", [1, 3, 33])
def test_quantize_rows_bit_equal_to_reference(cuda_device, R, K, kind, seed):
    x = mx._quant_inputs(R, K, kind, cuda_device)
    q, s = quantize_mxfp4(x, "stochastic", seed)
    assert q.dtype == s.dtype == torch.uint8 and q.shape == (R, K // 2) and s.shape == (R, K // 32)
    _assert_image(x, seed, q, s)
    # the entry point on poisoned buffers wider and longer than the result
    qbuf = torch.full((R + 1, K // 2 + 24), 0xA5, dtype=torch.uint8, device=cuda_device)
    sbuf = torch.full((R + 1, K // 32 + 5), 0xA5, dtype=torch.uint8, device=cuda_device)
    rc = _entry("")(x.data_ptr(), qbuf.data_ptr(), sbuf.data_ptr(), R, K, x.stride(0), qbuf.stride(0),
                    sbuf.stride(0), seed, _lib.stream_ptr(cuda_device))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.all(qbuf[:, K // 2:] == 0xA5) and torch.all(qbuf[R:] == 0xA5)
    assert torch.all(sbuf[:, K // 32:] == 0xA5) and torch.all(sbuf[R:] == 0xA5)
    _assert_image(x, seed, qbuf[:R, :K // 2], sbuf[:R, :K // 32])


def test_quantize_rows_unaligned_view(cuda_device):
    x = mx.unaligned_rows(cuda_device)                       # the by-element kernel
    for seed in sr.SEEDS:
        _assert_image(x, seed, *quantize_mxfp4(x, "stochastic", seed))


# ---- 2. transposing and dual kernels ---------------------------------------------------
def _run(x, dual, seed, qtpad=16, qpad=16, spad=3):
    """lc._run for the stochastic entry points: views of wider poisoned buffers,
    the padding checked unchanged."""
    R, C = x.shape
    dev = x.device
    qtb, qt = lc._poisoned(C, R // 2, qtpad, 0x7f, dev)
    stb, st = lc._poisoned(C, R // 32, spad, 0xff, dev)
    if dual:
        qb, q = lc._poisoned(R, C // 2, qpad, 0x7f, dev)
        sb, s = lc._poisoned(R, C // 32, spad, 0xff, dev)
        rc = _entry("_dual")(x.data_ptr(), q.data_ptr(), s.data_ptr(), qt.data_ptr(), st.data_ptr(),
                             R, C, x.stride(0), q.stride(0), s.stride(0), qt.stride(0), st.stride(0),
                             seed, _lib.stream_ptr(dev))
    else:
        rc = _entry("_t")(x.data_ptr(), qt.data_ptr(), st.data_ptr(), R, C, x.stride(0), qt.stride(0),
                          st.stride(0), seed, _lib.stream_ptr(dev))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.all(qtb[:, R // 2:] == 0x7f) and torch.all(stb[:, R // 32:] == 0xff)
    if not dual:
        return qt, st
    assert torch.all(qb[:, C // 2:] == 0x7f) and torch.all(sb[:, C // 32:] == 0xff)
    return q, s, qt, st


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [1, 3, 32, 100, 256])
@pytest.mark.parametrize("R", [32, 96, 256, 1152])
def test_quantize_t_bit_equal_to_reference(cuda_device, R, C, kind):
    """R = 1152 is 9 row tiles: the group index of the counter includes the tile origin."""
    x = lc._quant_inputs(R, C, kind, cuda_device)
    for seed in TR_SEEDS:
        _assert_image(x.t(), seed, *_run(x, False, seed))
        qt, st = quantize_mxfp4_t(x, "stochastic", seed)
        assert qt.shape == (C, R // 2) and st.shape == (C, R // 32)
        _assert_image(x.t(), seed, qt, st)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [32, 256])
@pytest.mark.parametrize("R", [32, 96, 256, 1152])
def test_quantize_dual_bit_equal_to_reference(cuda_device, R, C, kind):
    x = lc._quant_inputs(R, C, kind, cuda_device)
    for seed in TR_SEEDS:
        for q, s, qt, st in (_run(x, True, seed), quantize_mxfp4_dual(x, "stochastic", seed)):
            assert q.shape == (R, C // 2) and s.shape == (R, C // 32)
            _assert_image(x, seed, q, s)
            _assert_image(x.t(), (seed + 1) % M64, qt, st)    # its own noise


@pytest.mark.parametrize("R,C", [(32, 1), (160, 72), (96, 64)])
def test_quantisers_unaligned_views(cuda_device, R, C):
    """lc.quantisers_unaligned_views for the stochastic entry points: unaligned
    rows of x, qt rows with 3 bytes of padding, q rows with 5."""
    seed = 0x9E3779B97F4A7C15
    buf = torch.zeros((R, C + 3), device=cuda_device, dtype=torch.bfloat16)
    buf[:, 1:C + 1] = lc._rand((R, C), cuda_device, 43).bfloat16()
    x = buf[:, 1:C + 1]
    xa = x.contiguous()
    qtpad = lc._unaligned(F, R, F.unaligned_qtpad)
    for src, pad in ((x, 16), (x, qtpad), (xa, qtpad)):
        _assert_image(x.t(), seed, *_run(src, False, seed, qtpad=pad))
    if C % 32 == 0:
        for which, qtp, qp in F.unaligned_dual:
            q, s, qt, st = _run({"x": x, "xa": xa}[which], True, seed, qtpad=lc._unaligned(F, R, qtp),
                                qpad=lc._unaligned(F, C, qp))
            _assert_image(x, seed, q, s)
            _assert_image(x.t(), seed + 1, qt, st)


def test_contract_violation_launches_nothing(cuda_device):
    """R % 32, ldqt < R / 2, C % 32 for the dual entry, and an index the
    counter cannot hold (2^32 rows): hipErrorInvalidValue, nothing written."""
    dev = cuda_device
    x = torch.ones((48, 32), dtype=torch.bfloat16, device=dev)
    out = torch.full((64, 64), 0x7f, dtype=torch.uint8, device=dev)
    sc = torch.full((64, 4), 0xff, dtype=torch.uint8, device=dev)
    sp = _lib.stream_ptr(dev)
    xp, op, scp = x.data_ptr(), out.data_ptr(), sc.data_ptr()
    assert _entry("_t")(xp, op, scp, 48, 32, 32, 64, 4, 1, sp) == 1            # R % 32
    assert _entry("_t")(xp, op, scp, 32, 32, 32, F.short_ldqt, 4, 1, sp) == 1
    assert _entry("_dual")(xp, op, scp, op, scp, 32, 16, 32, 64, 4, 64, 4, 1, sp) == 1   # C % 32
    assert _entry("")(xp, op, scp, 32, 48, 48, 64, 4, 1, sp) == 1              # K % 32
    assert _entry("")(xp, op, scp, 2 ** 32, 32, 32, 64, 4, 1, sp) == 1
    assert _entry("_t")(xp, op, scp, 2 ** 32, 32, 32, 2 ** 31, 2 ** 27, 1, sp) == 1
    torch.cuda.synchronize()
    assert torch.all(out == 0x7f) and torch.all(sc == 0xff)


def test_grid_input_is_fixed(cuda_device):
    x = sr.grid_tensor(96, 96, 5)
    want = sr.ref(x)                                         # exact under either rounding
    xd = x.to(cuda_device)
    for seed in (0, 1, M64 - 1):
        q, s, qt, st = quantize_mxfp4_dual(xd, "stochastic", seed)
        assert torch.equal(q.cpu(), want[0]) and torch.equal(s.cpu(), want[1])
        assert torch.equal(sr.deq((qt.cpu(), st.cpu())), x.t().double())


# ---- 3. linear_mxfp4, stochastic ---------------------------------------------------------
def _ref_grads(x, w, dy, seed):
    """fp64 dx, dW from the dequantised reference images: dy's rows with seed,
    its columns with seed + 1, W^T and x^T round-to-nearest."""
    x, w, dy = x.cpu(), w.cpu(), dy.cpu()
    return (sr.deq(sr.ref(dy, seed)) @ sr.deq(sr.ref(w.t())).t(),
            sr.deq(sr.ref(dy.t(), (seed + 1) % M64)) @ sr.deq(sr.ref(x.t())).t())


def _fwd_bwd(x, w, dy, *rounding, **kw):
    xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = linear_mxfp4(xg, wg, *rounding, **kw)
    y.backward(dy)
    return y.detach(), xg.grad, wg.grad


@pytest.mark.parametrize("T,i,o", [(256, 256, 256), (512, 256, 768)])
def test_products_against_dequantised_fp64(cuda_device, T, i, o):
    x, w, dy = lc.operands(T, i, o, 61, cuda_device)
    seed = 0x9E3779B97F4A7C15
    y, dx, dw = _fwd_bwd(x, w, dy, "stochastic", seed=seed)
    y0, dx0, _ = _fwd_bwd(x, w, dy)
    assert torch.equal(lc._bytes(y), lc._bytes(y0))          # the forward is untouched
    rdx, rdw = _ref_grads(x, w, dy, seed)
    lc.check(dx, rdx)
    lc.check(dw, rdw)
    # the same seed twice is bit-identical, another seed is another gradient
    _, dx1, dw1 = _fwd_bwd(x, w, dy, "stochastic", seed=seed)
    assert torch.equal(lc._bytes(dx), lc._bytes(dx1)) and torch.equal(lc._bytes(dw), lc._bytes(dw1))
    _, dx2, _ = _fwd_bwd(x, w, dy, "stochastic", seed=seed + 2)
    assert not torch.equal(dx, dx2) and not torch.equal(dx, dx0)
    # one gradient alone equals the dual's
    xg = x.clone().requires_grad_()
    linear_mxfp4(xg, w, "stochastic", seed=seed).backward(dy)
    wg = w.clone().requires_grad_()
    linear_mxfp4(x, wg, "stochastic", seed=seed).backward(dy)
    assert torch.equal(lc._bytes(xg.grad), lc._bytes(dx)) and torch.equal(lc._bytes(wg.grad), lc._bytes(dw))


def test_main_grad_fresh_then_accumulate(cuda_device):
    T, i, o = 256, 512, 256
    x1, w, dy1 = lc.operands(T, i, o, 62, cuda_device)
    x2, _, dy2 = lc.operands(T, i, o, 63, cuda_device)
    wp, buf, ready = lc.main_grad_weight(w, i, o)
    linear_mxfp4(x1.clone().requires_grad_(), wp, "stochastic", seed=10).backward(dy1)
    r1 = _ref_grads(x1, w, dy1, 10)[1]
    assert wp.grad is None and ready == [1] and wp._mxk_grad_fresh is False
    lc.check(wp.main_grad, r1)
    assert torch.isnan(buf[:, i:]).all()                     # the padding is untouched
    linear_mxfp4(x2, wp, "stochastic", seed=12).backward(dy2)
    r2 = _ref_grads(x2, w, dy2, 12)[1]
    assert wp.grad is None and ready == [1, 1]
    lc.check(wp.main_grad, r1 + r2)
    assert torch.isnan(buf[:, i:]).all()


# ---- 4. model ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fp32_reference():
    return lc.fp32_reference()


def test_tiny_llama_stochastic_against_fp32_cpu(cuda_device, fp32_reference):
    """The loss is the round-to-nearest run's bit for bit (the forward is
    untouched); every gradient is finite with a cosine >= 0.695 against the fp32
    model: the reference emulation's lowest figure, 0.839
    (``test_mxfp4_sr_cpu.py``), less the 0.144 that ``test_gpu_mxfp4_linear.py``
    leaves under its own emulation figure.  A plumbing condition, not an
    accuracy claim."""
    ref_model, tok, ref_loss = fp32_reference
    m, loss = sr.sr_model_run(ref_model, tok, cuda_device, "stochastic")
    _, loss_rne = sr.sr_model_run(ref_model, tok, cuda_device, "nearest")
    torch.cuda.synchronize()
    print("loss", loss.item(), "nearest", loss_rne.item(), "fp32", ref_loss)
    assert torch.isfinite(loss).item() and torch.equal(loss.cpu(), loss_rne.cpu())
    worst = sr.min_cosine(ref_model, m)
    print("worst cosine", worst)
    assert worst >= 0.695
    m2, _ = sr.sr_model_run(ref_model, tok, cuda_device, "stochastic")   # reseeded: the same draws
    for (n, a), (_, b) in zip(m.named_parameters(), m2.named_parameters()):
        assert torch.equal(lc._bytes(a.grad), lc._bytes(b.grad)), n


def test_three_train_steps_leave_finite_parameters(cuda_device):
    from mxk8s.models.llama import LlamaConfig
    from mxk8s.ops.mxfp4 import sr_reseed
    from mxk8s.train.ddp_llama import build, train_step
    cfg = LlamaConfig.tiny()
    cfg.linear_dtype, cfg.grad_rounding = "mxfp4", "stochastic"
    torch.manual_seed(0)
    model, ddp, opt = build(cfg, cuda_device, bucket_mb=1.0)
    tok = torch.randint(0, cfg.vocab_size, (2, 129), device=cuda_device,
                        generator=torch.Generator(device=cuda_device).manual_seed(1))
    losses = []
    for step in range(3):
        sr_reseed(0, 0, step)
        losses.append(train_step(model, ddp, opt, tok))
    torch.cuda.synchronize()
    assert all(torch.isfinite(l).item() for l in losses)
    for n, p in model.named_parameters():
        assert torch.isfinite(p).all(), n
