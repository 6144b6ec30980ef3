"""Elementwise fp64 checks of ``native/kernels/optim.hip`` through ``_lib``:
one fused AdamW step (``mxk_adamw_bf16``) and the gradient sum of squares /
clip scale (``mxk_grad_sumsq``, ``mxk_grad_clip_scale``,
``mxk_clip_scale_from_sumsq``), at sizes that take the tail block and a
second trip of the grid-stride loops (the grid cap covers 4096 * 256 * 8 =
8 388 608 elements).

AdamW bounds, elementwise, against ``kernel_refs.adamw_step`` evaluated with
the hyper-parameters rounded to fp32 as the launcher receives them:

    m, v    4 * 2^-24 * sum |terms|               (two / three fp32 roundings)
    master  8 * 2^-24 * (|p decay| + |update|)

The master bound is relative to the update itself only where the update is
well conditioned, so the state is drawn in two interleaved populations:
generic elements have |p| >= 0.5 and v >= 0.05^2 (there the error of the
update, (lr / bc1) / denom * 2 * 2^-24 * (|b1 m| + |(1 - b1) g|) even where
the two terms of m cancel, is below 2^-24 |p|); every 16th element has p = 0
and m, g of one sign (no cancellation: the bound is then 8 roundings of the
update alone, which has at most 7.5: g, m (2), v (3, halved by the square
root), the two divisions, + eps, the product and powf's ulp in bc2), and
every 32nd of those v = 0 with a tiny gradient, where eps decides.
"""
import pytest
import torch

import kernel_refs as R
from mxk8s.ops import _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                   # fp32 unit round-off
CAP = 4096 * 256 * 8             # elements one trip of the grid-stride loops covers
GUARD = 64
INVALID = 1                      # hipErrorInvalidValue
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
P_BF16, P_F32 = 0x7FC1, 0x7FC12345


def _gen(dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return g


def _randn(n, dev, seed):
    return torch.randn(n, device=dev, generator=_gen(dev, seed))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _guarded(t):
    """t followed by GUARD poisoned elements, in one buffer."""
    if t.dtype == torch.bfloat16:
        buf = torch.full((t.numel() + GUARD,), P_BF16, dtype=torch.int16, device=t.device)
    else:
        buf = torch.full((t.numel() + GUARD,), P_F32, dtype=torch.int32, device=t.device)
    buf = buf.view(t.dtype)
    buf[:t.numel()] = t
    return buf


def _guard_intact(buf, n):
    g = _bits(buf[n:])
    return bool((g == (P_BF16 if buf.element_size() == 2 else P_F32)).all())


def _check(what, got, ref, mag, rel, atol=1e-30):
    ratio = R.max_ratio(got, ref, mag, rel, atol)
    print(f"RATIO {what} {ratio:.3g}")
    assert ratio <= 1, f"{what}: largest error / bound = {ratio:.3g}"


# ---- mxk_adamw_bf16 ---------------------------------------------------------
_state_cache = {}


def _adamw_state(n, dev):
    """(master, m, v, grad) of the docstring's two populations; read-only."""
    if n not in _state_cache:
        i = torch.arange(n, device=dev)
        grad = _randn(n, dev, 1) * torch.exp2(((i // 1024) % 7 - 3).float())
        p = _randn(n, dev, 2)
        p = torch.where(p >= 0, 0.5 + p, -0.5 + p)
        m = _randn(n, dev, 3) * 0.1
        v = (0.05 + 0.1 * _randn(n, dev, 4).abs()).pow(2)
        cond = i % 16 == 5                      # well-conditioned update, p = 0
        tiny = i % 32 == 5                      # ... and eps decides
        grad = torch.where(tiny, grad * 2.0 ** -20, grad)
        v = torch.where(tiny, torch.zeros_like(v), v)
        grad = grad.bfloat16()
        p = torch.where(cond, torch.zeros_like(p), p)
        m = torch.where(cond, m.abs() * torch.where(grad.float() < 0, -1.0, 1.0), m)
        m = torch.where(tiny, m * 2.0 ** -20, m)
        _state_cache[n] = (p, m, v, grad)
    return _state_cache[n]


def _adamw_launch(bufs, n, step, wd, scale_t, off=None):
    off = off or {}
    param, master, m, v, grad = bufs
    return _lib.lib().mxk_adamw_bf16(
        param.data_ptr() + off.get("param", 0), master.data_ptr() + off.get("master", 0),
        m.data_ptr() + off.get("m", 0), v.data_ptr() + off.get("v", 0),
        grad.data_ptr() + off.get("grad", 0), n, LR, B1, B2, EPS, wd, step,
        None if scale_t is None else scale_t.data_ptr(), _lib.stream_ptr(param.device))


def _adamw_bufs(n, dev):
    p, m, v, grad = _adamw_state(n, dev)
    param = _guarded(torch.zeros(n, dtype=torch.bfloat16, device=dev))
    _bits(param)[:n] = P_BF16              # the kernel must write every parameter
    return [param, _guarded(p), _guarded(m), _guarded(v), _guarded(grad)]


ADAMW_SIZES = [1, 7, 8, 8 * 256 + 5, CAP + 8 * 300 + 5]


@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("use_scale", [False, True], ids=["noscale", "scale0.25"])
@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("n", ADAMW_SIZES)
def test_adamw_step_elementwise(cuda_device, n, step, use_scale, wd):
    dev = cuda_device
    tag = f"adamw[n={n},step={step},{'scale' if use_scale else 'noscale'},wd={wd}]"
    p0, m0, v0, grad = _adamw_state(n, dev)
    scale_t = torch.tensor([0.25], dtype=torch.float32, device=dev) if use_scale else None
    bufs = _adamw_bufs(n, dev)
    assert _adamw_launch(bufs, n, step, wd, scale_t) == 0
    param, master, m, v, g_after = bufs
    p1, m1, v1, mag_p, mag_m, mag_v = R.adamw_step(
        p0, m0, v0, grad, R.f32(LR), R.f32(B1), R.f32(B2), R.f32(EPS), R.f32(wd), step,
        0.25 if use_scale else 1.0)
    _check(f"{tag} exp_avg", m[:n], m1, mag_m, 4 * U)
    _check(f"{tag} exp_avg_sq", v[:n], v1, mag_v, 4 * U)
    _check(f"{tag} master", master[:n], p1, mag_p, 8 * U)
    # the bf16 parameter copy is the round-to-nearest of the master written
    assert torch.equal(_bits(param[:n]), _bits(master[:n].bfloat16())), f"{tag}: param copy"
    assert torch.equal(_bits(g_after[:n]), _bits(grad)), f"{tag}: gradient modified"
    for b, name in zip(bufs, ("param", "master", "m", "v", "grad")):
        assert _guard_intact(b, n), f"{tag}: guard after {name} written"
    # a second run from the same state: the same bits
    again = _adamw_bufs(n, dev)
    assert _adamw_launch(again, n, step, wd, scale_t) == 0
    for a, b, name in zip(bufs, again, ("param", "master", "m", "v", "grad")):
        assert torch.equal(_bits(a), _bits(b)), f"{tag}: {name} differs run to run"


def test_adamw_rejections_write_nothing(cuda_device):
    dev = cuda_device
    n = 8 * 256 + 5
    bufs = _adamw_bufs(n, dev)
    before = [b.clone() for b in bufs]
    assert _adamw_launch(bufs, n, 0, 0.1, None) == INVALID           # step < 1
    for name, off in (("param", 2), ("grad", 2), ("master", 4), ("m", 4), ("v", 4)):
        assert _adamw_launch(bufs, n - 8, 1, 0.1, None, off={name: off}) == INVALID, name
    assert _adamw_launch(bufs, 0, 1, 0.1, None) == 0                  # nothing to do
    for a, b in zip(bufs, before):
        assert torch.equal(_bits(a), _bits(b))


# ---- sum of squares and clip scale ------------------------------------------
def _expected_partials(n):
    return min(4096, max(1, (n // 8 + 255) // 256))


def _sumsq(grad, n):
    L = _lib.lib()
    dev = grad.device
    nparts = L.mxk_sumsq_partials(n)
    assert nparts == _expected_partials(n)
    parts = torch.full((nparts + 1,), P_F32, dtype=torch.int32, device=dev).view(torch.float32)
    out = torch.full((1,), P_F32, dtype=torch.int32, device=dev).view(torch.float32)
    assert L.mxk_grad_sumsq(grad.data_ptr(), n, parts.data_ptr(), out.data_ptr(),
                            _lib.stream_ptr(dev)) == 0
    return parts, out, nparts


def _clip_ref(sumsq64, inv_world, max_norm):
    norm = sumsq64 ** 0.5 * R.f32(inv_world)
    mx = R.f32(max_norm)
    clip = mx / (norm + R.f32(1e-6)) if mx > 0 and norm > mx else 1.0
    return R.f32(inv_world) * clip, norm


@pytest.mark.parametrize("n", [1, 7, 8, 1000, CAP + 8 * 300 + 3])
def test_grad_sumsq_and_clip_scale(cuda_device, n):
    """Gradient magnitudes vary along the buffer (an error in which elements
    a thread or block visits changes the sum).  Sum of squares within 1e-5 of
    fp64 (a thread adds at most 17 squares in sequence here, then a six-level
    wave tree and four waves; the partials fold in double); norm and scale
    within 1e-5: half the sum's bound through the square root plus three fp32
    roundings."""
    dev = cuda_device
    L = _lib.lib()
    tag = f"sumsq[n={n}]"
    i = torch.arange(n, device=dev)
    grad = _guarded((_randn(n, dev, 7) * torch.exp2(((i // 777) % 9 - 4).float()) *
                     (1 + (i % 5).float())).bfloat16())
    ref = grad[:n].double().pow(2).sum().item()
    parts, out, nparts = _sumsq(grad, n)
    _check(f"{tag} sumsq", out, torch.tensor([ref], device=dev, dtype=torch.float64),
           torch.tensor([ref], device=dev, dtype=torch.float64), 1e-5, atol=0.0)
    # exactly nparts partials were written, they add up, the next element is untouched
    assert torch.isfinite(parts[:nparts]).all(), f"{tag}: a partial was not written"
    assert _bits(parts[nparts:]).item() == P_F32, f"{tag}: wrote past the partials"
    assert abs(parts[:nparts].double().sum().item() - ref) <= 1e-5 * ref
    assert _guard_intact(grad, n)

    norm_ref = ref ** 0.5 / 4
    for max_norm in (0.0, 0.5 * norm_ref, 2.0 * norm_ref):
        scale_ref, nref = _clip_ref(ref, 0.25, max_norm)
        if max_norm == 0.0 or max_norm > norm_ref:
            assert scale_ref == 0.25                 # clipping off / not needed
        else:
            assert scale_ref < 0.25
        for fused in (False, True):
            out2 = torch.full((2,), P_F32, dtype=torch.int32, device=dev).view(torch.float32)
            if fused:
                ws = torch.full((nparts + 1,), P_F32, dtype=torch.int32,
                                device=dev).view(torch.float32)
                st = L.mxk_grad_clip_scale(grad.data_ptr(), n, ws.data_ptr(), 0.25, max_norm,
                                           out2.data_ptr(), _lib.stream_ptr(dev))
                assert _bits(ws[nparts:]).item() == P_F32
            else:
                st = L.mxk_clip_scale_from_sumsq(out.data_ptr(), 0.25, max_norm, out2.data_ptr(),
                                                 _lib.stream_ptr(dev))
            assert st == 0
            want = torch.tensor([scale_ref, nref], device=dev, dtype=torch.float64)
            _check(f"{tag} clip[max_norm={max_norm:.3g},{'fused' if fused else 'from_sumsq'}]",
                   out2, want, want, 1e-5, atol=0.0)


def test_grad_sumsq_of_zeros(cuda_device):
    dev = cuda_device
    L = _lib.lib()
    n = 1000
    grad = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    parts, out, nparts = _sumsq(grad, n)
    assert _bits(out).item() == 0 and not _bits(parts[:nparts]).any()
    out2 = torch.full((2,), P_F32, dtype=torch.int32, device=dev).view(torch.float32)
    assert L.mxk_grad_clip_scale(grad.data_ptr(), n, parts.data_ptr(), 0.25, 1.0, out2.data_ptr(),
                                 _lib.stream_ptr(dev)) == 0
    assert out2.tolist() == [0.25, 0.0]


def test_grad_sumsq_rejections_write_nothing(cuda_device):
    dev = cuda_device
    L = _lib.lib()
    grad = torch.ones(64, dtype=torch.bfloat16, device=dev)
    parts = torch.full((2,), P_F32, dtype=torch.int32, device=dev).view(torch.float32)
    out = torch.full((2,), P_F32, dtype=torch.int32, device=dev).view(torch.float32)
    s = _lib.stream_ptr(dev)
    assert L.mxk_grad_sumsq(grad.data_ptr() + 2, 32, parts.data_ptr(), out.data_ptr(), s) == INVALID
    assert L.mxk_grad_sumsq(grad.data_ptr(), 0, parts.data_ptr(), out.data_ptr(), s) == INVALID
    assert L.mxk_grad_clip_scale(grad.data_ptr() + 2, 32, parts.data_ptr(), 0.25, 1.0,
                                 out.data_ptr(), s) == INVALID
    assert L.mxk_grad_clip_scale(grad.data_ptr(), 0, parts.data_ptr(), 0.25, 1.0, out.data_ptr(),
                                 s) == INVALID
    assert (_bits(parts) == P_F32).all() and (_bits(out) == P_F32).all()
