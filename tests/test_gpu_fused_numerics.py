"""Elementwise fp64 checks of the memory-bound kernels in
``native/kernels/fused_ops.hip`` and ``xent.hip``: RMSNorm / add-RMSNorm,
SwiGLU, RoPE and the fused cross-entropy, called through ``_lib`` so that the
saved statistics (rstd, lse, row loss) are visible.

Bound, per element, for every bf16 output:

    |got - ref64| <= 2^-8 mag + atol

``mag`` is the sum of the absolute values of the terms the closed form adds
(``tests/kernel_refs.py``).  Round-to-nearest bf16 (8 significant bits) is
half an ulp, 2^-9 of the result at the top of a binade and 2^-8 of it just
above a power of two.  So rounding alone reaches 1 / (1 + 2^-8) = 0.996 of
the bound at a result of 2^e (1 + 2^-8), and that is the largest ratio
measured on every large tensor here.  What is left for the fp32 evaluation
and ``__expf`` at that worst point is 2^-16 of the result, against an error
of a few 2^-24; everywhere else in the binade, and wherever terms cancel
(``mag`` then exceeds the result), the room is larger.  ``atol``
only matters next to zero: 1e-30 (fp32 / bf16 underflow is below 1.2e-38 times
factors of at most 2^20 here), and 2e-5 g at the cross-entropy label entry,
where p - 1 cancels for p ~ 1 and carries the error of lse.  fp32 statistics:
rstd within 1e-5 relative, lse and row loss within 1e-5 max(1, |ref|), at
least four times the fp32 bound of a sum of positive terms 40 adds deep
(40 * 2^-24 = 2.4e-6).  dw in fp32: 2^-20 sum_r |dy x rstd| per column.

The inputs tell rows and columns apart: row r is scaled by 2^((r mod 17) - 8)
(rstd spans 2^16), one row is all zero (rstd = eps^-1/2), one has magnitude
2^-10 (mean square below eps: eps decides), w has mixed signs and a
per-column pattern.  Every assertion message (and one RATIO line per check on
stdout) gives the largest error / bound ratio.
"""
import pytest
import torch

import kernel_refs as R
from mxk8s.ops import _lib

pytestmark = pytest.mark.gpu

REL = 2.0 ** -8
ATOL = 1e-30
EPS = 1e-5
INVALID = 1          # hipErrorInvalidValue


# ---- helpers ----------------------------------------------------------------
def _gen(dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return g


def _randn(shape, dev, seed):
    return torch.randn(shape, device=dev, generator=_gen(dev, seed))


def _poison(shape, dtype, dev):
    """A NaN bit pattern no kernel produces: unwritten outputs fail every
    bound, and written padding changes bits."""
    if dtype == torch.bfloat16:
        return torch.full(shape, 0x7FC1, dtype=torch.int16, device=dev).view(torch.bfloat16)
    assert dtype == torch.float32
    return torch.full(shape, 0x7FC12345, dtype=torch.int32, device=dev).view(torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def _stream(dev):
    return _lib.stream_ptr(dev)


def _check(what, got, ref, mag, rel=REL, atol=ATOL):
    ratio = R.max_ratio(got, ref, mag, rel, atol)
    print(f"RATIO {what} {ratio:.3g}")
    assert ratio <= 1, f"{what}: largest error / bound = {ratio:.3g}"
    return ratio


def _check_stat(what, got, ref, rel_to):
    """fp32 statistic: |got - ref| <= 1e-5 rel_to."""
    return _check(what, got, ref, rel_to, rel=1e-5, atol=0.0)


# ---- RMSNorm / add-RMSNorm --------------------------------------------------
def _rms_inputs(rows, H, dev):
    r = torch.arange(rows, device=dev)
    scale = torch.exp2(((r % 17) - 8).float())[:, None]
    x = _randn((rows, H), dev, 11) * scale
    delta = _randn((rows, H), dev, 12) * scale
    zero_row, tiny_row = (1, 2) if rows >= 3 else (1, 0)
    sgn = torch.where(_randn((H,), dev, 13) > 0, 1.0, -1.0)
    x[tiny_row] = sgn * 2.0 ** -10
    delta[tiny_row] = 0
    x[zero_row] = 0
    delta[zero_row] = 0
    c = torch.arange(H, device=dev)
    w = ((c % 2) * 2 - 1).float() * (0.5 + (c % 13).float() / 8)
    dy = _randn((rows, H), dev, 14) * torch.exp2(((r % 5) - 2).float())[:, None]
    dres = _randn((rows, H), dev, 15)
    return tuple(t.bfloat16() for t in (x, delta, w, dy, dres)) + (zero_row, tiny_row)


def _rms_fwd(x, w, delta=None):
    L = _lib.lib()
    rows, H = x.shape
    dev = x.device
    y = _poison((rows, H), torch.bfloat16, dev)
    rstd = _poison((rows,), torch.float32, dev)
    if delta is None:
        st = L.mxk_rmsnorm_fwd(x.data_ptr(), w.data_ptr(), y.data_ptr(), rstd.data_ptr(), rows, H,
                               EPS, _stream(dev))
        h = None
    else:
        h = _poison((rows, H), torch.bfloat16, dev)
        st = L.mxk_add_rmsnorm_fwd(x.data_ptr(), delta.data_ptr(), w.data_ptr(), h.data_ptr(),
                                   y.data_ptr(), rstd.data_ptr(), rows, H, EPS, _stream(dev))
    assert st == 0
    return y, rstd, h


def _rms_bwd(dy, x, w, rstd, dres):
    L = _lib.lib()
    rows, H = x.shape
    dev = x.device
    dx = _poison((rows, H), torch.bfloat16, dev)
    dw_bf16 = _poison((H,), torch.bfloat16, dev)
    dw_f32 = _poison((H,), torch.float32, dev)
    ws = _poison((L.mxk_rmsnorm_bwd_workspace(rows, H) // 4,), torch.float32, dev)
    st = L.mxk_rmsnorm_bwd(dy.data_ptr(), x.data_ptr(), w.data_ptr(), rstd.data_ptr(),
                           None if dres is None else dres.data_ptr(), dx.data_ptr(),
                           dw_bf16.data_ptr(), dw_f32.data_ptr(), ws.data_ptr(), rows, H,
                           _stream(dev))
    assert st == 0
    return dx, dw_bf16, dw_f32


RMS_SHAPES = [
    (3, 8), (5, 2056),                              # general kernel, one row per block
    (257, 128), (300, 4096), (1023, 4096),          # general, rows_per_block > 1, ragged last block
    (2, 16384),                                     # largest H the backward accepts
    (1024, 2048), (1025, 4096), (1024, 8192),       # wave kernel: boundary, uneven rows per wave
]


@pytest.mark.parametrize("fused_add", [False, True], ids=["plain", "add"])
@pytest.mark.parametrize("rows,H", RMS_SHAPES)
def test_rmsnorm_fwd_bwd_elementwise(cuda_device, rows, H, fused_add):
    """Forward (y, rstd, and h of the fused add), backward dx with / without
    the residual gradient, dw through dw_f32 and through the bf16 output, and
    both backward paths bitwise run to run."""
    tag = f"rms[{rows}x{H},{'add' if fused_add else 'plain'}]"
    x, delta, w, dy, dres, zero_row, _ = _rms_inputs(rows, H, cuda_device)
    eps = R.f32(EPS)
    if fused_add:
        y, rstd, h = _rms_fwd(x, w, delta)
        h_ref = (x.double() + delta.double()).bfloat16()
        assert torch.equal(_bits(h), _bits(h_ref)), f"{tag}: h is not bf16(x + delta)"
        # y is computed from the rounded h: the plain kernel fed h agrees bit for bit
        y2, rstd2, _ = _rms_fwd(h, w)
        assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(rstd), _bits(rstd2)), \
            f"{tag}: y / rstd not those of the bf16-rounded h"
        xin = h
    else:
        y, rstd, _ = _rms_fwd(x, w)
        xin = x
    y_ref, rs_ref, y_mag = R.rmsnorm_fwd(xin, w, eps)
    _check(f"{tag} y", y, y_ref, y_mag)
    _check_stat(f"{tag} rstd", rstd, rs_ref, rs_ref)
    assert rs_ref[zero_row].item() == pytest.approx(eps ** -0.5, rel=1e-12)
    assert not y[zero_row].any()

    res = dres if fused_add else None
    dx, dw_bf16, dw_f32 = _rms_bwd(dy, xin, w, rstd, res)
    dx_ref, dx_mag, dw_ref, dw_mag = R.rmsnorm_bwd(dy, xin, w, eps, res)
    _check(f"{tag} dx", dx, dx_ref, dx_mag)
    _check(f"{tag} dw_f32", dw_f32, dw_ref, dw_mag, rel=2.0 ** -20)
    _check(f"{tag} dw_bf16", dw_bf16, dw_ref, dw_mag)
    again = _rms_bwd(dy, xin, w, rstd, res)
    for a, b, name in zip((dx, dw_bf16, dw_f32), again, ("dx", "dw_bf16", "dw_f32")):
        assert torch.equal(_bits(a), _bits(b)), f"{tag}: {name} differs run to run"


# ---- SwiGLU -----------------------------------------------------------------
_G_SPECIAL = [0.0, -0.0, 2.0 ** -20, -2.0 ** -20, -1.278, 20.0, -20.0, 88.0, -88.0, 200.0, -200.0]


@pytest.mark.parametrize("rows,F", [(1, 8), (3, 1000), (130, 8200)])
def test_swiglu_elementwise(cuda_device, rows, F):
    """g covers +-0, +-2^-20, -1.278 (dg's bracket changes sign), +-20, +-88
    and +-200 against u and dh of mixed magnitudes: finite inputs give finite
    results within the bound."""
    dev = cuda_device
    L = _lib.lib()
    tag = f"swiglu[{rows}x{F}]"
    n = rows * F
    i = torch.arange(n, device=dev)
    g = _randn((n,), dev, 21) * 3
    special = torch.tensor(_G_SPECIAL, device=dev)
    # every third element cycles through the special values (for F = 8 only
    # a few fit, the larger shapes see all of them against many u / dh)
    g[::3] = special[(i[::3] // 3) % len(_G_SPECIAL)]
    u = _randn((n,), dev, 22) * torch.exp2(((i % 9) - 4).float())
    dh = _randn((n,), dev, 23) * torch.exp2(((i // 9 % 9) - 4).float())
    gu = torch.cat([g.view(rows, F), u.view(rows, F)], dim=1).bfloat16().contiguous()
    dh = dh.view(rows, F).bfloat16().contiguous()
    gb, ub = gu[:, :F], gu[:, F:]
    assert torch.isfinite(gu.float()).all()

    h = _poison((rows, F), torch.bfloat16, dev)
    assert L.mxk_swiglu_fwd(gu.data_ptr(), h.data_ptr(), rows, F, _stream(dev)) == 0
    h_ref, h_mag = R.swiglu_fwd(gb, ub)
    _check(f"{tag} h", h, h_ref, h_mag)

    dgu = _poison((rows, 2 * F), torch.bfloat16, dev)
    assert L.mxk_swiglu_bwd(gu.data_ptr(), dh.data_ptr(), dgu.data_ptr(), rows, F,
                            _stream(dev)) == 0
    dg_ref, dg_mag, du_ref, du_mag = R.swiglu_bwd(gb, ub, dh)
    _check(f"{tag} dg", dgu[:, :F], dg_ref, dg_mag)
    _check(f"{tag} du", dgu[:, F:], du_ref, du_mag)


# ---- RoPE -------------------------------------------------------------------
def _rope_call(x_buf, y_buf, cos, sin, tokens, heads, D, S, sign, x_tok, y_tok):
    return _lib.lib().mxk_rope_strided(x_buf.data_ptr(), y_buf.data_ptr(), cos.data_ptr(),
                                       sin.data_ptr(), tokens, heads, D, S, float(sign), x_tok,
                                       y_tok, _stream(x_buf.device))


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("B,S,heads,D", [(1, 1, 1, 16), (2, 5, 3, 64), (3, 17, 2, 128)])
def test_rope_strided_elementwise(cuda_device, B, S, heads, D, sign):
    """Token strides larger than heads * D and different for x and y, poisoned
    gaps in y, every table row distinct (token t of batch b uses row t mod S),
    and the in-place call bit-equal to the out-of-place one."""
    dev = cuda_device
    tag = f"rope[{B},{S},{heads},{D},{sign:+.0f}]"
    tokens, hd = B * S, heads * D
    x_tok, y_tok = hd + 8, hd + 24
    ang = torch.rand((S, D // 2), device=dev, generator=_gen(dev, 31)) * 6.283
    cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    assert S == 1 or len({tuple(r.tolist()) for r in cos.cpu()}) == S
    x = (_randn((tokens, heads, D), dev, 32) *
         torch.exp2((torch.arange(tokens, device=dev) % 7 - 3).float())[:, None, None]).bfloat16()
    x_buf = _poison((tokens, x_tok), torch.bfloat16, dev)
    x_buf[:, :hd] = x.view(tokens, hd)
    y_buf = _poison((tokens, y_tok), torch.bfloat16, dev)
    assert _rope_call(x_buf, y_buf, cos, sin, tokens, heads, D, S, sign, x_tok, y_tok) == 0
    y_ref, mag = R.rope(x, cos, sin, sign, S)
    _check(f"{tag} y", y_buf[:, :hd].reshape(tokens, heads, D), y_ref, mag)
    gap = _bits(y_buf[:, hd:])
    assert torch.equal(gap, torch.full_like(gap, 0x7FC1)), f"{tag}: gap of y written"
    assert torch.equal(_bits(x_buf[:, :hd]), _bits(x.view(tokens, hd))), f"{tag}: x modified"
    # in place (y == x, same stride): the same bits, gaps of x untouched
    assert _rope_call(x_buf, x_buf, cos, sin, tokens, heads, D, S, sign, x_tok, x_tok) == 0
    assert torch.equal(_bits(x_buf[:, :hd]), _bits(y_buf[:, :hd])), f"{tag}: in place differs"
    gap = _bits(x_buf[:, hd:])
    assert torch.equal(gap, torch.full_like(gap, 0x7FC1)), f"{tag}: gap of x written in place"


# ---- cross-entropy ----------------------------------------------------------
_XENT_ROWS = {       # (label, kind) per row
    (3, 8): [(0, "normal"), (7, "spread"), (-100, "normal")],
    (5, 2056): [(0, "normal"), (2055, "dominant"), (2047, "spread"), (2048, "normal"),
                (-100, "normal")],
    (4, 4104): [(2047, "normal"), (2048, "dominant"), (4103, "spread"), (-100, "spread")],
}


def _xent_logits(T, V, dev):
    """3 randn logits; 'spread' rows span +-60, in 'dominant' rows the label
    logit is 40 (p ~ 1)."""
    rows = _XENT_ROWS[(T, V)]
    x = _randn((T, V), dev, 41) * 3
    g = _gen(dev, 42)
    for r, (lab, kind) in enumerate(rows):
        if kind == "spread":
            x[r] = torch.linspace(-60, 60, V, device=dev)[torch.randperm(V, device=dev, generator=g)]
        elif kind == "dominant":
            x[r, lab] = 40.0
    labels = torch.tensor([lab for lab, _ in rows], dtype=torch.int64, device=dev)
    return x.bfloat16(), labels


def _xent_run_and_check(tag, x, labels, ld):
    """Forward and in-place backward on a [T, ld] buffer whose padding is
    poisoned; checks lse, row loss, gradient, ignored rows and the padding."""
    L = _lib.lib()
    dev = x.device
    T, V = x.shape
    buf = _poison((T, ld), torch.bfloat16, dev)
    buf[:, :V] = x
    loss = _poison((T,), torch.float32, dev)
    lse = _poison((T,), torch.float32, dev)
    gscale = torch.tensor([1.0 / 3.0], dtype=torch.float32, device=dev)
    g = gscale.double().item()
    assert L.mxk_xent_fwd(buf.data_ptr(), labels.data_ptr(), loss.data_ptr(), lse.data_ptr(), T, V,
                          ld, _stream(dev)) == 0
    assert torch.equal(_bits(buf[:, :V]), _bits(x)), f"{tag}: forward modified the logits"
    pad = _bits(buf[:, V:])
    assert torch.equal(pad, torch.full_like(pad, 0x7FC1)), f"{tag}: forward wrote the padding"
    lse_ref, loss_ref, d_ref, mag = R.xent(x, labels, g)
    assert torch.isfinite(lse_ref).all() and torch.isfinite(d_ref).all()
    _check_stat(f"{tag} lse", lse, lse_ref, lse_ref.abs().clamp_min(1))
    _check_stat(f"{tag} loss", loss, loss_ref, loss_ref.abs().clamp_min(1))
    assert L.mxk_xent_bwd(buf.data_ptr(), labels.data_ptr(), lse.data_ptr(), gscale.data_ptr(), T,
                          V, ld, _stream(dev)) == 0
    keep = labels >= 0
    atol = torch.full_like(mag, ATOL)
    atol[keep, labels[keep]] += 2e-5 * g
    _check(f"{tag} dlogits", buf[:, :V], d_ref, mag, atol=atol)
    pad = _bits(buf[:, V:])
    assert torch.equal(pad, torch.full_like(pad, 0x7FC1)), f"{tag}: backward wrote the padding"
    ign = (~keep).nonzero().flatten().tolist()
    assert ign
    for r in ign:
        assert _bits(loss[r:r + 1]).item() == 0, f"{tag}: loss of ignored row {r}"
        assert not _bits(buf[r, :V]).any(), f"{tag}: gradient of ignored row {r} not all zero bits"


@pytest.mark.parametrize("T,V", list(_XENT_ROWS))
def test_xent_elementwise(cuda_device, T, V):
    """Labels at 0, V-1, 2047, 2048 and an ignored row; +-60 spread and p ~ 1
    rows; lse and the row loss checked as fp32 statistics."""
    x, labels = _xent_logits(T, V, cuda_device)
    _xent_run_and_check(f"xent[{T}x{V}]", x, labels, V)


def test_xent_strided_rows(cuda_device):
    """ld = V + 24: padding bit-identical after forward and backward."""
    T, V = 5, 2056
    x, labels = _xent_logits(T, V, cuda_device)
    _xent_run_and_check(f"xent[{T}x{V},ld={V + 24}]", x, labels, V + 24)


@pytest.mark.parametrize("T,V", [(5, 2056), (4, 4104)])
def test_xent_masked_logits(cuda_device, T, V):
    """Aligned runs of eight -inf logits: at the start of a row (thread 0's
    first chunk), filling another thread's whole first chunk, and at the tail.
    A thread whose chunk is all -inf has m = -inf and sum = NaN; the
    m == -inf guards of the folds must discard it."""
    dev = cuda_device
    x = _randn((T, V), dev, 43) * 3
    ninf = float("-inf")
    x[0, 0:8] = ninf
    x[1, 8 * 37:8 * 37 + 8] = ninf
    x[2, V - 8:V] = ninf
    for lo in (0, 8 * 37, V - 8):
        x[3, lo:lo + 8] = ninf
    labs = [2047, 2048, 100, 9] + [-100] * (T - 4)
    if T == 4:                      # keep an ignored row: the first one, masks and all
        labs[0] = -100
    labels = torch.tensor(labs, dtype=torch.int64, device=dev)
    _xent_run_and_check(f"xent-masked[{T}x{V}]", x.bfloat16(), labels, V)


def test_xent_wrapper(cuda_device):
    """mxk8s.ops.xent.cross_entropy: all rows ignored gives loss 0 and
    gradient 0 (the documented clamp_min(1)); a normal batch matches fp64 to
    1e-5 relative."""
    from mxk8s.ops.xent import cross_entropy
    T, V = 5, 2056
    x, labels = _xent_logits(T, V, cuda_device)
    lg = x.clone().requires_grad_()
    loss = cross_entropy(lg, torch.full_like(labels, -100))
    loss.backward()
    assert loss.item() == 0 and not _bits(lg.grad).any()
    lg = x.clone().requires_grad_()
    loss = cross_entropy(lg, labels)
    count = int((labels >= 0).sum())
    _, rows_ref, d_ref, mag = R.xent(x, labels, 1.0 / count)
    ref = rows_ref.sum().item() / count
    ratio = abs(loss.item() - ref) / (1e-5 * abs(ref))
    print(f"RATIO xent-wrapper loss {ratio:.3g}")
    assert ratio <= 1, f"mean loss: error / bound = {ratio:.3g}"
    loss.backward()
    keep = labels >= 0
    atol = torch.full_like(mag, ATOL)
    atol[keep, labels[keep]] += 2e-5 / count
    _check("xent-wrapper dlogits", lg.grad, d_ref, mag, atol=atol)


# ---- contracts: a violation returns non-zero and launches nothing -----------
def _unchanged(outs):
    return all(torch.equal(_bits(o), torch.full_like(_bits(o), 0x7FC1 if o.element_size() == 2
                                                     else 0x7FC12345)) for o in outs)


class _RmsArgs:
    """Valid arguments of the three RMSNorm launchers with poisoned outputs;
    every buffer has 8 elements of slack so that a pointer can be offset."""

    def __init__(self, dev, rows=4, H=64, H_alloc=None):
        n = rows * (H_alloc or H) + 8
        bf = lambda: torch.zeros(n, dtype=torch.bfloat16, device=dev)   # noqa: E731
        self.rows, self.H, self.dev = rows, H, dev
        self.x, self.delta, self.w, self.dy, self.dres = bf(), bf(), bf(), bf(), bf()
        self.rstd_in = torch.ones(rows + 8, dtype=torch.float32, device=dev)
        self.y, self.h, self.dx = (_poison((n,), torch.bfloat16, dev) for _ in range(3))
        self.dw_bf16 = _poison((n,), torch.bfloat16, dev)
        self.rstd = _poison((rows + 8,), torch.float32, dev)
        self.dw_f32 = _poison((n,), torch.float32, dev)
        self.ws = _poison((rows * (H_alloc or H) + 8,), torch.float32, dev)
        self.outs = [self.y, self.h, self.dx, self.dw_bf16, self.rstd, self.dw_f32, self.ws]

    def p(self, name, off):
        return getattr(self, name).data_ptr() + off.get(name, 0)

    def fwd(self, off=None, rows=None, H=None):
        off = off or {}
        return _lib.lib().mxk_rmsnorm_fwd(
            self.p("x", off), self.p("w", off), self.p("y", off), self.p("rstd", off),
            self.rows if rows is None else rows, H or self.H, EPS, _stream(self.dev))

    def add_fwd(self, off=None, rows=None, H=None):
        off = off or {}
        return _lib.lib().mxk_add_rmsnorm_fwd(
            self.p("x", off), self.p("delta", off), self.p("w", off), self.p("h", off),
            self.p("y", off), self.p("rstd", off), self.rows if rows is None else rows,
            H or self.H, EPS, _stream(self.dev))

    def bwd(self, off=None, rows=None, H=None, with_dres=True):
        off = off or {}
        return _lib.lib().mxk_rmsnorm_bwd(
            self.p("dy", off), self.p("x", off), self.p("w", off), self.p("rstd_in", off),
            self.p("dres", off) if with_dres else None, self.p("dx", off), self.p("dw_bf16", off),
            self.p("dw_f32", off), self.p("ws", off), self.rows if rows is None else rows,
            H or self.H, _stream(self.dev))


def test_rmsnorm_contract_sizes(cuda_device):
    a = _RmsArgs(cuda_device)
    assert a.fwd() == 0 and a.add_fwd() == 0 and a.bwd() == 0      # the arguments are valid
    a = _RmsArgs(cuda_device)
    for call in (a.fwd, a.add_fwd, a.bwd):
        assert call(H=12) == INVALID                # H % 8
        assert call(rows=0) == 0 and call(rows=-3) == 0
    assert _unchanged(a.outs)
    big = _RmsArgs(cuda_device, rows=1, H=16392)     # H > 16384: backward only
    assert big.bwd() == INVALID
    assert _unchanged(big.outs)
    assert big.fwd() == 0


@pytest.mark.parametrize("H,rows", [(64, 4), (2048, 1024)], ids=["general", "wave-shape"])
def test_rmsnorm_contract_misaligned_pointers(cuda_device, H, rows):
    """Every pointer the kernels read or write 16 B at a time, offset by one
    bf16 element: rejected, nothing written.  (2048, 1024) is a shape the
    backward would give to the wave kernel."""
    a = _RmsArgs(cuda_device, rows=rows, H=H)
    for name in ("x", "w", "y"):
        assert a.fwd(off={name: 2}) == INVALID, name
    for name in ("x", "delta", "w", "h", "y"):
        assert a.add_fwd(off={name: 2}) == INVALID, name
    for name in ("dy", "x", "w", "dres", "dx"):
        assert a.bwd(off={name: 2}) == INVALID, name
    assert a.bwd(off={"w": 2}, with_dres=False) == INVALID
    assert a.bwd(off={"ws": 4}) == INVALID           # the dw slab is stored as float4
    assert _unchanged(a.outs)


def test_swiglu_contract(cuda_device):
    dev = cuda_device
    L = _lib.lib()
    gu = torch.zeros(4 * 32 + 8, dtype=torch.bfloat16, device=dev)
    dh = torch.zeros(4 * 16 + 8, dtype=torch.bfloat16, device=dev)
    h = _poison((4 * 16 + 8,), torch.bfloat16, dev)
    dgu = _poison((4 * 32 + 8,), torch.bfloat16, dev)
    s = _stream(dev)
    assert L.mxk_swiglu_fwd(gu.data_ptr(), h.data_ptr(), 4, 12, s) == INVALID       # F % 8
    assert L.mxk_swiglu_bwd(gu.data_ptr(), dh.data_ptr(), dgu.data_ptr(), 4, 12, s) == INVALID
    assert L.mxk_swiglu_fwd(gu.data_ptr() + 2, h.data_ptr(), 4, 16, s) == INVALID
    assert L.mxk_swiglu_fwd(gu.data_ptr(), h.data_ptr() + 2, 4, 16, s) == INVALID
    assert L.mxk_swiglu_bwd(gu.data_ptr(), dh.data_ptr() + 2, dgu.data_ptr(), 4, 16, s) == INVALID
    assert L.mxk_swiglu_bwd(gu.data_ptr(), dh.data_ptr(), dgu.data_ptr() + 2, 4, 16, s) == INVALID
    for rows in (0, -1):
        assert L.mxk_swiglu_fwd(gu.data_ptr(), h.data_ptr(), rows, 16, s) == 0
        assert L.mxk_swiglu_bwd(gu.data_ptr(), dh.data_ptr(), dgu.data_ptr(), rows, 16, s) == 0
    assert _unchanged([h, dgu])


def test_rope_contract(cuda_device):
    dev = cuda_device
    tokens, heads = 3, 2
    x = torch.zeros(tokens * 160, dtype=torch.bfloat16, device=dev)
    y = _poison((tokens * 160,), torch.bfloat16, dev)
    cos = torch.ones(64, dtype=torch.float32, device=dev)
    sin = torch.zeros(64, dtype=torch.float32, device=dev)

    def call(D, x_tok, y_tok, toks=tokens):
        return _rope_call(x, y, cos, sin, toks, heads, D, 1, 1.0, x_tok, y_tok)

    assert call(24, 48, 48) == INVALID               # D % 16
    assert call(32, 68, 64) == INVALID               # x_tok % 8
    assert call(32, 64, 68) == INVALID               # y_tok % 8
    assert call(32, 64, 56) == INVALID               # y_tok < heads * D
    assert call(32, 56, 64) == INVALID               # x_tok < heads * D
    assert call(32, 64, 64, toks=0) == 0 and call(32, 64, 64, toks=-2) == 0
    assert _unchanged([y])
    assert call(32, 64, 64) == 0                      # the valid call does write
    assert not _unchanged([y])


def test_xent_contract(cuda_device):
    dev = cuda_device
    L = _lib.lib()
    T = 3
    buf = _poison((T * 32,), torch.bfloat16, dev)    # also an output: the backward is in place
    labels = torch.zeros(T, dtype=torch.int64, device=dev)
    loss = _poison((T,), torch.float32, dev)
    lse = _poison((T,), torch.float32, dev)
    lse_in = torch.zeros(T, dtype=torch.float32, device=dev)
    g = torch.ones(1, dtype=torch.float32, device=dev)
    s = _stream(dev)

    def fwd(rows, V, ld):
        return L.mxk_xent_fwd(buf.data_ptr(), labels.data_ptr(), loss.data_ptr(), lse.data_ptr(),
                              rows, V, ld, s)

    def bwd(rows, V, ld):
        return L.mxk_xent_bwd(buf.data_ptr(), labels.data_ptr(), lse_in.data_ptr(), g.data_ptr(),
                              rows, V, ld, s)

    for call in (fwd, bwd):
        assert call(T, 12, 16) == INVALID            # V % 8
        assert call(T, 8, 12) == INVALID             # ld % 8
        assert call(0, 8, 8) == 0 and call(-1, 8, 8) == 0
    assert _unchanged([buf, loss, lse])
