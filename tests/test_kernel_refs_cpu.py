"""The fp64 closed forms in ``tests/kernel_refs.py`` against ``torch.autograd``
(and ``torch.optim.AdamW``) in float64: the GPU numerics tests compare the HIP
kernels with these forms, so a wrong form must not be able to hide a wrong
kernel.  Tolerance 1e-12 relative to ``mag`` (fp64 round-off is 1.1e-16 per
operation; the forms are a handful of operations and sums of at most 64
terms).

The two SwiGLU-epilogue GEMMs (``dgrad_swiglu``, ``w13_swiglu``) come with a
bound per element instead of ``mag``.  Their forms are checked against
autograd as the others; their bounds are checked here against a float32
emulation of each epilogue written as the kernel writes it (``exp2``, a
reciprocal, the same association, bf16 rounding): the emulation must stay
inside the bounds on both input families, every planted defect must leave them
on the tight family, and on the tight family the bound must be bf16 rounding
and little else (``loose_fraction`` <= 10 %, from the reference alone).
``tests/test_gpu_swiglu_gemm_numerics.py`` derives the bounds.

The plain and the RoPE-epilogue GEMM (``gemm_plain``, ``gemm_rope``;
``tests/test_gpu_gemm_numerics.py`` derives their bounds) are checked the same
way, with the *exact* family next to tight and signed: the unmutated emulation
is bit-equal on it, every planted defect changes bits, and the conditions the
GPU tests assert from the reference alone (max S <= 256, ``loose_fraction``)
hold for every shape they use.  Which family catches which planted defect
(asserted at 1, 5, 16 and 19 K-tiles):

  drop_last_ktile    tight (a whole K-tile is 5 % of |d| at K = 1216) and exact
  drop_k, dup_k,     exact at every K (the one asserted); tight surely only
  swap_chunks        while one term of K is above bf16 rounding (2^-8): at
                     K = 1216 a term is 2^-10 |d| on average and tight sees
                     it by luck, where an element's own rounding error is large
  stale_b            tight and exact
  transpose_c16      tight (row and column scales differ) and exact
  split_half_twice   tight and exact
  partner_32, pos_off_64, head_past
                     exact with the quarter-turn table (bits), and signed with
                     the model's tables (its bound)"""
import functools

import pytest
import torch
import torch.nn.functional as F

import kernel_refs as R

RTOL = 1e-12


def _r(shape, seed):
    return torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def _close(got, ref, mag, what):
    ratio = ((got - ref).abs() / (RTOL * mag + 1e-300)).max().item()
    assert ratio <= 1, f"{what}: error / bound = {ratio:.3g}"
    assert (mag >= ref.abs() * (1 - 1e-12)).all(), f"{what}: mag below |ref|"


@pytest.mark.parametrize("rows,H", [(1, 8), (5, 24), (7, 64)])
@pytest.mark.parametrize("with_res", [False, True])
def test_rmsnorm_forms(rows, H, with_res):
    eps = 1e-5
    x = _r((rows, H), 1) * (2.0 ** (torch.arange(rows) % 5 - 2))[:, None].double()
    if rows > 2:
        x[1] = 0           # rstd = eps^-1/2
        x[2] *= 2.0 ** -10  # eps decides
    w, dy, dres = _r(H, 2), _r((rows, H), 3), _r((rows, H), 4)
    xa, wa = x.clone().requires_grad_(), w.clone().requires_grad_()
    ya = xa * torch.rsqrt(xa.pow(2).mean(-1, keepdim=True) + eps) * wa
    y, rs, mag_y = R.rmsnorm_fwd(x, w, eps)
    _close(y, ya.detach(), mag_y, "y")
    _close(rs, torch.rsqrt(x.pow(2).mean(-1) + eps), rs, "rstd")
    if rows > 2:
        assert rs[1].item() == pytest.approx(eps ** -0.5, rel=1e-14)
    # the residual stream is an identity branch beside the norm: its gradient
    # dres adds to dx
    outs, grads = ([ya, xa * 1.0], [dy, dres]) if with_res else ([ya], [dy])
    gx, gw = torch.autograd.grad(outs, [xa, wa], grads)
    dx, mag_dx, dw, mag_dw = R.rmsnorm_bwd(dy, x, w, eps, dres if with_res else None)
    _close(dx, gx, mag_dx, "dx")
    _close(dw, gw, mag_dw, "dw")


@pytest.mark.parametrize("rows,Fd", [(1, 8), (3, 40)])
def test_swiglu_forms(rows, Fd):
    g = _r((rows, Fd), 5) * 3
    special = torch.tensor([0.0, -0.0, 2.0 ** -20, -2.0 ** -20, -1.278, 20, -20, 88, -88, 200, -200],
                           dtype=torch.float64)
    g.view(-1)[:min(g.numel(), special.numel())] = special[:g.numel()]
    u, dh = _r((rows, Fd), 6), _r((rows, Fd), 7)
    ga, ua = g.clone().requires_grad_(), u.clone().requires_grad_()
    ha = F.silu(ga) * ua
    gg, gu = torch.autograd.grad(ha, [ga, ua], dh)
    h, mag_h = R.swiglu_fwd(g, u)
    _close(h, ha.detach(), mag_h, "h")
    dg, mag_dg, du, mag_du = R.swiglu_bwd(g, u, dh)
    _close(dg, gg, mag_dg, "dg")
    _close(du, gu, mag_du, "du")
    assert torch.isfinite(dg).all() and torch.isfinite(du).all()


@pytest.mark.parametrize("B,S,heads,D", [(1, 1, 1, 16), (2, 5, 3, 32)])
def test_rope_forms(B, S, heads, D):
    x = _r((B * S, heads, D), 8)
    ang = _r((S, D // 2), 9) * 3
    cos, sin = ang.cos(), ang.sin()
    # complex form: (a + i b) (c + i sign s), position t mod S
    pos = torch.arange(B * S) % S
    z = torch.complex(x[..., :D // 2], x[..., D // 2:])
    for sign in (1.0, -1.0):
        rot = torch.complex(cos[pos], sign * sin[pos])[:, None, :]
        zr = z * rot
        y, mag = R.rope(x, cos, sin, sign, S)
        _close(y, torch.cat([zr.real, zr.imag], -1), mag, f"rope sign {sign}")
    # sign -1 is the backward (transpose) of sign +1
    xa = x.clone().requires_grad_()
    c, s = cos[pos][:, None, :], sin[pos][:, None, :]
    a, b = xa[..., :D // 2], xa[..., D // 2:]
    ya = torch.cat([a * c - b * s, b * c + a * s], -1)
    dy = _r(x.shape, 10)
    (gx,) = torch.autograd.grad(ya, xa, dy)
    back, mag = R.rope(dy, cos, sin, -1.0, S)
    _close(back, gx, mag, "rope backward")
    # distinct table rows give distinct outputs for the same input vector
    if S > 1:
        same = torch.ones((S, 1, D), dtype=torch.float64)
        ys, _ = R.rope(same, cos, sin, 1.0, S)
        assert len({tuple(r.flatten().tolist()) for r in ys}) == S


@pytest.mark.parametrize("T,V", [(3, 8), (6, 40)])
def test_xent_forms(T, V):
    x = _r((T, V), 11) * 3
    labels = torch.arange(T) * 7 % V
    labels[-1] = -100
    labels[0] = V - 1
    if T > 3:
        x[1, :8] = float("-inf")          # masked run, label elsewhere
        labels[1] = 9
        x[2] = torch.linspace(-60, 60, V, dtype=torch.float64)
        x[3, labels[3]] = 40.0            # p ~ 1
    g = 0.37
    xa = x.clone().requires_grad_()
    rows = F.cross_entropy(xa, labels, ignore_index=-100, reduction="none")
    (gx,) = torch.autograd.grad(rows.sum() * g, xa)
    lse, loss, dl, mag = R.xent(x, labels, g)
    _close(lse, torch.logsumexp(x, -1), lse.abs(), "lse")
    _close(loss, rows.detach(), lse.abs() + 60, "row loss")
    _close(dl, gx, mag, "dlogits")
    assert loss[-1].item() == 0 and not dl[-1].any()
    assert torch.isfinite(dl).all() and torch.isfinite(loss).all()
    # mean over counted rows, the wrapper's reduction
    mean = F.cross_entropy(x, labels, ignore_index=-100)
    assert (loss.sum() / (labels >= 0).sum()).item() == pytest.approx(mean.item(), rel=1e-13)


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("scale", [1.0, 0.25])
def test_adamw_form_vs_torch_optim(step, wd, scale):
    n = 37
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    p, m, v, grad = _r(n, 12), _r(n, 13) * 0.1, (_r(n, 14) * 0.1).pow(2), _r(n, 15)
    par = torch.nn.Parameter(p.clone())
    opt = torch.optim.AdamW([par], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    opt.state[par] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(),
                      "exp_avg_sq": v.clone()}
    par.grad = grad * scale
    opt.step()
    st = opt.state[par]
    assert int(st["step"].item()) == step
    p1, m1, v1, mag_p, mag_m, mag_v = R.adamw_step(p, m, v, grad, lr, b1, b2, eps, wd, step, scale)
    _close(m1, st["exp_avg"], mag_m, "exp_avg")
    _close(v1, st["exp_avg_sq"], mag_v, "exp_avg_sq")
    _close(p1, par.detach(), mag_p, "param")


# ---- the SwiGLU-epilogue GEMMs ------------------------------------------------
def test_swiglu_gemm_forms_vs_autograd():
    M, Fd, K = 6, 10, 12
    dy, w2, gu = _r((M, K), 21), _r((K, Fd), 22), _r((M, 2 * Fd), 23) * 3
    gu[0, :4] = torch.tensor([0.0, -1.2785, 40.0, -40.0], dtype=torch.float64)
    ga = gu.clone().requires_grad_()
    ((F.silu(ga[:, :Fd]) * ga[:, Fd:]) @ w2.t()).backward(dy)
    dg, bound_dg, du, bound_du = R.dgrad_swiglu(dy, w2, gu)
    g, u = gu[:, :Fd], gu[:, Fd:]
    t = (dy @ w2) * u * torch.sigmoid(g)
    _close(torch.cat([dg, du], -1), ga.grad, torch.cat([t.abs() * (1 + g.abs()), du.abs()], -1), "dgu")
    assert (bound_dg >= 2.0 ** -8 * dg.abs()).all() and (bound_du >= 2.0 ** -8 * du.abs()).all()
    x, w13 = _r((M, K), 24), _r((2 * Fd, K), 25)
    gu2, bound_gu, h, bound_h = R.w13_swiglu(x, w13)
    acc = x @ w13.t()
    g = acc[:, :Fd]
    _close(gu2, acc, x.abs() @ w13.t().abs(), "gu")
    _close(h, F.silu(g) * acc[:, Fd:], h.abs(), "h")
    assert (bound_gu >= 2.0 ** -8 * gu2.abs()).all() and (bound_h >= 2.0 ** -8 * h.abs()).all()
    # the derivative that bound_h weighs delta_g with is silu'
    ga = g.clone().requires_grad_()
    (gs,) = torch.autograd.grad(F.silu(ga).sum(), ga)
    _close(torch.sigmoid(g) * (1 + g * torch.sigmoid(-g)), gs, 1 + g.abs(), "silu'")


DGRAD_CPU_SHAPES = [(256, 256, 64), (512, 512, 320), (256, 256, 1024)]
W13_CPU_SHAPES = [(256, 128, 64), (512, 384, 320), (256, 128, 448)]
DGRAD_MUTATIONS = ["rows_up_4", "u_offset", "swap_64_127", "drop_last_ktile", "sigmoid_neg", "f_plus"]
W13_MUTATIONS = ["u_offset", "swap_64_127", "drop_last_ktile", "sigmoid_neg"]


@functools.lru_cache(maxsize=None)
def _dgrad_case(M, Fd, K, family):
    inputs = R.dgrad_inputs(M, Fd, K, family)
    return inputs, R.dgrad_swiglu(*inputs)


@functools.lru_cache(maxsize=None)
def _w13_case(M, Fd, K, family):
    inputs = R.w13_inputs(M, Fd, K, family)
    return inputs, R.w13_swiglu(*inputs)


def test_swiglu_gemm_inputs_are_structured():
    (dy, w2, gu), (dg, _, du, _) = _dgrad_case(256, 256, 64, "tight")
    Fd = 256
    assert (dy >= 0).all() and not dy[R.DGRAD_ZERO_ROW].any() and not w2[:, R.DGRAD_ZERO_COL].any()
    assert ((w2 >= 0).all(0) | (w2 <= 0).all(0)).all() and (w2 < 0).any() and (w2 > 0).any()
    for i, v in enumerate(R.DGRAD_G_COLUMNS):
        assert (gu[:, R.dgrad_g_column(i)] == torch.tensor(v).bfloat16()).all()
    assert not gu[R.DGRAD_U_ZERO_ROW, Fd:].any() and not gu[:, Fd + R.DGRAD_U_ZERO_COL].any()
    assert gu[:, :Fd].abs().max() <= 250
    for family in ("tight", "signed"):
        (x, w13), (gu_ref, _, _, _) = _w13_case(256, 128, 448, family)
        assert 32 < gu_ref.abs().max() <= 64
        assert not x[R.W13_ZERO_X_ROW].any() and not w13[R.W13_ZERO_W_ROW].any()
    (x, w13), _ = _w13_case(256, 128, 448, "tight")
    assert (x >= 0).all() and ((w13 >= 0).all(1) | (w13 <= 0).all(1)).all()
    # no operand product near the flush-to-zero range
    for a, b in ((dy, w2), (x, w13)):
        assert a[a != 0].abs().min().double() * b[b != 0].abs().min().double() > 2.0 ** -60


@pytest.mark.parametrize("family", ["tight", "signed"])
@pytest.mark.parametrize("M,Fd,K", DGRAD_CPU_SHAPES)
def test_dgrad_swiglu_emulation_within_bounds(M, Fd, K, family):
    inputs, (dg, bound_dg, du, bound_du) = _dgrad_case(M, Fd, K, family)
    got_dg, got_du = R.dgrad_swiglu_emulated(*inputs)
    for what, got, ref, bound in (("dg", got_dg, dg, bound_dg), ("du", got_du, du, bound_du)):
        ratio = R.bound_ratio(got, ref, bound)
        print(f"RATIO emulated dgrad[{M}x{Fd}x{K},{family}] {what} {ratio:.3g}")
        assert ratio <= 1, f"{what}: error / bound = {ratio:.3g}"
        if family == "tight":
            loose = R.loose_fraction(ref, bound)
            print(f"LOOSE dgrad[{M}x{Fd}x{K}] {what} {loose:.3f}")
            assert loose <= 0.10, f"{what}: {loose:.3f} of the bounds are not bf16 rounding alone"


@pytest.mark.parametrize("mutation", DGRAD_MUTATIONS)
@pytest.mark.parametrize("M,Fd,K", DGRAD_CPU_SHAPES)
def test_dgrad_swiglu_bounds_catch(M, Fd, K, mutation):
    inputs, (dg, bound_dg, du, bound_du) = _dgrad_case(M, Fd, K, "tight")
    got_dg, got_du = R.dgrad_swiglu_emulated(*inputs, mutation=mutation)
    ratio = max(R.bound_ratio(got_dg, dg, bound_dg), R.bound_ratio(got_du, du, bound_du))
    assert ratio > 1, f"{mutation} stays inside the bounds ({ratio:.3g})"


@pytest.mark.parametrize("family", ["tight", "signed"])
@pytest.mark.parametrize("M,Fd,K", W13_CPU_SHAPES)
def test_w13_swiglu_emulation_within_bounds(M, Fd, K, family):
    inputs, (gu, bound_gu, h, bound_h) = _w13_case(M, Fd, K, family)
    got_gu, got_h = R.w13_swiglu_emulated(*inputs)
    for what, got, ref, bound in (("gu", got_gu, gu, bound_gu), ("h", got_h, h, bound_h)):
        ratio = R.bound_ratio(got, ref, bound)
        print(f"RATIO emulated w13[{M}x{Fd}x{K},{family}] {what} {ratio:.3g}")
        assert ratio <= 1, f"{what}: error / bound = {ratio:.3g}"
        if family == "tight":
            loose = R.loose_fraction(ref, bound)
            print(f"LOOSE w13[{M}x{Fd}x{K}] {what} {loose:.3f}")
            assert loose <= 0.10, f"{what}: {loose:.3f} of the bounds are not bf16 rounding alone"


@pytest.mark.parametrize("mutation", W13_MUTATIONS)
@pytest.mark.parametrize("M,Fd,K", W13_CPU_SHAPES)
def test_w13_swiglu_bounds_catch(M, Fd, K, mutation):
    inputs, (gu, bound_gu, h, bound_h) = _w13_case(M, Fd, K, "tight")
    got_gu, got_h = R.w13_swiglu_emulated(*inputs, mutation=mutation)
    ratio = max(R.bound_ratio(got_gu, gu, bound_gu), R.bound_ratio(got_h, h, bound_h))
    assert ratio > 1, f"{mutation} stays inside the bounds ({ratio:.3g})"


# ---- the plain and the RoPE-epilogue GEMM --------------------------------------
# (the module docstring lists which family catches which planted defect)
GEMM_CPU_SHAPES = [(256, 256, 64), (512, 768, 320), (256, 256, 1216)]
GEMM_SINGLE_K = ("drop_k", "dup_k", "swap_chunks")


@functools.lru_cache(maxsize=4)
def _gemm_case(M, N, K, family):
    a, b = R.gemm_inputs(M, N, K, family)
    return (a, b), R.gemm_plain(a, b)


def _bit_equal(got, ref):
    return torch.equal(got.bfloat16().view(torch.int16), ref.bfloat16().view(torch.int16))


def test_gemm_form_and_inputs():
    a, b = _r((6, 12), 31), _r((12, 10), 32)
    d, bound, S = R.gemm_plain(a, b)
    _close(d, torch.einsum("mk,kn->mn", a, b), S, "d")
    assert (bound >= 2.0 ** -8 * d.abs()).all()
    a, b = R.gemm_inputs(256, 256, 64, "tight")
    assert (a >= 0).all() and ((b >= 0).all(0) | (b <= 0).all(0)).all() and (b < 0).any() and (b > 0).any()
    for family in ("tight", "signed"):
        a, b = R.gemm_inputs(256, 256, 64, family)
        assert not a[R.GEMM_A_ZERO[0]].any() and not a[:, R.GEMM_A_ZERO[1]].any()
        assert not b[R.GEMM_B_ZERO[0]].any() and not b[:, R.GEMM_B_ZERO[1]].any()
        nz = torch.cat([a[a != 0].abs().double(), b[b != 0].abs().double()])
        # [2^-4, 1.5) times a scale in [2^-4, 2^4], rounded to bf16
        assert nz.min() >= 2.0 ** -8 and nz.max() <= 1.5 * 2.0 ** 4
    a, b = R.gemm_inputs(1, 1, 1, "signed")
    assert a.item() != 0 and b.item() != 0
    assert not torch.equal(R.gemm_inputs(256, 256, 64, "exact")[0],
                           R.gemm_inputs(256, 256, 64, "exact", 1)[0])
    cos, sin = R.quarter_turn_tables(256)
    assert cos.dtype == torch.float32 and ((cos.abs() + sin.abs()) == 1).all() and (cos * sin == 0).all()
    turns = (cos + 2 * sin).long()               # 1, 2, -1, -2
    assert sorted(turns.unique().tolist()) == [-2, -1, 1, 2]
    # rows and frequencies tell apart: no table row equals another, no column either
    assert len({tuple(r.tolist()) for r in turns}) == 256
    assert len({tuple(c.tolist()) for c in turns.t()}) == 64


@pytest.mark.parametrize("M,N,K", R.GEMM_GPU_SHAPES)
def test_gemm_input_conditions_of_every_gpu_shape(M, N, K):
    """What tests/test_gpu_gemm_numerics.py asserts from the reference alone,
    for every shape it uses: max S <= 256 on exact (with at least 18 nonzero
    products per element and every k used, on the tiled shapes), and on tight
    a bound that is bf16 rounding and little else."""
    a, b = R.gemm_inputs(M, N, K, "exact")
    S = a.float().abs() @ b.float().abs()        # integers below 2^24: exact in fp32
    assert S.max().item() <= R.GEMM_EXACT_MAX_S, S.max().item()
    if K >= 64:
        used = (a != 0).float() @ (b != 0).float()
        assert used.min().item() >= 18, used.min().item()
        assert (a != 0).any(0).all() and (b != 0).any(1).all()
    if M * N <= 512 * 1536:
        a, b = R.gemm_inputs(M, N, K, "tight")
        d, bound, S = R.gemm_plain(a, b)
        assert torch.equal(S, d.abs())
        assert R.loose_fraction(d, bound) <= 0.10


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("family", R.GEMM_FAMILIES)
@pytest.mark.parametrize("M,N,K", GEMM_CPU_SHAPES + [(256, 256, 1024)])
def test_gemm_emulation_within_bounds(M, N, K, family, split):
    (a, b), (d, bound, S) = _gemm_case(M, N, K, family)
    got = R.gemm_emulated(a, b, split=split).bfloat16()
    ratio, r, c = R.worst_ratio(got, d, bound)
    print(f"RATIO emulated gemm[{M}x{N}x{K},{family},split{int(split)}] {ratio:.3g}")
    assert ratio <= 1, f"error / bound = {ratio:.3g} at ({r}, {c})"
    if family == "exact":
        assert S.max().item() <= R.GEMM_EXACT_MAX_S and _bit_equal(got, d)


def _gemm_caught(M, N, K, family, mutation):
    (a, b), (d, bound, _) = _gemm_case(M, N, K, family)
    got = R.gemm_emulated(a, b, mutation=mutation).bfloat16()
    return not _bit_equal(got, d) if family == "exact" else R.bound_ratio(got, d, bound) > 1


# one K-tile has no previous stage whose b could be stale
@pytest.mark.parametrize("M,N,K,mutation", [(*s, m) for s in GEMM_CPU_SHAPES + [(256, 256, 1024)]
                                            for m in R.GEMM_MUTATIONS if not (m == "stale_b" and s[2] < 128)])
def test_gemm_checks_catch(M, N, K, mutation):
    caught = {f: _gemm_caught(M, N, K, f, mutation) for f in R.GEMM_FAMILIES}
    print(f"CAUGHT gemm[{M}x{N}x{K}] {mutation} {caught}")
    assert caught["exact"], f"{mutation}: bit-equal on exact"
    # a single term of K = 1216 is 2^-10 |d| on average, under bf16 rounding:
    # tight sees it only where it meets an element whose rounding error is
    # already near the bound, so nothing is asserted of tight there
    if mutation not in GEMM_SINGLE_K:
        assert caught["tight"], f"{mutation}: inside the bound on tight"


@functools.lru_cache(maxsize=None)
def _rope_tables(kind):
    if kind == "quarter":
        return R.quarter_turn_tables(R.GEMM_ROPE_S)
    from mxk8s.ops.fused import rope_tables
    return rope_tables(R.GEMM_ROPE_S, 128)


@functools.lru_cache(maxsize=4)
def _rope_case(N, rope_cols, K, family):
    a, b = R.gemm_inputs(R.GEMM_ROPE_M, N, K, family)
    cos, sin = _rope_tables("quarter" if family == "exact" else "real")
    return (a, b, cos, sin), R.gemm_rope(a, b, cos, sin, R.GEMM_ROPE_S, rope_cols)


def test_gemm_rope_form():
    """gemm_rope is the rotate-half form of ``rope`` (checked against the
    complex product above) applied to the heads below rope_cols."""
    M, N, K, S, rope_cols = 8, 384, 12, 4, 256
    a, b = _r((M, K), 41), _r((K, N), 42)
    ang = _r((S, 64), 43) * 3
    ref, bound = R.gemm_rope(a, b, ang.cos(), ang.sin(), S, rope_cols)
    d = a @ b
    want, mag = R.rope(d[:, :rope_cols].reshape(M, 2, 128), ang.cos(), ang.sin(), 1.0, S)
    _close(ref[:, :rope_cols], want.reshape(M, rope_cols), mag.reshape(M, rope_cols), "rope of d")
    assert torch.equal(ref[:, rope_cols:], d[:, rope_cols:] + 0.0)
    assert (bound >= 2.0 ** -8 * ref.abs()).all()


@pytest.mark.parametrize("family", R.GEMM_FAMILIES)
@pytest.mark.parametrize("K", [64, 320])
@pytest.mark.parametrize("N,rope_cols", R.GEMM_ROPE_COLS)
def test_gemm_rope_emulation_within_bounds(N, rope_cols, K, family):
    inputs, (ref, bound) = _rope_case(N, rope_cols, K, family)
    got = R.gemm_rope_emulated(*inputs, R.GEMM_ROPE_S, rope_cols)
    ratio, r, c = R.worst_ratio(got, ref, bound)
    print(f"RATIO emulated rope[{N}/{rope_cols}x{K},{family}] {ratio:.3g}")
    assert ratio <= 1, f"error / bound = {ratio:.3g} at ({r}, {c})"
    if family == "exact":
        assert _bit_equal(got, ref)


@pytest.mark.parametrize("mutation", R.GEMM_ROPE_MUTATIONS)
@pytest.mark.parametrize("K", [64, 320])
@pytest.mark.parametrize("N,rope_cols", R.GEMM_ROPE_COLS)
def test_gemm_rope_checks_catch(N, rope_cols, K, mutation):
    caught = {}
    for family in ("signed", "exact"):
        inputs, (ref, bound) = _rope_case(N, rope_cols, K, family)
        got = R.gemm_rope_emulated(*inputs, R.GEMM_ROPE_S, rope_cols, mutation=mutation)
        caught[family] = not _bit_equal(got, ref) if family == "exact" else R.bound_ratio(got, ref, bound) > 1
    print(f"CAUGHT rope[{N}/{rope_cols}x{K}] {mutation} {caught}")
    assert caught["exact"] and caught["signed"], caught


def test_ratio_helper_flags_nan_and_scales():
    ref = torch.tensor([1.0, 2.0], dtype=torch.float64)
    assert R.max_ratio(ref.clone(), ref, ref.abs(), 2.0 ** -8, 1e-30) == 0
    assert R.max_ratio(ref * (1 + 2.0 ** -8), ref, ref.abs(), 2.0 ** -8, 0.0) == pytest.approx(1.0)
    assert not R.max_ratio(torch.tensor([1.0, float("nan")]), ref, ref.abs(), 1.0, 1.0) <= 1
    assert R.f32(0.999) == 0.9990000128746033
