"""fp64 closed forms of the memory-bound kernels (``native/kernels/fused_ops.hip``,
``xent.hip``, ``optim.hip``), shared by the GPU numerics tests.

Every function takes tensors of any float dtype on any device, converts them
exactly to fp64 and returns fp64.  Next to each result it returns ``mag``: the
sum of the absolute values of the terms the closed form adds, which is what an
elementwise error bound has to be relative to (``mag == |ref|`` where nothing
cancels).  ``tests/test_kernel_refs_cpu.py`` checks each form against
``torch.autograd`` / ``torch.optim.AdamW`` in float64.

The two bf16 GEMMs with a SwiGLU epilogue have their own section: closed forms
computed on the CPU with a bound per element instead of ``mag``, the inputs the
CPU and GPU tests share, and a float32 emulation of each epilogue.  The plain
bf16 GEMMs and the RoPE-epilogue GEMM follow in the same form, with a third
input family (sparse small integers) on which the output must be bit-equal.
"""
from __future__ import annotations

import math

import torch


def f32(v: float) -> float:
    """The value a C ``float`` argument receives, as an exact Python float."""
    return torch.tensor(v, dtype=torch.float32).double().item()


def max_ratio(got: torch.Tensor, ref: torch.Tensor, mag: torch.Tensor, rel: float,
              atol) -> float:
    """max over elements of |got - ref| / (rel * mag + atol); NaN / inf in
    ``got`` give a ratio that fails ``<= 1``."""
    got = got.double()
    if got.numel() == 0:
        return 0.0
    if not torch.isfinite(got).all():
        return float("inf")
    return ((got - ref).abs() / (rel * mag + atol)).max().item()


# ---------------------------------------------------------------- RMSNorm ---
def rmsnorm_fwd(x, w, eps: float):
    """-> (y, rstd, mag_y) with rstd = (mean(x^2) + eps)^-1/2, y = x rstd w."""
    x, w = x.double(), w.double()
    rs = (x.pow(2).mean(-1) + eps).rsqrt()
    y = x * rs[:, None] * w
    return y, rs, y.abs()


def rmsnorm_bwd(dy, x, w, eps: float, dres=None):
    """-> (dx, mag_dx, dw, mag_dw).
    dx = rs dy w - rs^3 x mean(dy w x) [+ dres];  dw = sum_r dy x rs."""
    dy, x, w = dy.double(), x.double(), w.double()
    rs = (x.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    g = dy * w
    c = (g * x).mean(-1, keepdim=True)
    dx = rs * g - rs.pow(3) * x * c
    mag = rs * g.abs() + rs.pow(3) * x.abs() * c.abs()
    if dres is not None:
        dx = dx + dres.double()
        mag = mag + dres.double().abs()
    t = dy * x * rs
    return dx, mag, t.sum(0), t.abs().sum(0)


# ----------------------------------------------------------------- SwiGLU ---
def swiglu_fwd(g, u):
    """-> (h, mag) with h = g sigmoid(g) u."""
    g, u = g.double(), u.double()
    h = g * torch.sigmoid(g) * u
    return h, h.abs()


def swiglu_bwd(g, u, dh):
    """-> (dg, mag_dg, du, mag_du) with s = sigmoid(g):
    dg = dh u s (1 + g (1 - s)),  du = dh g s."""
    g, u, dh = g.double(), u.double(), dh.double()
    s = torch.sigmoid(g)
    one_minus_s = torch.sigmoid(-g)      # no cancellation for large g
    t = dh * u * s
    dg = t * (1 + g * one_minus_s)
    mag_dg = t.abs() * (1 + g.abs() * one_minus_s)
    du = dh * g * s
    return dg, mag_dg, du, du.abs()


# ------------------------------------------- SwiGLU-epilogue bf16 GEMMs ---
# mxk_gemm_bf16_dgrad_swiglu and mxk_gemm_bf16_w13_swiglu: fp64 on the CPU
# (no GPU BLAS), each result with its per-element error bound.
# tests/test_gpu_swiglu_gemm_numerics.py derives the bounds.
GEMM_ATOL = 1e-30
_LOG2E_F32 = f32(-1.44269504)


def gemm_term(a, b):
    """a [M][K], b [K][N], bf16 values -> (d, S, delta) in fp64 on the CPU:
    d = a b, S = |a| |b|, delta = K 2^-23 S (fp32 accumulation of exact
    products, any order, with a factor 2 of margin)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    S = a.abs() @ b.abs()
    return a @ b, S, a.shape[1] * 2.0 ** -23 * S


def _c(g):
    """Relative error of the fp32 sigmoid chain at g: g * -log2(e) (2^-24
    relative, |g| 2^-24 after exp2), one ulp each of exp2 and rcp, and a
    handful of fp32 multiplies."""
    return (g.abs() + 8) * 2.0 ** -23


def dgrad_swiglu(dy, w2, gu):
    """dy [M][K], w2 [K][F], gu [M][2F] = [g | u] -> (dg, bound_dg, du,
    bound_du) with d = dy w2, s = sigmoid(g), f = 1 + g sigmoid(-g):
    dg = d u s f,  du = d g s."""
    d, _, delta = gemm_term(dy, w2)
    g, u = gu.detach().double().cpu().chunk(2, -1)
    s, f = torch.sigmoid(g), 1 + g * torch.sigmoid(-g)
    c = _c(g)
    dg = d * u * s * f
    du = d * g * s
    # the kernel evaluates f as (g + 1) - g s: its terms are |1 + g| and |g| s
    bound_dg = (2.0 ** -8 * dg.abs() + delta * (u * s * f).abs() +
                c * (d * u * s).abs() * ((1 + g).abs() + g.abs() * s) + GEMM_ATOL)
    bound_du = 2.0 ** -8 * du.abs() + delta * (g * s).abs() + c * du.abs() + GEMM_ATOL
    return dg, bound_dg, du, bound_du


def w13_swiglu(x, w13):
    """x [M][K], w13 [2F][K] = [gate | up] rows -> (gu, bound_gu, h, bound_h)
    with gu = x w13^T and h = silu(g) u from the unrounded g, u."""
    gu, _, delta = gemm_term(x, w13.detach().t())
    g, u = gu.chunk(2, -1)
    delta_g, delta_u = delta.chunk(2, -1)
    s = torch.sigmoid(g)
    dsilu = s * (1 + g * torch.sigmoid(-g))
    h = g * s * u
    bound_gu = 2.0 ** -8 * gu.abs() + delta + GEMM_ATOL
    bound_h = (2.0 ** -8 * h.abs() + delta_g * (u * dsilu).abs() + delta_u * (g * s).abs() +
               _c(g) * h.abs() + GEMM_ATOL)
    return gu, bound_gu, h, bound_h


def bound_ratio(got, ref, bound) -> float:
    """max over elements of |got - ref| / bound; NaN / inf in ``got`` give inf."""
    got = got.detach().double().cpu()
    if not torch.isfinite(got).all():
        return float("inf")
    return ((got - ref).abs() / bound).max().item()


def loose_fraction(ref, bound) -> float:
    """Share of the elements whose bound exceeds 1.05 * 2^-8 |ref| + atol: on
    the tight family at most 10 % may (the bound is then bf16 rounding and
    little else, from the reference alone)."""
    return (bound > 1.05 * 2.0 ** -8 * ref.abs() + GEMM_ATOL).double().mean().item()


# Inputs of the two GEMMs, made on the CPU from a seed (the CPU emulation and
# the GPU tests see the same tensors).  family "tight": every dot product adds
# terms of one sign (S = |d|); "signed": plain signed operands, d cancels.
# Magnitudes lie in [2^-4, 1.5): no product of two operands is below 2^-60.
DGRAD_G_COLUMNS = (0.0, 2.0 ** -20, -1.2785, 17.0, -17.0, -30.0, -87.0, -88.5, -100.0, -126.0, 100.0,
                   128.0)
DGRAD_ZERO_ROW, DGRAD_ZERO_COL = 5, 3          # of dy / of W2
DGRAD_U_ZERO_ROW, DGRAD_U_ZERO_COL = 9, 11


def _operand(shape, gen, signed):
    mag = 2.0 ** -4 + 1.4375 * torch.rand(shape, generator=gen, dtype=torch.float64)
    if not signed:
        return mag
    return mag * torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0)


def _signs(n, gen):
    return torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()


def _pow2(idx, mod, shift):
    return torch.exp2(((idx % mod) - shift).double())


def dgrad_g_column(i: int) -> int:
    """Column of g that holds DGRAD_G_COLUMNS[i] in every row."""
    return 7 + 19 * i


def dgrad_inputs(M: int, F: int, K: int, family: str, seed: int = 0, row0: int = 0):
    """-> bf16 (dy [M][K], w2 [K][F], gu [M][2F]).  dy row r scaled
    2^((r mod 9) - 4), W2 column c scaled 2^((c mod 7) - 3) with a sign per
    column, one zero row of dy and one zero column of W2; g random times
    2^((r mod 5) - 2) with whole columns at DGRAD_G_COLUMNS, u with a
    per-column scale, a zero row and a zero column.  row0 shifts the row
    patterns (two row blocks of one matrix then differ)."""
    assert family in ("tight", "signed") and F >= dgrad_g_column(len(DGRAD_G_COLUMNS) - 1) + 1
    gen = torch.Generator().manual_seed(1000 * seed + row0 + (1 if family == "signed" else 0))
    signed = family == "signed"
    r, c = torch.arange(M) + row0, torch.arange(F)
    dy = _operand((M, K), gen, signed) * _pow2(r, 9, 4)[:, None]
    w2 = _operand((K, F), gen, signed) * (_pow2(c, 7, 3) * _signs(F, gen))[None, :] * 2.0 ** -4
    dy[DGRAD_ZERO_ROW] = 0
    w2[:, DGRAD_ZERO_COL] = 0
    g = torch.randn((M, F), generator=gen, dtype=torch.float64) * _pow2(r, 5, 2)[:, None]
    for i, v in enumerate(DGRAD_G_COLUMNS):
        g[:, dgrad_g_column(i)] = v
    u = _operand((M, F), gen, True) * _pow2(c, 3, 1)[None, :] * _pow2(r, 4, 1)[:, None]
    u[DGRAD_U_ZERO_ROW] = 0
    u[:, DGRAD_U_ZERO_COL] = 0
    return dy.bfloat16(), w2.bfloat16(), torch.cat([g, u], -1).bfloat16()


W13_ZERO_X_ROW, W13_ZERO_W_ROW = 6, 10


def w13_inputs(M: int, F: int, K: int, family: str, seed: int = 0):
    """-> bf16 (x [M][K], w13 [2F][K]).  x row r scaled 2^((r mod 5) - 4),
    W13 row n scaled 2^((n mod 3) - 2) with a sign per output feature, one
    zero row each; x then scaled by the power of two that puts max |gu| in
    (32, 64], so the c(g) term stays small against bf16 rounding.  Seven of
    eight negative gate features are scaled 2^-4 more: for g << 0 the weight
    of delta_g in bound_h, |silu'(g) / silu(g)| |g| = |f| ~ |g|, would exceed
    bf16 rounding, so most negative g stay above -4 and every eighth feature
    still saturates the sigmoid."""
    assert family in ("tight", "signed")
    gen = torch.Generator().manual_seed(1000 * seed + 500 + (1 if family == "signed" else 0))
    signed = family == "signed"
    x = _operand((M, K), gen, signed) * _pow2(torch.arange(M), 5, 4)[:, None]
    n = torch.arange(2 * F)
    sign = _signs(2 * F, gen)
    damp = torch.where((n < F) & (sign < 0) & (n % 8 != 1), 2.0 ** -4, 1.0)
    w = _operand((2 * F, K), gen, signed) * (_pow2(n, 3, 2) * sign * damp)[:, None]
    x[W13_ZERO_X_ROW] = 0
    w[W13_ZERO_W_ROW] = 0
    x, w = x.bfloat16().double(), w.bfloat16().double()
    top = (x @ w.t()).abs().max().item()
    x = x * 2.0 ** (5 - math.floor(math.log2(top)))
    return x.bfloat16(), w.bfloat16()


def dgrad_swiglu_emulated(dy, w2, gu, mutation: str = ""):
    """The kernel's arithmetic in float32 on the CPU: fp32 accumulation, then
    x = g * -log2(e), s = 1 / (1 + exp2(x)), t = d s, du = t g,
    dg = (t u) ((g + 1) - g s), rounded to bf16.  ``mutation`` plants one
    defect (tests/test_kernel_refs_cpu.py lists them)."""
    M, K = dy.shape
    F = w2.shape[1]
    a, b = dy.float(), w2.float()
    if mutation == "drop_last_ktile":
        a, b = a[:, :K - 64], b[:K - 64]
    d = a @ b if a.shape[1] else torch.zeros((M, F))
    g, u = _swiglu_operands(gu.float(), F, mutation)
    one, l2e = torch.tensor(1.0), torch.tensor(_LOG2E_F32, dtype=torch.float32)
    x = g * l2e
    s = one / (one + torch.exp2(-x if mutation == "sigmoid_neg" else x))
    t = d * s
    du = t * g
    fac = one + g * s if mutation == "f_plus" else (g + one) - g * s
    dg = (t * u) * fac
    return dg.bfloat16(), du.bfloat16()


def w13_swiglu_emulated(x, w13, mutation: str = ""):
    """As above for the up-projection: gu = bf16(acc), h = bf16((g s) u) from
    the fp32 accumulators."""
    M, K = x.shape
    F = w13.shape[0] // 2
    a, b = x.float(), w13.float().t()
    if mutation == "drop_last_ktile":
        a, b = a[:, :K - 64], b[:K - 64]
    acc = a @ b if a.shape[1] else torch.zeros((M, 2 * F))
    g, u = _swiglu_operands(acc, F, mutation)
    one, l2e = torch.tensor(1.0), torch.tensor(_LOG2E_F32, dtype=torch.float32)
    x2 = g * l2e
    s = one / (one + torch.exp2(-x2 if mutation == "sigmoid_neg" else x2))
    return acc.bfloat16(), ((g * s) * u).bfloat16()


def _swiglu_operands(gu, F, mutation):
    """(g, u) as the epilogue pairs them with d, under a planted defect."""
    M = gu.shape[0]
    g, u = gu[:, :F].clone(), gu[:, F:].clone()
    rows = torch.arange(M) % 128
    if mutation == "rows_up_4":          # pass 0 (rows 0-31 of a 128-row block) reads 4 rows up
        sel = rows < 32
        g[sel], u[sel] = torch.roll(g, 4, 0)[sel], torch.roll(u, 4, 0)[sel]
    elif mutation == "u_offset":         # u read at column offset F - 128
        u = torch.roll(gu, 128, 1)[:, F:].clone()
    elif mutation == "swap_64_127":      # gate and up exchanged for rows 64-127
        sel = rows >= 64
        g[sel], u[sel] = gu[:, F:][sel], gu[:, :F][sel]
    else:
        assert mutation in ("", "drop_last_ktile", "sigmoid_neg", "f_plus"), mutation
    return g, u


# ---------------------------------- plain and RoPE-epilogue bf16 GEMMs ---
# mxk_gemm_bf16_tn / _tn_variant / _ex* and mxk_gemm_bf16_rope: fp64 on the
# CPU with a bound per element.  tests/test_gpu_gemm_numerics.py derives the
# bounds; the shapes its cases use are listed here, so that
# tests/test_kernel_refs_cpu.py checks the conditions on the inputs for
# exactly those.
GEMM_FAMILIES = ("tight", "signed", "exact")
GEMM_A_ZERO = (5, 3)            # row m and column k of a
GEMM_B_ZERO = (7, 3)            # row k and column n of b
GEMM_EXACT_MAX_S = 256          # integers up to 2^8 are exact in bf16

GEMM_TN_KS = (64, 128, 192, 256, 320, 384, 448, 832, 1216)   # 1-7, 13 and 19 K-tiles
GEMM_TN_SHAPES = ((256, 256), (512, 768))
GEMM_TN_XCD_SHAPE = (4096, 4096, 256)
GEMM_STRIDED_SHAPE = (512, 768, 320)
GEMM_GENERIC_SHAPES = ((1, 1, 1), (17, 33, 65), (255, 257, 63), (256, 256, 64))
GEMM_EX_SHAPES = tuple((256, 512, K) for K in (64, 128, 256)) + \
    tuple((512, 768, K) for K in (192, 320, 448, 1216))
GEMM_EX_XCD_SHAPE = (4096, 4096, 192)
GEMM_SPLIT_SHAPES = ((512, 768, 1024), (256, 256, 1024), (256, 256, 960))
GEMM_ROPE_M, GEMM_ROPE_S = 512, 256
GEMM_ROPE_COLS = ((1536, 1280), (1280, 1152))     # (N, rope_cols)
GEMM_ROPE_KS = (64, 256, 320)
GEMM_LINEAR_SHAPES = ((512, 768, 256), (512, 256, 768), (768, 256, 512))   # fwd, dgrad, wgrad
GEMM_GPU_SHAPES = tuple(dict.fromkeys(
    tuple((M, N, K) for M, N in GEMM_TN_SHAPES for K in GEMM_TN_KS) +
    (GEMM_TN_XCD_SHAPE, GEMM_STRIDED_SHAPE) + GEMM_GENERIC_SHAPES + GEMM_EX_SHAPES +
    (GEMM_EX_XCD_SHAPE,) + GEMM_SPLIT_SHAPES +
    tuple((GEMM_ROPE_M, N, K) for N, _ in GEMM_ROPE_COLS for K in GEMM_ROPE_KS) + GEMM_LINEAR_SHAPES))


def gemm_inputs(M: int, N: int, K: int, family: str, seed: int = 0):
    """-> bf16 (a [M][K], b [K][N]).

    tight / signed: magnitudes in [2^-4, 1.5), a's row r scaled
    2^((r mod 9) - 4), b's column c scaled 2^((c mod 7) - 3) with a sign per
    column; row GEMM_A_ZERO[0] and column GEMM_A_ZERO[1] of a, row
    GEMM_B_ZERO[0] and column GEMM_B_ZERO[1] of b are zero (where the matrix
    has more than 8 of them).  On tight a >= 0 and a column of b has one sign:
    S = |d|.
    exact: an entry is nonzero with probability min(1, sqrt(48 / K)), then
    +-1 or +-2: every partial sum of a dot product is an integer of magnitude
    at most S (asserted <= GEMM_EXACT_MAX_S by the callers), exact in fp32
    and in bf16 in any order."""
    assert family in GEMM_FAMILIES
    if family == "exact":
        gen = torch.Generator().manual_seed(1000 * seed + 902)
        p = min(1.0, math.sqrt(48.0 / K))

        def small(shape):
            nz = (torch.rand(shape, generator=gen) < p).double()
            mag = torch.where(torch.rand(shape, generator=gen) < 0.5, 1.0, 2.0).double()
            return (nz * mag * _signs(shape, gen)).bfloat16()
        return small((M, K)), small((K, N))
    signed = family == "signed"
    gen = torch.Generator().manual_seed(1000 * seed + 900 + (1 if signed else 0))
    a = _operand((M, K), gen, signed) * _pow2(torch.arange(M), 9, 4)[:, None]
    b = _operand((K, N), gen, signed) * (_pow2(torch.arange(N), 7, 3) * _signs(N, gen))[None, :]
    for t, (r, c) in ((a, GEMM_A_ZERO), (b, GEMM_B_ZERO)):
        if t.shape[0] > 8:
            t[r] = 0
        if t.shape[1] > 8:
            t[:, c] = 0
    return a.bfloat16(), b.bfloat16()


def gemm_plain(a, b):
    """a [M][K], b [K][N] -> (d, bound, S): d = a b in fp64 and
    bound = 2^-8 |d| + K 2^-23 S + atol."""
    d, S, delta = gemm_term(a, b)
    d = d + 0.0                       # an exact zero is +0, as a sum that starts from +0
    return d, 2.0 ** -8 * d.abs() + delta + GEMM_ATOL, S


def worst_ratio(got, ref, bound):
    """-> (largest |got - ref| / bound, its row, its column); NaN / inf in
    ``got`` give inf at the first such element."""
    got = got.detach().double().cpu()
    bad = ~torch.isfinite(got)
    ratio = torch.where(bad, torch.full_like(got, float("inf")), (got - ref).abs() / bound)
    i = int(ratio.argmax())
    return ratio.view(-1)[i].item(), i // ratio.shape[1], i % ratio.shape[1]


def quarter_turn_tables(S: int, half: int = 64):
    """-> fp32 (cos, sin) [S][half], each (position, frequency) one of the four
    quarter turns (1, 0), (0, 1), (-1, 0), (0, -1), picked by a hash of both
    indices: rotating exact integers by it is an exact signed permutation."""
    pos, f = torch.arange(S, dtype=torch.int64)[:, None], torch.arange(half, dtype=torch.int64)[None, :]
    h = (pos * 2654435761 + f * 2246822519 + 374761393) & 0xFFFFFFFF
    h = ((h ^ (h >> 15)) * 2246822519) & 0xFFFFFFFF
    turn = ((h ^ (h >> 13)) >> 7) & 3
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[turn]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[turn]
    return cos.contiguous(), sin.contiguous()


def _rope_heads(x, rope_cols):
    """x [M][N] -> (lo, hi) [M][heads][64] of the heads below rope_cols."""
    v = x[:, :rope_cols].reshape(x.shape[0], rope_cols // 128, 2, 64)
    return v[:, :, 0], v[:, :, 1]


def gemm_rope(a, b, cos, sin, S: int, rope_cols: int):
    """The RoPE-epilogue GEMM: d = a b, then in every 128-column head below
    rope_cols, with (x, y) = d[.., i], d[.., i + 64] and (c, s) of row t at
    table row t mod S:  x' = x c - y s,  y' = y c + x s (the fp32 tables are
    exact inputs).  -> (ref, bound) in fp64; columns from rope_cols on carry
    the plain GEMM and its bound."""
    d, bound, _ = gemm_plain(a, b)
    M = d.shape[0]
    pos = torch.arange(M) % S
    c = cos.detach().double().cpu()[pos][:, None, :]
    s = sin.detach().double().cpu()[pos][:, None, :]
    x, y = _rope_heads(d, rope_cols)
    # what the bf16 rounding of the accumulators and their accumulation leave in x, y
    ex, ey = (v - GEMM_ATOL for v in _rope_heads(bound, rope_cols))
    rx = x * c + (-(y * s))           # the kernel's form: the same sign of an exact zero
    ry = y * c + x * s
    bx = (2.0 ** -8 * rx.abs() + c.abs() * ex + s.abs() * ey +
          2.0 ** -23 * ((x * c).abs() + (y * s).abs()) + GEMM_ATOL)
    by = (2.0 ** -8 * ry.abs() + c.abs() * ey + s.abs() * ex +
          2.0 ** -23 * ((y * c).abs() + (x * s).abs()) + GEMM_ATOL)
    ref, bnd = d.clone(), bound.clone()
    ref[:, :rope_cols] = torch.stack([rx, ry], 2).reshape(M, rope_cols)
    bnd[:, :rope_cols] = torch.stack([bx, by], 2).reshape(M, rope_cols)
    return ref, bnd


GEMM_MUTATIONS = ("drop_last_ktile", "drop_k", "dup_k", "swap_chunks", "stale_b", "transpose_c16",
                  "split_half_twice")
GEMM_ROPE_MUTATIONS = ("partner_32", "pos_off_64", "head_past")


def gemm_emulated(a, b, mutation: str = "", split: bool = False):
    """The kernels' arithmetic in float32 on the CPU: fp32 accumulation of
    a [M][K] b [K][N] (``split``: two K halves accumulated apart, then added,
    as the split tail's fixup does), fp32 result.  ``mutation`` plants one
    defect, the single-k ones in rows 16-31 only (one fragment of one wave):
    drop_last_ktile  the last 64 k are not accumulated
    drop_k           k0 = K / 2 + 1 is skipped
    dup_k            a[.., k0] is read again in place of a[.., k0 + 1]
    swap_chunks      the 8-wide chunk of k0 exchanged between rows 16 and 17 of a
    stale_b          the last K-tile multiplies the previous K-tile's b
    transpose_c16    rows 32-47 x columns 16-31 of the result transposed
    split_half_twice the fixup adds the first half's partial twice"""
    a32, b32 = a.float().clone(), b.float().clone()
    K = a32.shape[1]
    k0 = K // 2 + 1
    if mutation == "drop_last_ktile":
        a32[:, K - 64:] = 0
    elif mutation == "drop_k":
        a32[16:32, k0] = 0
    elif mutation == "dup_k":
        a32[16:32, k0 + 1] = a32[16:32, k0]
    elif mutation == "swap_chunks":
        c0 = k0 // 8 * 8
        a32[[16, 17], c0:c0 + 8] = a32[[17, 16], c0:c0 + 8]
    elif mutation == "stale_b":
        b32[K - 64:] = b32[K - 128:K - 64].clone()
    else:
        assert mutation in ("", "transpose_c16", "split_half_twice"), mutation
    if split or mutation == "split_half_twice":
        lo = a32[:, :K // 2] @ b32[:K // 2]
        acc = lo + (lo if mutation == "split_half_twice" else a32[:, K // 2:] @ b32[K // 2:])
    else:
        acc = a32 @ b32
    if mutation == "transpose_c16":
        acc[32:48, 16:32] = acc[32:48, 16:32].t().clone()
    return acc


def gemm_rope_emulated(a, b, cos, sin, S: int, rope_cols: int, mutation: str = ""):
    """mxk_gemm_bf16_rope in float32 on the CPU: the accumulators rounded to
    bf16, then per lane its own 8 columns and the partner's 64 columns away,
    x' = fma(x, c, -(y s)) and y' = fma(y, c, x s) in fp32 (the fma's one
    rounding is made in fp64 here), rounded to bf16.  Mutations:
    partner_32   the partner chunk is read 32 columns away
    pos_off_64   the table row is that of the token 64 rows further down
    head_past    one more head than rope_cols says is rotated"""
    assert mutation in ("",) + GEMM_ROPE_MUTATIONS, mutation
    out = gemm_emulated(a, b).bfloat16()
    M, N = out.shape
    cols = rope_cols + (128 if mutation == "head_past" else 0)
    assert cols <= N
    pos = (torch.arange(M) + (64 if mutation == "pos_off_64" else 0)) % S
    col = torch.arange(128)
    lo = col < 64
    c = cos.float().cpu()[pos][:, None, :][..., col & 63]
    s = sin.float().cpu()[pos][:, None, :][..., col & 63]
    own = out[:, :cols].float().reshape(M, cols // 128, 128)
    par = own[..., col ^ (32 if mutation == "partner_32" else 64)]
    x, y = torch.where(lo, own, par), torch.where(lo, par, own)
    rx = (x.double() * c.double() - (y * s).double()).float()
    ry = (y.double() * c.double() + (x * s).double()).float()
    out[:, :cols] = torch.where(lo, rx, ry).reshape(M, cols).bfloat16()
    return out


# ------------------------------------------------------------------- RoPE ---
def rope(x, cos, sin, sign: float, S: int):
    """x: [tokens, heads, D]; cos / sin: [S, D/2]; token t sits at table row
    t mod S.  Rotate-half pairing (i, i + D/2):
      a' = a c - sign b s,   b' = b c + sign a s.      -> (y, mag)"""
    x = x.double()
    tokens, _, D = x.shape
    half = D // 2
    pos = torch.arange(tokens, device=x.device) % S
    c = cos.double()[pos][:, None, :]
    s = sign * sin.double()[pos][:, None, :]
    a, b = x[..., :half], x[..., half:]
    y = torch.cat([a * c - b * s, b * c + a * s], dim=-1)
    mag = torch.cat([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], dim=-1)
    return y, mag


# ---------------------------------------------------------- cross-entropy ---
def xent(logits, labels, g: float):
    """Rows with a negative label are ignored (loss 0, gradient 0).
    -> (lse, loss_rows, dlogits, mag) with dlogits = g (softmax - onehot) and
    mag = g p, plus g at the label entry."""
    x = logits.double()
    lse = torch.logsumexp(x, dim=-1)
    keep = labels >= 0
    lab = labels.clamp_min(0)
    picked = x.gather(1, lab[:, None])[:, 0]
    loss = torch.where(keep, lse - picked, torch.zeros_like(lse))
    p = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(p).scatter_(1, lab[:, None], 1.0)
    gk = (keep.double() * g)[:, None]
    return lse, loss, gk * (p - onehot), abs(g) * keep.double()[:, None] * (p + onehot)


# ------------------------------------------------------------------ AdamW ---
def adamw_step(p, m, v, grad, lr, b1, b2, eps, wd, step: int, scale: float = 1.0):
    """One decoupled-weight-decay Adam step (torch.optim.AdamW's rule):
      g = scale grad;  m' = b1 m + (1 - b1) g;  v' = b2 v + (1 - b2) g^2
      p' = p (1 - lr wd) - (lr / (1 - b1^step)) m' / (sqrt(v') / sqrt(1 - b2^step) + eps)
    -> (p', m', v', mag_p, mag_m, mag_v)"""
    p, m, v = p.double(), m.double(), v.double()
    g = grad.double() * scale
    m1 = b1 * m + (1 - b1) * g
    mag_m = (b1 * m).abs() + ((1 - b1) * g).abs()
    v1 = b2 * v + (1 - b2) * g * g
    mag_v = (b2 * v).abs() + (1 - b2) * g * g
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    upd = (lr / bc1) * m1 / (v1.sqrt() / bc2 ** 0.5 + eps)
    decayed = p * (1 - lr * wd)
    return decayed - upd, m1, v1, decayed.abs() + upd.abs(), mag_m, mag_v
