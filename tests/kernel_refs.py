"""fp64 closed forms of the memory-bound kernels (``native/kernels/fused_ops.hip``,
``xent.hip``, ``optim.hip``), shared by the GPU numerics tests.

Every function takes tensors of any float dtype on any device, converts them
exactly to fp64 and returns fp64.  Next to each result it returns ``mag``: the
sum of the absolute values of the terms the closed form adds, which is what an
elementwise error bound has to be relative to (``mag == |ref|`` where nothing
cancels).  ``tests/test_kernel_refs_cpu.py`` checks each form against
``torch.autograd`` / ``torch.optim.AdamW`` in float64.
"""
from __future__ import annotations

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
