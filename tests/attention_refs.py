"""fp64 reference of the flash attention (``native/kernels/attention_*.hip``),
the terms of its elementwise error bounds, and the input families that drive
the kernels where a softmax over random data hides errors.  Plain torch on any
device, in the style of ``kernel_refs.py``; shared by
``test_attention_refs_cpu.py`` and ``test_gpu_attention_numerics.py``.

Layouts are the kernels': q / o / dout / dq ``[B, S, Hq, D]``, k / v / dk / dv
``[B, S, Hkv, D]``, lse and the per-row terms ``[B, Hq, S]``.  Query ``i`` sees
key ``j`` under the mask ``(not causal or j <= i) and (doc is None or
doc_start[i] <= j)``; ``doc`` is a ``mxk8s.ops.attention.DocMask``.

Bounds, per element (``eps_i = 2^-16 smag_i`` of the query row ``i``)::

    o       2^-8 |ref| + (2^-8 + eps_i) mag_o + 1e-30
    lse     2^-17 smag_i + 2^-20 max(1, |ref|)
    dv      2^-8 |ref| + (2^-8 + eps) mag_dv + 1e-30
    dq, dk  2^-8 |ref| + (2^-8 + eps) mag + 2^-16 magc + 1e-30

* ``2^-8 |ref|``: round-to-nearest of the bf16 output (half an ulp just above
  a power of two).
* ``2^-8 mag``: P (forward, dV) and dS (dQ, dK) enter the MFMA as bf16, 2^-9 of
  each term; the other 2^-9 covers ``l`` summed from the unrounded terms while
  the numerator sums rounded ones.
* ``eps``: the worst-case fp32 error of a 128-term dot product is
  ``128 * 2^-24 = 2^-17`` of the sum of its terms' magnitudes; it reaches P
  through the exponent, once in the numerator and once in ``l`` / ``lse``.
  ``smag`` is that sum for the scaled score, or ``|lse|`` if larger (the
  shift ``scale s - lse`` is formed in fp32 at that magnitude).
* ``2^-16 magc``: the same for ``dP - delta`` before dS is rounded.
* a key row of dK / dV collects many query rows (of every query head of its
  GQA group): its ``eps`` is the largest ``eps_i`` of the rows that see it.

The terms are derived, not tuned.  ``test_attention_refs_cpu.py`` holds a torch
model of the forward kernel's arithmetic that stays inside the ``o`` and
``lse`` bounds on every family below, and mutants of it that do not.
"""
from __future__ import annotations

import math
import types

import torch

from kernel_refs import f32, max_ratio  # noqa: F401  (re-exported for the tests)

D = 128
TILE = 64                       # keys per tile of the forward / dQ walk
LOG2E = 1.4426950408889634
DEFAULT_SCALE = f32(1.0 / math.sqrt(D))
REL = 2.0 ** -8
ATOL = 1e-30


# ------------------------------------------------------------------ mask ---
def visible(S: int, causal: bool, doc, device) -> torch.Tensor:
    """bool [B or 1, 1, S, S]: query i (dim -2) sees key j (dim -1)."""
    j = torch.arange(S, device=device)
    vis = (j[None, :] <= j[:, None]) if causal else torch.ones(S, S, dtype=torch.bool, device=device)
    vis = vis[None, None]
    if doc is not None:
        vis = vis & doc.bool_mask().to(device)[:, None]
    return vis


def _heads(t: torch.Tensor, group: int = 1) -> torch.Tensor:
    """[B, S, H, D] -> fp64 [B, H * group, S, D]."""
    t = t.double().transpose(1, 2)
    return t.repeat_interleave(group, dim=1) if group > 1 else t


def _smag(aq, ak, vis, scale, lse):
    """max(|scale| max_j sum_d |q_id k_jd| over the visible j, |lse_i|)."""
    t = (aq @ ak.transpose(-1, -2)).masked_fill(~vis, 0.0).amax(-1) * abs(scale)
    return torch.maximum(t, lse.abs())


# ------------------------------------------------------------- reference ---
def attn_fwd_ref(q, k, v, scale: float, causal: bool, doc=None):
    """-> (o [B,S,Hq,D], lse [B,Hq,S], mag_o [B,S,Hq,D], smag [B,Hq,S]), fp64.
    P = softmax(scale q k^T) under the mask, o = P v, lse = ln sum_j exp(scale s_ij),
    mag_o = P |v|, smag as in the module docstring."""
    B, S, Hq, _ = q.shape
    G = Hq // k.shape[2]
    qd, kd, vd = _heads(q), _heads(k, G), _heads(v, G)
    vis = visible(S, causal, doc, q.device)
    s = (qd @ kd.transpose(-1, -2) * scale).masked_fill(~vis, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    del s
    o = p @ vd
    mag = p @ vd.abs()
    del p
    smag = _smag(qd.abs(), kd.abs(), vis, scale, lse)
    return o.transpose(1, 2).contiguous(), lse, mag.transpose(1, 2).contiguous(), smag


def attn_bwd_ref(q, k, v, o, lse, dout, scale: float, causal: bool, doc=None):
    """The backward from what ``attn_bwd`` receives (``o`` and ``lse`` are
    inputs, at whatever precision they come in):

        P = exp(scale s - lse),  delta_i = sum_d dO o,  dP = dO v^T,
        dS = P (dP - delta),  dq = scale dS k,  dk = scale dS^T q,  dv = P^T dO

    dk / dv and their magnitudes summed over the query heads of a GQA group.
    -> namespace of fp64 tensors: dq, mag_dq, magc_dq [B,S,Hq,D]; dk, mag_dk,
    magc_dk, dv, mag_dv [B,S,Hkv,D]; smag [B,Hq,S]; eps_q [B,Hq,S] and eps_k
    [B,Hkv,S] (largest eps of the rows, of every head of the group, that see
    the key)."""
    B, S, Hq, _ = q.shape
    Hkv = k.shape[2]
    G = Hq // Hkv
    a = abs(scale)
    qd, kd, vd = _heads(q), _heads(k, G), _heads(v, G)
    do, od, lse = _heads(dout), _heads(o), lse.double()
    vis = visible(S, causal, doc, q.device)
    s = qd @ kd.transpose(-1, -2) * scale
    p = torch.exp(s - lse[..., None]).masked_fill(~vis, 0.0)
    del s
    delta = (do * od).sum(-1, keepdim=True)
    adelta = (do * od).abs().sum(-1, keepdim=True)
    ds = p * (do @ vd.transpose(-1, -2) - delta)
    pc = p * (do.abs() @ vd.abs().transpose(-1, -2) + adelta)

    def group(t):           # [B, Hq, S, D] -> [B, S, Hkv, D], summed over the group
        return t.view(B, Hkv, G, S, D).sum(2).transpose(1, 2).contiguous()

    def rows(t):
        return t.transpose(1, 2).contiguous()

    r = types.SimpleNamespace()
    r.dq = rows(ds @ kd * scale)
    r.mag_dq = rows(ds.abs() @ kd.abs() * a)
    r.magc_dq = rows(pc @ kd.abs() * a)
    dst, pct = ds.transpose(-1, -2), pc.transpose(-1, -2)
    r.dk = group(dst @ qd * scale)
    r.mag_dk = group(dst.abs() @ qd.abs() * a)
    r.magc_dk = group(pct @ qd.abs() * a)
    del ds, pc, dst, pct
    pt = p.transpose(-1, -2)
    r.dv = group(pt @ do)
    r.mag_dv = group(pt @ do.abs())
    del p, pt
    r.smag = _smag(qd.abs(), kd.abs(), vis, scale, lse)
    r.eps_q = r.smag * 2.0 ** -16
    seen = torch.where(vis, r.eps_q[..., None], r.eps_q.new_zeros(())).amax(-2)   # [B, Hq, S(key)]
    r.eps_k = seen.view(B, Hkv, G, S).amax(2)
    return r


# ---------------------------------------------------------------- bounds ---
def _per_row(t):    # [B, H, S] -> [B, S, H, 1]
    return t.transpose(1, 2)[..., None]


def bound_o(o, mag_o, smag):
    return REL * o.abs() + (REL + _per_row(smag) * 2.0 ** -16) * mag_o + ATOL


def bound_lse(lse, smag):
    return smag * 2.0 ** -17 + 2.0 ** -20 * lse.abs().clamp_min(1.0)


def bound_dv(r):
    return REL * r.dv.abs() + (REL + _per_row(r.eps_k)) * r.mag_dv + ATOL


def bound_dq(r):
    return REL * r.dq.abs() + (REL + _per_row(r.eps_q)) * r.mag_dq + 2.0 ** -16 * r.magc_dq + ATOL


def bound_dk(r):
    return REL * r.dk.abs() + (REL + _per_row(r.eps_k)) * r.mag_dk + 2.0 ** -16 * r.magc_dk + ATOL


def worst(got, ref, bound):
    """(largest |got - ref| / bound, index tuple of that element); a NaN / inf
    in ``got`` gives (inf, its index)."""
    got = got.double()
    bad = ~torch.isfinite(got)
    if bool(bad.any()):
        at = bad.flatten().nonzero()[0].item()
        ratio = torch.full((), float("inf"))
    else:
        rel = (got - ref).abs() / bound
        at = rel.flatten().argmax().item()
        ratio = rel.flatten()[at]
    idx = []
    for n in reversed(got.shape):
        idx.append(at % n)
        at //= n
    return float(ratio), tuple(reversed(idx))


# -------------------------------------------------------- input families ---
# name -> (kind, parameter).  "scale" families are ``random`` at another scale.
FAMILIES = {
    "random": ("random", None),
    "probe+1": ("probe", 1),
    "probe0": ("probe", 0),
    "probe-1": ("probe", -1),
    "probe-64": ("probe", -64),
    "ramp7.5": ("ramp", 7.5),
    "ramp8.5": ("ramp", 8.5),
    "ramp40": ("ramp", 40.0),
    "ramp-7.5": ("ramp", -7.5),
    "ramp-40": ("ramp", -40.0),
    "sawtooth": ("sawtooth", 7.5),
    "offset+300": ("offset", 300.0),
    "offset-300": ("offset", -300.0),
}
DOC_FAMILIES = {
    "random": ("random", None),
    "probe_prev_doc": ("probe_doc", -1),     # the last key of the previous document
    "probe_doc_start": ("probe_doc", 0),     # the first key of the row's own document
    "ramp8.5": ("ramp", 8.5),
    "offset+300": ("offset", 300.0),
}
SAW_DROP = 30.0      # log2 units the sawtooth falls at every fourth tile
SCALES = {"scale0.02": f32(0.02), "scale0.3": f32(0.3)}


def _seed(name: str, shape) -> int:
    h = 1469598103934665603
    for ch in f"{name}{tuple(shape)}".encode():
        h = ((h ^ ch) * 1099511628211) % (1 << 62)
    return h


def build_inputs(name: str, B: int, S: int, Hq: int, Hkv: int, scale: float = DEFAULT_SCALE,
                 doc=None, device="cpu"):
    """bf16 q, k, v, dout of the family ``name`` (FAMILIES / DOC_FAMILIES),
    seeded by the name and the shape, generated on the CPU so that every
    device sees the same bits.  Distinct heads and batch rows get distinct
    data.  -> namespace(q, k, v, dout, target): ``target`` int64 [B, S] for
    the probes (the key row i aims at), else None."""
    kind, par = (DOC_FAMILIES if doc is not None and name in DOC_FAMILIES else FAMILIES)[name]
    g = torch.Generator().manual_seed(_seed(name, (B, S, Hq, Hkv)))
    G = Hq // Hkv

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    def unit():     # one direction per batch row and KV head, [B, 1, Hkv, D]
        u = rn(B, 1, Hkv, D)
        return u / u.norm(dim=-1, keepdim=True)

    def per_q_head(t):      # [B, S, Hkv, D] -> [B, S, Hq, D]
        return t.repeat_interleave(G, dim=2)

    target = None
    v = rn(B, S, Hkv, D)
    dout = rn(B, S, Hq, D)
    if kind == "random":
        k = rn(B, S, Hkv, D)
        q = rn(B, S, Hq, D) * torch.exp2(torch.arange(Hq) % 3).view(1, 1, Hq, 1)
    elif kind in ("probe", "probe_doc"):
        k = rn(B, S, Hkv, D).bfloat16().float()
        i = torch.arange(S)
        if kind == "probe":
            target = ((i + par) % S).expand(B, S)
        else:
            target = (doc.doc_start.cpu().long() + par) % S
        aimed = torch.gather(k, 1, target[:, :, None, None].expand(B, S, Hkv, D))
        # 2 k_target, plus what tells the heads of one group apart
        q = 2 * per_q_head(aimed) + 0.25 * rn(B, S, Hq, D)
    elif kind in ("ramp", "sawtooth"):
        u = unit()
        per_tile = par / (8 * scale * LOG2E)        # g per 64 keys: `par` log2 units of 8 g
        j = torch.arange(S, dtype=torch.float32)
        gj = per_tile * j / TILE
        if kind == "sawtooth":
            gj = gj - SAW_DROP / (8 * scale * LOG2E) * torch.floor(j / (4 * TILE))
        k = gj.view(1, S, 1, 1) * u + 0.05 * rn(B, S, Hkv, D)
        q = 8 * per_q_head(u.expand(B, S, Hkv, D)) + 0.05 * rn(B, S, Hq, D)
    elif kind == "offset":
        u = unit()
        k = (par / (8 * scale)) * u + 0.5 * rn(B, S, Hkv, D)
        q = 8 * per_q_head(u.expand(B, S, Hkv, D)) + 0.5 * rn(B, S, Hq, D)
    else:
        raise KeyError(name)
    out = types.SimpleNamespace(q=q, k=k, v=v, dout=dout)
    for n in ("q", "k", "v", "dout"):
        setattr(out, n, getattr(out, n).bfloat16().to(device))
    out.target = None if target is None else target.to(device)
    return out


# --------------------------------- conditions the inputs must meet (fp64) ---
def tile_increments(q, k, scale, causal, doc=None):
    """Per query row, the maximum over each 64-key tile's visible keys of
    ``scale log2(e) s`` and its change from tile to tile.
    -> (inc [B,Hq,S,T-1], both [..] bool: both tiles have a visible key,
        whole [..] bool: the later tile's last key is visible)."""
    B, S, Hq, _ = q.shape
    G = Hq // k.shape[2]
    vis = visible(S, causal, doc, q.device)
    s = _heads(q) @ _heads(k, G).transpose(-1, -2) * (scale * LOG2E)
    s = s.masked_fill(~vis, float("-inf"))
    tmax = s.view(B, Hq, S, S // TILE, TILE).amax(-1)
    both = torch.isfinite(tmax[..., 1:]) & torch.isfinite(tmax[..., :-1])
    inc = torch.where(both, tmax[..., 1:] - tmax[..., :-1], tmax.new_zeros(()))
    whole = vis[..., TILE - 1::TILE][..., 1:].expand_as(both)
    return inc, both, whole


def check_conditions(name, inp, scale, causal, doc=None, lse=None):
    """Raise AssertionError unless the inputs of family ``name`` drive the
    regime they are for, judged on the fp64 reference alone.

    * probe: the target key holds >= 0.9 of every row that sees it; where the
      mask hides it, it would hold >= 0.9 of the row if it were visible.
    * ramp: between tiles whose last key the row sees, every increment of the
      tile maximum lies in (0, 8) for slope 7.5, (8, 16) for 8.5, above 30 for
      40, below 0 for the negative slopes.  The tile a causal row sees only
      the head of (its diagonal tile) climbs by part of the slope, from one
      key's share of it (which the 0.05 noise can outweigh) up to all of it:
      there the increment only has to stay under the upper end.
    * sawtooth: (0, 8) except into every fourth tile, where it falls.
    * offset: min |lse| > 200 (``lse``: the reference's)."""
    families = DOC_FAMILIES if doc is not None and name in DOC_FAMILIES else FAMILIES
    kind, par = families.get(name, ("random", None))
    if kind in ("probe", "probe_doc"):
        B, S, Hq, _ = inp.q.shape
        G = Hq // inp.k.shape[2]
        vis = visible(S, causal, doc, inp.q.device)
        s = _heads(inp.q) @ _heads(inp.k, G).transpose(-1, -2) * scale
        t = inp.target[:, None, :, None].expand(B, Hq, S, 1)
        st = s.gather(-1, t)[..., 0]
        seen = vis.expand(B, Hq, S, S).gather(-1, t)[..., 0]
        rest = torch.logsumexp(s.masked_fill(~vis, float("-inf")), dim=-1)
        total = torch.where(seen, rest, torch.logaddexp(rest, st))
        w = torch.exp(st - total)
        assert w.min().item() >= 0.9, f"{name}: the target holds only {w.min().item():.3f} of a row"
        if kind == "probe" and par == 1 and causal:
            assert int((~seen).sum()) == B * Hq * (S - 1)
    elif kind in ("ramp", "sawtooth"):
        inc, both, whole = tile_increments(inp.q, inp.k, scale, causal, doc)
        lo, hi = {7.5: (0.0, 8.0), 8.5: (8.0, 16.0), 40.0: (30.0, math.inf),
                  -7.5: (-math.inf, 0.0), -40.0: (-math.inf, 0.0)}[par]
        full = both & whole
        part = both & ~whole
        rising = torch.ones_like(both)
        if kind == "sawtooth":
            T = inc.shape[-1] + 1
            falls = (torch.arange(1, T, device=inc.device) % 4 == 0).expand_as(both)
            rising = ~falls
            bad = both & falls & ~(inc < 0)
            assert not bool(bad.any()), f"{name}: no fall into a fourth tile"
        assert bool((full & rising).any()), f"{name}: no row sees two whole tiles"
        sel = inc[full & rising]
        assert sel.min().item() > lo and sel.max().item() < hi, \
            f"{name}: increments {sel.min().item():.3f} .. {sel.max().item():.3f} outside ({lo}, {hi})"
        if bool((part & rising).any()):
            sel = inc[part & rising]
            assert sel.max().item() < hi, \
                f"{name}: part-tile increments {sel.min().item():.3f} .. {sel.max().item():.3f}"
    elif kind == "offset":
        assert lse.abs().min().item() > 200, f"{name}: min |lse| = {lse.abs().min().item():.1f}"
