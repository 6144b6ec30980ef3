"""The fp64 attention reference, its bounds and its input families
(``tests/attention_refs.py``) on the CPU, before any kernel is judged by them.

1. ``attn_fwd_ref`` / ``attn_bwd_ref`` against ``torch.autograd`` on
   ``attention_ref`` in float64 (GQA, a ``DocMask``, a non-default scale).
2. ``model_fwd``: a torch model of the forward kernel's arithmetic
   (``attention_fwd.hip``): 64-key tiles, fp32 scores, the online softmax in the
   log2 domain with the lazy rescale (the row maximum moves only when it grew
   by more than 8; switchable), ``l`` summed from the unrounded P, P rounded to
   bf16 into an fp32 accumulator, bf16 output, ``lse = m scale + ln l``.  It
   stays inside the ``o`` and ``lse`` bounds on every family with every
   condition of ``check_conditions`` holding: the record that the reference
   and the bounds agree with a correct implementation.
3. Mutants of that model, each a bug a flash-attention kernel can have, must
   break a bound by a ratio above 10 on the family named in ``CAUGHT_BY``.
   That is what shows the GPU tests would fail on a subtly wrong kernel
   without ever running a wrong kernel on a GPU.
"""
import math

import pytest
import torch

import attention_refs as AR
from mxk8s.ops.attention import DocMask, attention_ref

SHAPE = (1, 512, 4, 2)                       # B, S, Hq, Hkv
DOC_LENGTHS = [[1, 63, 64, 65, 127, 192]]    # boundaries on, before and after a tile edge


# ---- 1. against autograd ------------------------------------------------------
@pytest.mark.parametrize("B,S,Hq,Hkv,causal,doc_lengths,scale", [
    (2, 128, 6, 2, True, None, None),
    (1, 192, 4, 1, False, None, 0.3),
    (2, 128, 4, 2, True, [[1, 63, 64], [128]], None),
    (1, 64, 3, 3, True, None, 0.02),
])
def test_refs_match_autograd_fp64(B, S, Hq, Hkv, causal, doc_lengths, scale):
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(B, S, h, AR.D, generator=g, dtype=torch.float64).requires_grad_()
               for h in (Hq, Hkv, Hkv))
    dout = torch.randn(B, S, Hq, AR.D, generator=g, dtype=torch.float64)
    doc = DocMask.from_lengths(doc_lengths, S) if doc_lengths else None
    sc = scale if scale is not None else 1.0 / math.sqrt(AR.D)
    want = attention_ref(q, k, v, causal=causal, scale=scale, doc=doc)
    assert want.dtype == torch.float64
    want.backward(dout)

    o, lse, mag_o, smag = AR.attn_fwd_ref(q.detach(), k.detach(), v.detach(), sc, causal, doc)
    assert o.dtype == torch.float64 and o.shape == (B, S, Hq, AR.D) and lse.shape == (B, Hq, S)
    assert (o - want.detach()).abs().max().item() <= 1e-12 * want.detach().abs().max().item()
    s = torch.einsum("bihd,bjhd->bhij", q.detach(), k.detach().repeat_interleave(Hq // Hkv, 2)) * sc
    s = s.masked_fill(~AR.visible(S, causal, doc, "cpu"), float("-inf"))
    assert torch.allclose(lse, torch.logsumexp(s, -1), rtol=1e-13, atol=1e-13)
    assert bool((mag_o >= o.abs() * (1 - 1e-12)).all())
    assert bool((smag >= lse.abs()).all()) and bool((smag >= s.amax(-1) * (1 - 1e-12)).all())

    r = AR.attn_bwd_ref(q.detach(), k.detach(), v.detach(), o, lse, dout, sc, causal, doc)
    for name, got, grad, mag in (("dq", r.dq, q.grad, r.mag_dq), ("dk", r.dk, k.grad, r.mag_dk),
                                 ("dv", r.dv, v.grad, r.mag_dv)):
        assert got.shape == grad.shape, name
        assert (got - grad).abs().max().item() <= 1e-11 * grad.abs().max().item(), name
        assert bool((mag >= got.abs() * (1 - 1e-12)).all()), name
    # dP - delta cancels inside dS: the cancellation magnitudes dominate the plain ones
    assert bool((r.magc_dq >= r.mag_dq * (1 - 1e-12)).all())
    assert bool((r.magc_dk >= r.mag_dk * (1 - 1e-12)).all())
    # a key's eps is the largest of the rows that see it
    vis = AR.visible(S, causal, doc, "cpu").expand(B, Hq, S, S)
    for b, hk, j in ((0, 0, 0), (B - 1, Hkv - 1, S - 1), (0, Hkv - 1, S // 2)):
        G = Hq // Hkv
        rows = torch.stack([torch.where(vis[b, hk * G + x, :, j], r.eps_q[b, hk * G + x],
                                        torch.zeros(())) for x in range(G)])
        assert r.eps_k[b, hk, j].item() == rows.max().item()


# ---- 2. a model of the forward kernel's arithmetic ------------------------------
MUTANTS = ("leak", "no_diagonal", "no_max", "skip_rescale", "fresh_lse", "default_scale")


def model_fwd(q, k, v, scale, causal, doc=None, lazy=True, mutant=None):
    """-> (o bf16 [B,S,Hq,D], lse fp32 [B,Hq,S]) on the CPU, in the arithmetic of
    ``mxk_attn_fwd_dma_kernel`` (``lazy``: its PIPE forms, variants 3 / 4 / 10).

    Mutants: ``leak`` key i + 1 visible to the rows i % 64 == 63; ``no_diagonal``
    key i hidden from row i > 0; ``no_max`` P = exp2(c s) with no shift;
    ``skip_rescale`` the maximum moves but l and the accumulator keep their old
    reference point; ``fresh_lse`` lse from the true running maximum while l
    belongs to the stale one; ``default_scale`` 1 / sqrt(D) whatever was passed."""
    assert mutant is None or mutant in MUTANTS
    B, S, Hq, _ = q.shape
    G = Hq // k.shape[2]
    q, k, v = q.cpu(), k.cpu(), v.cpu()
    qf = q.float().transpose(1, 2)
    kf = k.float().transpose(1, 2).repeat_interleave(G, dim=1)
    vf = v.float().transpose(1, 2).repeat_interleave(G, dim=1)
    vis = AR.visible(S, causal, doc, "cpu").expand(B, 1, S, S).clone()
    i = torch.arange(S)
    if mutant == "leak" and causal:
        edge = i[(i % AR.TILE == AR.TILE - 1) & (i + 1 < S)]
        vis[:, :, edge, edge + 1] = True
    if mutant == "no_diagonal" and causal:
        vis[:, :, i[1:], i[1:]] = False
    if mutant == "default_scale":
        scale = AR.DEFAULT_SCALE
    scale = torch.tensor(scale, dtype=torch.float32)
    c = scale * torch.tensor(AR.LOG2E, dtype=torch.float32)
    ninf = torch.tensor(float("-inf"))
    # the DOC kernels start from a finite floor (a row may meet a fully masked tile first)
    m = torch.full((B, Hq, S), -1.7e38 / max(1.0, c.item()) if doc is not None else float("-inf"))
    fresh = m.clone()
    l = torch.zeros(B, Hq, S)
    acc = torch.zeros(B, Hq, S, AR.D)
    for kv0 in range(0, S, AR.TILE):
        s = qf @ kf[:, :, kv0:kv0 + AR.TILE].transpose(-1, -2)
        s = torch.where(vis[..., kv0:kv0 + AR.TILE], s, ninf)
        mx = s.amax(-1)
        fresh = torch.maximum(fresh, mx)
        m_new = torch.maximum(m, mx)
        grow = (m_new - m) * c > 8.0 if lazy else torch.ones_like(m, dtype=torch.bool)
        m_new = torch.where(grow, m_new, m)
        alpha = torch.where(grow, torch.exp2((m - m_new) * c), torch.ones(()))
        if mutant == "skip_rescale":
            alpha = torch.where(torch.isfinite(alpha) & (alpha > 0), torch.ones(()), alpha)
        if mutant == "no_max":
            p = torch.exp2(s * c)
            m_new, alpha = torch.zeros_like(m), torch.ones_like(m)
        else:
            p = torch.exp2(s * c + (-m_new * c)[..., None])
        l = l * alpha + p.sum(-1)
        acc = acc * alpha[..., None] + p.bfloat16().float() @ vf[:, :, kv0:kv0 + AR.TILE]
        m = m_new
    o = (acc * (1.0 / l)[..., None]).bfloat16().transpose(1, 2).contiguous()
    lse = (fresh if mutant == "fresh_lse" else m) * scale + torch.log(l)
    return o, lse


def _doc():
    return DocMask.from_lengths(DOC_LENGTHS, SHAPE[1])


def _cases():
    for name in AR.FAMILIES:
        for causal in (True, False):
            yield name, AR.DEFAULT_SCALE, causal, False
    for name, sc in AR.SCALES.items():
        for causal in (True, False):
            yield name, sc, causal, False
    for name in AR.DOC_FAMILIES:
        yield name, AR.DEFAULT_SCALE, True, True


_cache = {}


def _reference(name, scale, causal, with_doc):
    """Inputs and fp64 reference of a case, conditions checked; computed once."""
    key = (name, scale, causal, with_doc)
    if key not in _cache:
        doc = _doc() if with_doc else None
        family = "random" if name in AR.SCALES else name
        inp = AR.build_inputs(family, *SHAPE, scale=scale, doc=doc)
        o, lse, mag_o, smag = AR.attn_fwd_ref(inp.q, inp.k, inp.v, scale, causal, doc)
        AR.check_conditions(family, inp, scale, causal, doc, lse=lse)
        _cache[key] = (inp, doc, o, lse, AR.bound_o(o, mag_o, smag), AR.bound_lse(lse, smag))
    return _cache[key]


def _ratios(name, scale, causal, with_doc, **model):
    inp, doc, o, lse, b_o, b_lse = _reference(name, scale, causal, with_doc)
    got_o, got_lse = model_fwd(inp.q, inp.k, inp.v, scale, causal, doc, **model)
    return AR.worst(got_o, o, b_o), AR.worst(got_lse, lse, b_lse)


def _id(case):
    name, _, causal, with_doc = case
    return f"{name}-{'doc' if with_doc else 'causal' if causal else 'full'}"


@pytest.mark.parametrize("lazy", [True, False], ids=["lazy", "eager"])
@pytest.mark.parametrize("case", list(_cases()), ids=_id)
def test_model_of_the_forward_is_within_the_bounds(case, lazy):
    (ro, at_o), (rl, at_l) = _ratios(*case, lazy=lazy)
    print(f"RATIO model {_id(case)} o {ro:.3g} lse {rl:.3g}")
    assert ro <= 1, f"o: largest error / bound = {ro:.3g} at (b, row, head, column) {at_o}"
    assert rl <= 1, f"lse: largest error / bound = {rl:.3g} at (b, head, row) {at_l}"


def test_builders_are_seeded_and_tell_heads_apart():
    a = AR.build_inputs("probe-1", *SHAPE)
    b = AR.build_inputs("probe-1", *SHAPE)
    for n in ("q", "k", "v", "dout"):
        t = getattr(a, n)
        assert t.dtype == torch.bfloat16 and torch.equal(t, getattr(b, n))
        assert not torch.equal(t[:, :, 0], t[:, :, 1]), n
    two = AR.build_inputs("ramp8.5", 2, 128, 2, 1)
    assert not torch.equal(two.q[0], two.q[1]) and not torch.equal(two.k[0], two.k[1])


def test_a_builder_that_leaves_its_regime_fails_the_conditions():
    doc = None
    inp = AR.build_inputs("random", *SHAPE)
    inp.target = torch.arange(SHAPE[1]).expand(1, -1)
    _, lse, _, _ = AR.attn_fwd_ref(inp.q, inp.k, inp.v, AR.DEFAULT_SCALE, True, doc)
    for name in ("probe0", "ramp7.5", "ramp8.5", "ramp40", "ramp-7.5", "sawtooth", "offset+300"):
        with pytest.raises(AssertionError):
            AR.check_conditions(name, inp, AR.DEFAULT_SCALE, True, doc, lse=lse)
    ramp = AR.build_inputs("ramp7.5", *SHAPE)
    with pytest.raises(AssertionError):
        AR.check_conditions("ramp8.5", ramp, AR.DEFAULT_SCALE, False)


# ---- 3. mutants ---------------------------------------------------------------
# mutant -> (family that catches it, scale, causal, which output breaks)
CAUGHT_BY = {
    "leak": ("probe+1", AR.DEFAULT_SCALE, True, "o"),
    "no_diagonal": ("probe0", AR.DEFAULT_SCALE, True, "o"),
    "no_max": ("offset+300", AR.DEFAULT_SCALE, False, "o"),
    "skip_rescale": ("ramp8.5", AR.DEFAULT_SCALE, True, "o"),
    "fresh_lse": ("ramp7.5", AR.DEFAULT_SCALE, False, "lse"),
    "default_scale": ("scale0.3", AR.SCALES["scale0.3"], True, "o"),
}


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutant_is_caught(mutant):
    name, scale, causal, output = CAUGHT_BY[mutant]
    (ro, _), (rl, _) = _ratios(name, scale, causal, False, mutant=mutant)
    print(f"RATIO mutant {mutant} on {name} o {ro:.3g} lse {rl:.3g}")
    assert (ro if output == "o" else rl) > 10, (mutant, name, ro, rl)


def test_more_than_one_family_catches_each_mask_and_rescale_mutant():
    """Beyond the one family CAUGHT_BY names: the other regimes that must see it."""
    also = {
        "leak": [("ramp40", AR.DEFAULT_SCALE, True), ("ramp7.5", AR.DEFAULT_SCALE, True)],
        "no_diagonal": [("ramp40", AR.DEFAULT_SCALE, True), ("offset+300", AR.DEFAULT_SCALE, True)],
        "no_max": [("offset-300", AR.DEFAULT_SCALE, True), ("ramp40", AR.DEFAULT_SCALE, False)],
        "skip_rescale": [("ramp40", AR.DEFAULT_SCALE, False), ("sawtooth", AR.DEFAULT_SCALE, False)],
        "fresh_lse": [("sawtooth", AR.DEFAULT_SCALE, True)],
        "default_scale": [("scale0.02", AR.SCALES["scale0.02"], False)],
    }
    for mutant, cases in also.items():
        for name, scale, causal in cases:
            (ro, _), (rl, _) = _ratios(name, scale, causal, False, mutant=mutant)
            print(f"RATIO mutant {mutant} on {name} o {ro:.3g} lse {rl:.3g}")
            assert max(ro, rl) > 10, (mutant, name, ro, rl)


def test_probe_sees_the_leak_far_better_than_random():
    """Why the families exist: on ``random`` every visible key weighs about
    1 / i, so a leaked key moves the output by a few bounds at S = 512 and by
    less as S grows; on ``probe+1`` it takes the row over, at any S."""
    (r_random, _), _ = _ratios("random", AR.DEFAULT_SCALE, True, False, mutant="leak")
    (r_probe, _), _ = _ratios("probe+1", AR.DEFAULT_SCALE, True, False, mutant="leak")
    print(f"RATIO leak random {r_random:.3g} probe+1 {r_probe:.3g}")
    assert r_probe > 20 * r_random
