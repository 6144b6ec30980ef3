"""Elementwise fp64 checks of the flash-attention kernels
(``native/kernels/attention_fwd.hip``, ``attention_fwd256.hip``,
``attention_bwd.hip``, ``attention_bwd256.hip``, ``attention_dq256.hip``) on
inputs that drive the mask edges, the lazy rescale, ``scale`` and large
``|lse|``: the reference, the per-element bounds and the input families are
``tests/attention_refs.py`` (read its docstring first);
``tests/test_attention_refs_cpu.py`` shows on a CPU model that a correct
forward stays inside the bounds and that a leaked key, a dropped diagonal, a
missing maximum subtraction, a skipped rescale, a stale-maximum ``lse`` and an
ignored ``scale`` each break them by more than ten times.

How the kernels are called:

* through ``mxk8s.ops._lib`` (``mxk_attn_fwd_variant``, ``mxk_attn_bwd_variant``,
  ``mxk_attn_fwd_doc``, ``mxk_attn_bwd_doc``), so every buffer is the test's;
* ``o``, ``lse``, ``dq``, ``dk``, ``dv`` and the backward workspace start as NaN
  bit patterns no kernel produces (an element no workgroup writes fails its
  bound) and are 64 elements longer than needed; the tail must keep its bits;
* the backward's ``o`` and ``lse`` are the fp64 reference rounded to bf16 /
  fp32, not the forward kernel's output: a backward failure never depends on
  the forward;
* the conditions of each family (``check_conditions``) are asserted on the
  fp64 reference before a kernel result is looked at;
* a test case is one (shape, family, mask) with the reference computed once;
  the variants run inside it, each check prints ``RATIO <case>:v<variant>:<output>
  <largest error / bound>``, and the case fails, after every variant ran,
  with the (b, row, head, column) - (b, head, row) for ``lse`` - of the worst
  element of each output over its bound.  A forward variant the library was
  not built with (``mxk_attn_fwd_variant_built``: 5-9 are A/B records of the
  experiments library) is left out, as ``test_gpu_attention.py`` skips it.

Backward variant 8 adds dQ with packed-bf16 atomics, so its dQ is summed in
bf16 and cannot meet a bound that assumes an fp32 accumulator: its ``dk`` and
``dv`` are under the bound here and its ``dq`` stays with
``test_attn_bwd_onepass_v7_v8``.

Shapes (B, S, Hq, Hkv), the smallest that reach every tile path
(``test_shapes_resolve_as_the_table_says`` asserts the degradations through
``mxk_attn_bwd_plan``):

    (1, 128, 2, 2)    one query block; backward 9 -> 5
    (1, 640, 4, 2)    five query blocks, ten key tiles, S % 256 != 0: backward
                      9 -> 5, forward 10 runs as 4
    (2, 768, 6, 2)    group of 3: 9 -> 6; three 256-key blocks, batch stride,
                      q / k / v views of one fused buffer
    (1, 1024, 8, 1)   MQA, two quads, every K / V ring slot reused
    (1, 512, 12, 1)   three quads

Forward: every built variant on (1, 640, 4, 2) and (1, 1024, 8, 1), 4 and 10
on the others; backward: 0-9 on (1, 640, 4, 2), (2, 768, 6, 2) and
(1, 1024, 8, 1), the default 9 on the others; all 13 families, causal and
full.  Nothing of the crossing was thinned.

The whole file takes about 10 s on an MI355X.  Largest error / bound of the
recorded run (``profiles/attention_numerics/ratios.txt``, every RATIO line of
it), per output, with the case that produced it; no kernel change was needed:

    o     0.834   random, causal, (2, 768, 6, 2), forward 4
    lse   0.0367  probe-1, full, (1, 512, 12, 1), forward 4
    dq    0.877   ramp-7.5, causal, (1, 640, 4, 2), backward 0
    dk    0.844   probe+1, causal, (1, 128, 2, 2), backward 9 (runs as 5)
    dv    0.809   ramp7.5, causal, (1, 128, 2, 2), backward 9 (runs as 5)
"""
import pytest
import torch

import attention_refs as AR
from mxk8s.ops import _lib
from mxk8s.ops.attention import DocMask

pytestmark = pytest.mark.gpu

D = AR.D
PAD = 64
SHAPES = [(1, 128, 2, 2), (1, 640, 4, 2), (2, 768, 6, 2), (1, 1024, 8, 1), (1, 512, 12, 1)]
WIDE = {(1, 640, 4, 2), (1, 1024, 8, 1)}                      # every forward variant
WIDE_BWD = {(1, 640, 4, 2), (2, 768, 6, 2), (1, 1024, 8, 1)}    # every backward variant
FUSED = {(2, 768, 6, 2)}                                      # q / k / v views of one buffer
RESOLVES_TO = {(1, 128, 2, 2): 5, (1, 640, 4, 2): 5, (2, 768, 6, 2): 6, (1, 1024, 8, 1): 9,
               (1, 512, 12, 1): 9}
DOC_SHAPE = (2, 768, 6, 2)
DOC_LENGTHS = [[1, 63, 64, 65, 127, 448], [768]]
FWD_ALL = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10)
BWD_ALL = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)


# ---- helpers ----------------------------------------------------------------
def _poison(n, dtype, dev):
    """``_poison`` of test_gpu_fused_numerics.py, flat and PAD elements longer."""
    if dtype == torch.bfloat16:
        return torch.full((n + PAD,), 0x7FC1, dtype=torch.int16, device=dev).view(torch.bfloat16)
    return torch.full((n + PAD,), 0x7FC12345, dtype=torch.int32, device=dev).view(torch.float32)


def _tail_kept(flat, n):
    bits = flat[n:].view(torch.int16 if flat.element_size() == 2 else torch.int32)
    want = 0x7FC1 if flat.element_size() == 2 else 0x7FC12345
    return bool((bits == want).all())


def _place(inp, shape, dev):
    """The inputs on the device; for the FUSED shapes q / k / v become views of
    one [B, S, (Hq + 2 Hkv) D] buffer (token stride, the Llama layout)."""
    B, S, Hq, Hkv = shape
    q, k, v = inp.q.to(dev), inp.k.to(dev), inp.v.to(dev)
    if shape in FUSED:
        qkv = torch.cat([q.reshape(B, S, -1), k.reshape(B, S, -1), v.reshape(B, S, -1)], dim=-1)
        q = qkv[..., :Hq * D].view(B, S, Hq, D)
        k = qkv[..., Hq * D:(Hq + Hkv) * D].view(B, S, Hkv, D)
        v = qkv[..., (Hq + Hkv) * D:].view(B, S, Hkv, D)
        assert not q.is_contiguous() and q.stride(1) == (Hq + 2 * Hkv) * D
    return q, k, v, inp.dout.to(dev).contiguous()


class _Case:
    """Inputs, fp64 reference and bounds of one (shape, family, scale, mask)."""

    def __init__(self, shape, name, scale, causal, dev, doc_lengths=None, backward=False):
        B, S, Hq, Hkv = shape
        self.shape, self.scale, self.causal, self.dev = shape, AR.f32(scale), causal, dev
        self.doc = DocMask.from_lengths(doc_lengths, S) if doc_lengths else None
        family = "random" if name in AR.SCALES else name
        inp = AR.build_inputs(family, B, S, Hq, Hkv, scale=self.scale, doc=self.doc)
        if inp.target is not None:
            inp.target = inp.target.to(dev)
        self.q, self.k, self.v, self.dout = _place(inp, shape, dev)
        inp.q, inp.k = self.q, self.k
        if self.doc is not None:
            self.doc = self.doc.to(dev)
        mask = "doc" if self.doc is not None else "causal" if causal else "full"
        self.id = f"{B}x{S}x{Hq}x{Hkv}:{name}:{mask}"
        self.o, self.lse, mag_o, smag = AR.attn_fwd_ref(self.q, self.k, self.v, self.scale, causal,
                                                        self.doc)
        AR.check_conditions(family, inp, self.scale, causal, self.doc, lse=self.lse)
        self.b_o = AR.bound_o(self.o, mag_o, smag)
        self.b_lse = AR.bound_lse(self.lse, smag)
        if backward:
            self.o_in = self.o.bfloat16()
            self.lse_in = self.lse.float()
            self.r = AR.attn_bwd_ref(self.q, self.k, self.v, self.o_in, self.lse_in, self.dout,
                                     self.scale, causal, self.doc)
            self.b_dq, self.b_dk, self.b_dv = AR.bound_dq(self.r), AR.bound_dk(self.r), AR.bound_dv(self.r)
        self.failures = []

    def check(self, variant, output, got, ref, bound):
        ratio, at = AR.worst(got, ref, bound)
        print(f"RATIO {self.id}:v{variant}:{output} {ratio:.3g}")
        if not ratio <= 1:
            where = "(b, head, row)" if output == "lse" else "(b, row, head, column)"
            self.failures.append(f"{self.id} variant {variant} {output}: largest error / bound = "
                                 f"{ratio:.3g} at {where} {at}")

    def require(self, ok, what):
        if not ok:
            self.failures.append(f"{self.id} {what}")

    def forward(self, variant):
        """``variant`` None: the document-mask kernel."""
        B, S, Hq, Hkv = self.shape
        L = _lib.lib()
        n_o, n_l = B * S * Hq * D, B * Hq * S
        o, lse = _poison(n_o, torch.bfloat16, self.dev), _poison(n_l, torch.float32, self.dev)
        q, k, v = self.q, self.k, self.v
        if variant is None:
            st = L.mxk_attn_fwd_doc(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                                    lse.data_ptr(), self.doc.doc_start.data_ptr(), B, S, Hq, Hkv, D,
                                    q.stride(1), k.stride(1), v.stride(1), self.scale,
                                    _lib.stream_ptr(self.dev))
            variant = "doc"
        else:
            st = L.mxk_attn_fwd_variant(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                                        lse.data_ptr(), B, S, Hq, Hkv, D, q.stride(1), k.stride(1),
                                        v.stride(1), self.scale, int(self.causal), variant,
                                        _lib.stream_ptr(self.dev))
        assert st == 0, (self.id, variant, st)
        torch.cuda.synchronize()
        self.check(variant, "o", o[:n_o].view(B, S, Hq, D), self.o, self.b_o)
        self.check(variant, "lse", lse[:n_l].view(B, Hq, S), self.lse, self.b_lse)
        self.require(_tail_kept(o, n_o) and _tail_kept(lse, n_l),
                     f"variant {variant}: wrote past the end of o or lse")

    def backward(self, variant):
        """``variant`` None: the document-mask kernels."""
        B, S, Hq, Hkv = self.shape
        L = _lib.lib()
        n_q, n_k = B * S * Hq * D, B * S * Hkv * D
        if variant is None:
            n_ws = L.mxk_attn_bwd_doc_workspace(B, S, Hq) // 4
        else:
            n_ws = L.mxk_attn_bwd_workspace_variant(B, S, Hq, variant) // 4
        dq, dk, dv = (_poison(n, torch.bfloat16, self.dev) for n in (n_q, n_k, n_k))
        ws = _poison(n_ws, torch.float32, self.dev)
        q, k, v = self.q, self.k, self.v
        head = (q.data_ptr(), k.data_ptr(), v.data_ptr(), self.o_in.data_ptr(), self.dout.data_ptr(),
                self.lse_in.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ws.data_ptr())
        dims = (B, S, Hq, Hkv, D, q.stride(1), k.stride(1), v.stride(1), Hkv * D, Hkv * D, self.scale)
        if variant is None:
            st = L.mxk_attn_bwd_doc(*head, self.doc.doc_start.data_ptr(), self.doc.doc_end.data_ptr(),
                                    *dims, _lib.stream_ptr(self.dev))
            variant = "doc"
        else:
            st = L.mxk_attn_bwd_variant(*head, *dims, int(self.causal), variant,
                                        _lib.stream_ptr(self.dev))
        assert st == 0, (self.id, variant, st)
        torch.cuda.synchronize()
        if variant != 8:        # dQ summed in bf16 by atomics: see the module docstring
            self.check(variant, "dq", dq[:n_q].view(B, S, Hq, D), self.r.dq, self.b_dq)
        self.check(variant, "dk", dk[:n_k].view(B, S, Hkv, D), self.r.dk, self.b_dk)
        self.check(variant, "dv", dv[:n_k].view(B, S, Hkv, D), self.r.dv, self.b_dv)
        self.require(_tail_kept(dq, n_q) and _tail_kept(dk, n_k) and _tail_kept(dv, n_k)
                     and _tail_kept(ws, n_ws),
                     f"variant {variant}: wrote past the end of dq, dk, dv or the workspace")

    def done(self):
        assert not self.failures, "\n".join(self.failures)


def _fwd_variants(shape, wanted=None):
    L = _lib.lib()
    wanted = wanted or (FWD_ALL if shape in WIDE else (4, 10))
    return [v for v in wanted if L.mxk_attn_fwd_variant_built(v)]


def _sid(shape):
    return "x".join(str(n) for n in shape)


def _mask(causal):
    return "causal" if causal else "full"


# ---- the table of shapes keeps meaning what it says ---------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_shapes_resolve_as_the_table_says(cuda_device, shape):
    import ctypes
    B, S, Hq, Hkv = shape
    tok = (Hq + 2 * Hkv) * D if shape in FUSED else None
    for causal in (0, 1):
        out = (ctypes.c_long * 7)(*([-7] * 7))
        st = _lib.lib().mxk_attn_bwd_plan(B, S, Hq, Hkv, tok or Hq * D, tok or Hkv * D,
                                          tok or Hkv * D, Hkv * D, Hkv * D, causal, 9, out)
        assert st == 0 and out[0] == RESOLVES_TO[shape], (shape, causal, st, out[0])
    # forward variant 10 takes whole 256-row blocks only (attn_fwd256_ok); else it runs 4
    assert (S % 256 != 0) == (shape in {(1, 128, 2, 2), (1, 640, 4, 2)})


# ---- forward ----------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False], ids=_mask)
@pytest.mark.parametrize("name", list(AR.FAMILIES))
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_attn_fwd_elementwise(cuda_device, shape, name, causal):
    case = _Case(shape, name, AR.DEFAULT_SCALE, causal, cuda_device)
    for variant in _fwd_variants(shape):
        case.forward(variant)
    case.done()


# ---- backward ---------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False], ids=_mask)
@pytest.mark.parametrize("name", list(AR.FAMILIES))
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_attn_bwd_elementwise(cuda_device, shape, name, causal):
    case = _Case(shape, name, AR.DEFAULT_SCALE, causal, cuda_device, backward=True)
    for variant in (BWD_ALL if shape in WIDE_BWD else (9,)):
        case.backward(variant)
    case.done()


# ---- document mask ----------------------------------------------------------
@pytest.mark.parametrize("name", list(AR.DOC_FAMILIES))
def test_attn_doc_elementwise(cuda_device, name):
    """``mxk_attn_fwd_doc`` / ``mxk_attn_bwd_doc``: documents that end on, one
    before and one after a tile edge next to a row that is one document.  The
    probes aim at the last key of the previous document (hidden) and the first
    of the row's own (the earliest it may see); ``ramp8.5`` restarts its climb
    inside each document through the mask alone."""
    case = _Case(DOC_SHAPE, name, AR.DEFAULT_SCALE, True, cuda_device, doc_lengths=DOC_LENGTHS,
                 backward=True)
    case.forward(None)
    case.backward(None)
    case.done()


# ---- scale ------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False], ids=_mask)
@pytest.mark.parametrize("name", list(AR.SCALES))
@pytest.mark.parametrize("shape", sorted(WIDE), ids=_sid)
def test_attn_scale_elementwise(cuda_device, shape, name, causal):
    """``scale`` 0.02 and 0.3 on ``random``: the forward's log2-domain factor,
    ``lse`` as the natural log of the scaled scores, the backward's -lse / scale
    accumulator preload and its final multiply."""
    case = _Case(shape, name, AR.SCALES[name], causal, cuda_device, backward=True)
    for variant in _fwd_variants(shape, (4, 10)):
        case.forward(variant)
    for variant in (5, 6, 9):
        case.backward(variant)
    case.done()
