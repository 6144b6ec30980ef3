"""Flash attention on the hand-written gfx950 kernels
(``native/kernels/attention_fwd.hip``, ``attention_bwd.hip`` and the
``attention_*256.hip`` kernels their dispatchers call).

``flash_attention(q, k, v, causal=True)`` takes q [B, S, Hq, 128] and k/v
[B, S, Hkv, 128] bf16 tensors whose last two dims are contiguous (token
strides are free, so q/k/v may be views of a fused QKV projection) and
returns o [B, S, Hq, 128] — the layout the output projection consumes, no
transposes.  GQA: Hq % Hkv == 0.  The forward also produces the per-row
log-sum-exp that the backward kernel uses to recompute P.

``attention_ref`` is the fp32 PyTorch reference the tests compare against
(float64 inputs stay float64).  The elementwise bounds of the kernels are
checked against the fp64 reference in ``tests/attention_refs.py``
(``attn_fwd_ref`` / ``attn_bwd_ref``, with the magnitude terms of the bounds
and the adversarial input families) by ``tests/test_gpu_attention_numerics.py``.
"""
from __future__ import annotations

import math
import os

import torch

from . import _lib

HEAD_DIM = 128
BLOCK_Q = 128


def supported(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> bool:
    """Shapes/layouts the HIP kernels handle (others use the reference path)."""
    if q.device.type != "cuda" or q.dtype != torch.bfloat16:
        return False
    B, S, Hq, D = q.shape
    if D != HEAD_DIM or S % BLOCK_Q or k.shape[2] == 0 or Hq % k.shape[2]:
        return False
    for t in (q, k, v):
        if t.stride(-1) != 1 or t.stride(-2) != D or t.stride(0) != S * t.stride(1) \
                or t.stride(1) % 8 or t.data_ptr() % 16:
            return False
    return True


class DocMask:
    """Document boundaries of packed rows: attention is causal within a
    document.  Query ``i`` of batch row ``b`` sees key ``j`` iff
    ``doc_start[b, i] <= j <= i``; ``doc_start[b, i]`` is the index of the
    first token of ``i``'s document and ``doc_end[b, j]`` (derived, never
    supplied) the exclusive end of ``j``'s.  Both are int32 ``[B, S]`` on one
    device and are not meant to be modified.  Built only through the
    constructors below, which produce valid tables: ``doc_start[b, 0] == 0``
    and ``doc_start[b, i]`` is ``doc_start[b, i - 1]`` or ``i``.  Positions
    are not reset at a boundary (RoPE is relative)."""

    __slots__ = ("doc_start", "doc_end")

    def __init__(self, doc_start: torch.Tensor, doc_end: torch.Tensor, _token=None):
        if _token is not DocMask:
            raise TypeError("build a DocMask with from_lengths / from_ids / from_eos / "
                            "from_doc_start")
        object.__setattr__(self, "doc_start", doc_start)
        object.__setattr__(self, "doc_end", doc_end)

    def __setattr__(self, name, value):
        raise AttributeError("DocMask is immutable")

    @classmethod
    def _from_first(cls, first: torch.Tensor) -> "DocMask":
        """``first`` bool [B, S]: token i opens a document (column 0 always does)."""
        first = first.clone()
        first[:, 0] = True
        B, S = first.shape
        idx = torch.arange(S, device=first.device).expand(B, S)
        start = torch.where(first, idx, idx.new_zeros(())).cummax(dim=1).values
        # the end of i's document: the next opening after i, or S
        nxt = torch.where(first, idx, idx.new_full((), S))
        nxt = torch.cat([nxt[:, 1:], nxt.new_full((B, 1), S)], dim=1)
        end = nxt.flip(1).cummin(dim=1).values.flip(1)
        return cls(start.to(torch.int32).contiguous(), end.to(torch.int32).contiguous(),
                   _token=cls)

    @classmethod
    def from_lengths(cls, lengths, S: int, device=None) -> "DocMask":
        """``lengths``: per batch row, the list of its document lengths (each >= 1, summing to S)."""
        first = torch.zeros((len(lengths), S), dtype=torch.bool)
        for b, row in enumerate(lengths):
            row = [int(n) for n in row]
            if not row or min(row) < 1 or sum(row) != S:
                raise ValueError(f"document lengths of row {b} must be >= 1 and sum to {S}: {row}")
            pos = 0
            for n in row:
                first[b, pos] = True
                pos += n
        m = cls._from_first(first)
        return m.to(device) if device is not None else m

    @classmethod
    def from_ids(cls, doc_ids: torch.Tensor) -> "DocMask":
        """``doc_ids`` integer [B, S]: a boundary is where the id changes."""
        if doc_ids.dim() != 2 or doc_ids.shape[1] < 1:
            raise ValueError(f"doc_ids must be [B, S], got {tuple(doc_ids.shape)}")
        first = torch.ones_like(doc_ids, dtype=torch.bool)
        first[:, 1:] = doc_ids[:, 1:] != doc_ids[:, :-1]
        return cls._from_first(first)

    @classmethod
    def from_eos(cls, tokens: torch.Tensor, eos_id: int) -> "DocMask":
        """A document ends after each ``eos_id`` of ``tokens`` [B, S]."""
        if tokens.dim() != 2 or tokens.shape[1] < 1:
            raise ValueError(f"tokens must be [B, S], got {tuple(tokens.shape)}")
        first = torch.ones_like(tokens, dtype=torch.bool)
        first[:, 1:] = tokens[:, :-1] == eos_id
        return cls._from_first(first)

    @classmethod
    def from_doc_start(cls, t: torch.Tensor, validate: bool = True) -> "DocMask":
        """From a ``doc_start`` table [B, S]; ``validate`` checks the validity
        rule on the host and raises ``ValueError``."""
        if t.dim() != 2 or t.shape[1] < 1 or t.is_floating_point():
            raise ValueError(f"doc_start must be an integer [B, S] tensor, got {tuple(t.shape)} "
                             f"{t.dtype}")
        idx = torch.arange(t.shape[1], device=t.device).expand_as(t)
        if validate:
            h = t.detach().cpu().long()
            hi = idx.cpu()
            if bool((h[:, 0] != 0).any()):
                raise ValueError("doc_start[b, 0] must be 0")
            ok = (h[:, 1:] == h[:, :-1]) | (h[:, 1:] == hi[:, 1:])
            if not bool(ok.all()):
                b, i = (~ok).nonzero()[0].tolist()
                raise ValueError(f"doc_start[{b}, {i + 1}] = {int(h[b, i + 1])} is neither "
                                 f"doc_start[{b}, {i}] = {int(h[b, i])} nor {i + 1}")
        return cls._from_first(t == idx)

    def to(self, device) -> "DocMask":
        return DocMask(self.doc_start.to(device), self.doc_end.to(device), _token=DocMask)

    @property
    def shape(self):
        return tuple(self.doc_start.shape)

    @property
    def device(self):
        return self.doc_start.device

    def bool_mask(self) -> torch.Tensor:
        """[B, S, S] bool, True where query i sees key j."""
        S = self.doc_start.shape[1]
        j = torch.arange(S, device=self.device)
        return (j[None, None, :] >= self.doc_start[:, :, None]) & (j[None, None, :] <= j[None, :, None])

    def visible_fraction(self) -> float:
        """Visible (query, key) pairs over the causal S (S + 1) / 2, averaged over the rows."""
        B, S = self.doc_start.shape
        i = torch.arange(S, device=self.device)
        pairs = (i[None, :] - self.doc_start.long() + 1).sum().item()
        return float(pairs) / (B * S * (S + 1) / 2)


def _check_doc(doc: DocMask, q: torch.Tensor, causal: bool) -> None:
    if not isinstance(doc, DocMask):
        raise TypeError(f"doc must be a DocMask, got {type(doc).__name__}")
    if not causal:
        raise ValueError("a document mask is causal within a document: causal=False with doc "
                         "is not supported")
    if doc.shape != tuple(q.shape[:2]):
        raise ValueError(f"doc tables are {doc.shape}, q is [B, S] = {tuple(q.shape[:2])}")
    if doc.device != q.device:
        raise ValueError(f"doc is on {doc.device}, q on {q.device}: move it with doc.to(device)")


def attention_ref(q, k, v, causal: bool = True, scale: float | None = None,
                  doc: DocMask | None = None) -> torch.Tensor:
    """fp32 reference (fp64 for float64 inputs): q [B,S,Hq,D], k/v [B,S,Hkv,D]
    -> [B,S,Hq,D] (q.dtype).  ``doc``: causal within a document (``DocMask``)."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    if doc is not None:
        _check_doc(doc, q, causal)
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    qf = q.to(ct).transpose(1, 2)
    kf = k.to(ct).transpose(1, 2).repeat_interleave(Hq // Hkv, dim=1)
    vf = v.to(ct).transpose(1, 2).repeat_interleave(Hq // Hkv, dim=1)
    s = qf @ kf.transpose(-1, -2) * scale
    if causal:
        mask = torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1)
        s = s.masked_fill(mask, float("-inf"))
    if doc is not None:
        s = s.masked_fill(~doc.bool_mask()[:, None], float("-inf"))
    o = torch.softmax(s, dim=-1) @ vf
    return o.transpose(1, 2).to(q.dtype)


def attn_fwd(q, k, v, causal: bool = True, scale: float | None = None, variant: int | None = None,
             doc: DocMask | None = None):
    """HIP forward: returns (o [B,S,Hq,D] bf16, lse [B,Hq,S] fp32).

    ``scale`` (default ``1 / sqrt(D)``) multiplies the raw scores
    ``s = q k^T``: ``o = softmax(scale s) v`` under the mask, and ``lse`` is
    the natural-log ``ln sum_j exp(scale s_ij)`` of the scaled scores over the
    visible keys - what ``attn_bwd`` takes back with the same ``scale``.

    ``doc`` (a ``DocMask``): causal within a document, on the DOC form of
    variant 4 (``mxk_attn_fwd_doc``); it cannot be combined with ``variant``.

    ``variant`` 4 (default): K/V by LDS-DMA, software-pipelined body (exp of
    one P chunk under the PV MFMAs of the previous one), lazy rescale (the
    row max is only moved when it grows by more than 2^8), loop unrolled by
    two so the LDS read addresses are loop invariants - 0.313 vs 0.339 ms for
    variant 2 per Llama-3-8B layer (profiles/r2_attention/); 3 is 4 without
    the unroll, 2 the plain DMA body, 1 the plain body unrolled, 0 stages K/V
    through registers (A/B runs)."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    o = torch.empty((B, S, Hq, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, Hq, S), dtype=torch.float32, device=q.device)
    if doc is not None:
        if variant is not None:
            raise ValueError("attn_fwd: variant= cannot be combined with doc=")
        _check_doc(doc, q, causal)
        st = _lib.lib().mxk_attn_fwd_doc(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                                         lse.data_ptr(), doc.doc_start.data_ptr(), B, S, Hq, Hkv, D,
                                         q.stride(1), k.stride(1), v.stride(1), float(scale),
                                         _lib.stream_ptr(q.device))
        _lib.check(st, "mxk_attn_fwd_doc")
        return o, lse
    variant = 4 if variant is None else variant
    st = _lib.lib().mxk_attn_fwd_variant(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                                         lse.data_ptr(), B, S, Hq, Hkv, D, q.stride(1),
                                         k.stride(1), v.stride(1), float(scale), int(causal),
                                         int(variant), _lib.stream_ptr(q.device))
    _lib.check(st, "mxk_attn_fwd")
    return o, lse


_BWD_VARIANT = int(os.environ.get("MXK_ATTN_BWD_VARIANT", "9"))


def attn_bwd(q, k, v, o, lse, dout, causal: bool = True, scale: float | None = None,
             dk=None, dv=None, variant: int | None = None, doc: DocMask | None = None):
    """HIP backward: returns (dq [B,S,Hq,D], dk [B,S,Hkv,D], dv [B,S,Hkv,D]).

    ``dk``/``dv`` may be preallocated views (e.g. slices of a fused dQKV
    buffer) with a token stride; by default they are fresh contiguous tensors.
    ``variant`` 0-9, default 9: the variants, their history and how a layout
    one does not take degrades (9 -> 6 -> 5) are listed beside ``AttnBwdPlan``
    in ``native/kernels/attention_plan.h``.  ``doc`` (a ``DocMask``): causal
    within a document, on the DOC forms of variant 5's kernels
    (``mxk_attn_bwd_doc``); it cannot be combined with ``variant``."""
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    if doc is not None and variant is not None:
        raise ValueError("attn_bwd: variant= cannot be combined with doc=")
    variant = _BWD_VARIANT if variant is None else variant
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    dout = dout.contiguous()
    dq = torch.empty((B, S, Hq, D), dtype=q.dtype, device=q.device)
    if dk is None:
        dk = torch.empty((B, S, Hkv, D), dtype=k.dtype, device=k.device)
    if dv is None:
        dv = torch.empty((B, S, Hkv, D), dtype=v.dtype, device=v.device)
    L = _lib.lib()
    if doc is not None:
        _check_doc(doc, q, causal)
        ws = torch.empty(L.mxk_attn_bwd_doc_workspace(B, S, Hq) // 4, dtype=torch.float32,
                         device=q.device)
        st = L.mxk_attn_bwd_doc(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                                dout.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                                dv.data_ptr(), ws.data_ptr(), doc.doc_start.data_ptr(),
                                doc.doc_end.data_ptr(), B, S, Hq, Hkv, D, q.stride(1), k.stride(1),
                                v.stride(1), dk.stride(1), dv.stride(1), float(scale),
                                _lib.stream_ptr(q.device))
        _lib.check(st, "mxk_attn_bwd_doc")
        return dq, dk, dv
    ws = torch.empty(L.mxk_attn_bwd_workspace_variant(B, S, Hq, int(variant)) // 4,
                     dtype=torch.float32, device=q.device)
    st = L.mxk_attn_bwd_variant(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                                dout.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                                dv.data_ptr(), ws.data_ptr(), B, S, Hq, Hkv, D, q.stride(1),
                                k.stride(1), v.stride(1), dk.stride(1), dv.stride(1),
                                float(scale), int(causal), int(variant),
                                _lib.stream_ptr(q.device))
    _lib.check(st, "mxk_attn_bwd")
    return dq, dk, dv


class _FlashAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal, scale):
        o, lse = attn_fwd(q, k, v, causal=causal, scale=scale)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.causal, ctx.scale = causal, scale
        return o

    @staticmethod
    def backward(ctx, dout):
        q, k, v, o, lse = ctx.saved_tensors
        dq, dk, dv = attn_bwd(q, k, v, o, lse, dout, causal=ctx.causal, scale=ctx.scale)
        return dq, dk, dv, None, None


class _DocFlashAttention(torch.autograd.Function):
    """Causal-within-a-document attention on the DOC kernels (``DocMask``)."""

    @staticmethod
    def forward(ctx, q, k, v, doc, scale):
        o, lse = attn_fwd(q, k, v, causal=True, scale=scale, doc=doc)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.doc, ctx.scale = doc, scale
        return o

    @staticmethod
    def backward(ctx, dout):
        q, k, v, o, lse = ctx.saved_tensors
        dq, dk, dv = attn_bwd(q, k, v, o, lse, dout, causal=True, scale=ctx.scale, doc=ctx.doc)
        return dq, dk, dv, None, None


# The fused projection's split + RoPE + attention as one autograd node
# (MXK_FUSED_ROPE_BWD=0 turns it off): the forward rotates q / k out of
# their qkv slices (the stand-alone RoPE pass) and runs the flash forward;
# the backward writes d(qkv) of the UN-rotated projection straight into one
# buffer - the RoPE backward fused into the dQ / dK stores of variant 9
# (mxk_attn_bwd_rope), dV in place - instead of separate dq / dk / dv, two
# RoPE passes over them and a dV copy (~400 MB of HBM traffic per
# Llama-3-8B layer at micro-batch 8).
_FUSED_ROPE_BWD = os.environ.get("MXK_FUSED_ROPE_BWD", "1") != "0"


def _split_qkv(qkv, hq: int, hkv: int, hd: int):
    """q [B,S,hq,hd], k and v [B,S,hkv,hd] as views of a fused [B, S, (hq + 2 hkv) hd] buffer."""
    B, S, _ = qkv.shape
    return (qkv[..., :hq * hd].view(B, S, hq, hd),
            qkv[..., hq * hd:(hq + hkv) * hd].view(B, S, hkv, hd),
            qkv[..., (hq + hkv) * hd:].view(B, S, hkv, hd))


def _fused_node_layout(S: int, hq: int, hkv: int, hd: int, cos) -> bool:
    """Heads and sequence lengths the fused RoPE nodes take (what backward
    variant 9 takes: GQA quads, S % 256), with rotary tables that cover S."""
    return (hd == HEAD_DIM and hkv > 0 and hq % hkv == 0 and (hq // hkv) % 4 == 0
            and S % 256 == 0 and cos.shape[0] >= S)


class _QKVRoPEAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cos, sin, hq: int, hkv: int, hd: int, causal: bool, scale):
        from .fused import _rope_launch
        q, k, v = _split_qkv(qkv, hq, hkv, hd)
        q = _rope_launch(q, cos, sin, 1.0)
        k = _rope_launch(k, cos, sin, 1.0)
        o, lse = attn_fwd(q, k, v, causal=causal, scale=scale)
        ctx.save_for_backward(q, k, v, o, lse, cos, sin)
        ctx.causal, ctx.scale, ctx.dims = causal, scale, (hq, hkv, hd)
        return o

    @staticmethod
    def backward(ctx, dout):
        q, k, v, o, lse, cos, sin = ctx.saved_tensors
        dqkv = _rope_attn_backward(q, k, v, o, lse, cos, sin, dout, ctx.dims, ctx.causal, ctx.scale)
        return dqkv, None, None, None, None, None, None, None


def _rope_attn_backward(q, k, v, o, lse, cos, sin, dout, dims, causal, scale):
    """d(qkv) [B, S, (hq + 2 hkv) hd] of the un-rotated projection from the
    rotated q / k the forward attended with."""
    from .fused import _rope_launch
    hq, hkv, hd = dims
    B, S = q.shape[:2]
    scale = scale if scale is not None else 1.0 / math.sqrt(hd)
    dqkv = torch.empty((B, S, (hq + 2 * hkv) * hd), dtype=q.dtype, device=q.device)
    dq, dk, dv = _split_qkv(dqkv, hq, hkv, hd)
    dout = dout.contiguous()
    if _BWD_VARIANT == 9:
        L = _lib.lib()
        ws = torch.empty(L.mxk_attn_bwd_workspace_variant(B, S, hq, 9) // 4,
                         dtype=torch.float32, device=q.device)
        st = L.mxk_attn_bwd_rope(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(),
                                 dout.data_ptr(), lse.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                                 dv.data_ptr(), ws.data_ptr(), B, S, hq, hkv, hd, q.stride(1),
                                 k.stride(1), v.stride(1), dq.stride(1), dk.stride(1),
                                 dv.stride(1), cos.data_ptr(), sin.data_ptr(), float(scale),
                                 int(causal), _lib.stream_ptr(q.device))
        if st == 0:
            return dqkv
        if st != 1:     # 1 = hipErrorInvalidValue: a layout variant 9 does not take
            _lib.check(st, "mxk_attn_bwd_rope")
    # other variants: the backward into the slices, then the RoPE passes
    gq, _, _ = attn_bwd(q, k, v, o, lse, dout, causal=causal, scale=scale, dk=dk, dv=dv)
    _rope_launch(gq, cos, sin, -1.0, out=dq)
    _rope_launch(dk, cos, sin, -1.0, out=dk)     # in place: a thread reads both halves first
    return dqkv


class _ProjRoPEAttention(torch.autograd.Function):
    """x -> qkv = x W^T -> RoPE(q, k) -> flash attention -> o as one node:
    the projection GEMM applies the rotary embedding in its epilogue
    (mxk_gemm_bf16_rope: q / k leave the GEMM rotated, no stand-alone RoPE
    pass and no rotated copies), the attention runs on q / k / v as strided
    views of that one buffer, and the backward takes d(qkv) of the
    un-rotated projection from the fused attention backward into the
    projection's input- and weight-gradient GEMMs (the weight gradient
    straight into the flat gradient buffer, as Linear does)."""

    @staticmethod
    def forward(ctx, x, weight, cos, sin, hq: int, hkv: int, hd: int, causal: bool, scale):
        from .fused import _rope_launch
        from .linear import _fwd
        B, S, K = x.shape
        x2 = x.reshape(-1, K)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        N = weight.shape[0]
        qkv = torch.empty((B * S, N), dtype=x.dtype, device=x.device)
        st = _lib.lib().mxk_gemm_bf16_rope(x2.data_ptr(), weight.data_ptr(), qkv.data_ptr(),
                                           B * S, N, K, x2.stride(0), weight.stride(0),
                                           qkv.stride(0), cos.data_ptr(), sin.data_ptr(), S,
                                           (hq + hkv) * hd, _lib.stream_ptr(x.device))
        qkv = qkv.view(B, S, N)
        q, k, v = _split_qkv(qkv, hq, hkv, hd)
        if st != 0:
            if st != 1:
                _lib.check(st, "mxk_gemm_bf16_rope")
            qkv.copy_(_fwd(x2, weight).view(B, S, N))
            _rope_launch(q, cos, sin, 1.0, out=q)      # in place
            _rope_launch(k, cos, sin, 1.0, out=k)
        o, lse = attn_fwd(q, k, v, causal=causal, scale=scale)
        ctx.save_for_backward(x2, weight, q, k, v, o, lse, cos, sin)
        ctx.causal, ctx.scale, ctx.dims, ctx.xshape = causal, scale, (hq, hkv, hd), x.shape
        return o

    @staticmethod
    def backward(ctx, dout):
        from .linear import _dgrad, _weight_grad
        x2, weight, q, k, v, o, lse, cos, sin = ctx.saved_tensors
        dqkv = _rope_attn_backward(q, k, v, o, lse, cos, sin, dout, ctx.dims, ctx.causal, ctx.scale)
        dqkv2 = dqkv.view(-1, dqkv.shape[-1])
        need_x, need_w = ctx.needs_input_grad[:2]
        dx = _dgrad(dqkv2, weight).view(ctx.xshape) if need_x else None
        dw = _weight_grad(weight, dqkv2, x2) if need_w else None
        return dx, dw, None, None, None, None, None, None, None


def proj_rope_attention(x: torch.Tensor, weight: torch.Tensor, cos: torch.Tensor,
                        sin: torch.Tensor, hq: int, hkv: int, hd: int, causal: bool = True,
                        scale: float | None = None):
    """o [B, S, hq, hd] = attention(RoPE(split(x W^T))) as one node (see
    _ProjRoPEAttention); None when the layout is not the fused path's."""
    if not (_FUSED_ROPE_BWD and _FUSED_ROPE_FWD and x.is_cuda and x.dtype == torch.bfloat16
            and weight.dtype == torch.bfloat16 and x.dim() == 3 and weight.is_contiguous()
            and weight.shape[0] == (hq + 2 * hkv) * hd
            and _fused_node_layout(x.shape[1], hq, hkv, hd, cos)):
        return None
    S = x.shape[1]
    return _ProjRoPEAttention.apply(x, weight, cos[:S].float().contiguous(),
                                    sin[:S].float().contiguous(), hq, hkv, hd, causal, scale)


# the rotary embedding in the fused QKV projection's GEMM epilogue
# (MXK_FUSED_ROPE_FWD=0: the GEMM, then the stand-alone RoPE pass)
_FUSED_ROPE_FWD = os.environ.get("MXK_FUSED_ROPE_FWD", "1") != "0"


def qkv_rope_attention(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, hq: int, hkv: int,
                       hd: int, causal: bool = True, scale: float | None = None):
    """Attention output o [B, S, hq, hd] of a fused projection qkv [B, S,
    (hq + 2 hkv) hd] with rotary embedding on q and k, as one autograd node
    whose backward returns d(qkv) from the fused kernels; None when the
    layout is not the fused path's (the caller then runs qkv_rope +
    flash_attention)."""
    if not (_FUSED_ROPE_BWD and qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 3
            and qkv.is_contiguous() and qkv.data_ptr() % 16 == 0
            and qkv.shape[-1] == (hq + 2 * hkv) * hd
            and _fused_node_layout(qkv.shape[1], hq, hkv, hd, cos)):
        return None
    S = qkv.shape[1]
    return _QKVRoPEAttention.apply(qkv, cos[:S].float().contiguous(), sin[:S].float().contiguous(),
                                   hq, hkv, hd, causal, scale)


def flash_attention(q, k, v, causal: bool = True, scale: float | None = None,
                    doc: DocMask | None = None) -> torch.Tensor:
    """Attention o [B,S,Hq,D] for q [B,S,Hq,D], k/v [B,S,Hkv,D] (GQA).

    Runs the HIP kernels for supported CUDA bf16 inputs (``supported``);
    CPU / other dtypes take the fp32 reference (used by the CPU tests).
    ``doc`` (a ``DocMask`` of q's [B, S] on q's device): causal within a
    document, for packed rows; ``causal=False`` with it is a ``ValueError``."""
    if doc is not None:
        _check_doc(doc, q, causal)
        if supported(q, k, v):
            return _DocFlashAttention.apply(q, k, v, doc, scale)
        if q.device.type == "cuda":
            raise RuntimeError(f"flash_attention: unsupported shape/layout on GPU: q "
                               f"{tuple(q.shape)} strides {q.stride()} (need head_dim 128, "
                               f"S % 128 == 0)")
        return attention_ref(q, k, v, causal=True, scale=scale, doc=doc)
    if supported(q, k, v):
        return _FlashAttention.apply(q, k, v, causal, scale)
    if q.device.type == "cuda":
        raise RuntimeError(f"flash_attention: unsupported shape/layout on GPU: q {tuple(q.shape)} "
                           f"strides {q.stride()} (need head_dim 128, S % 128 == 0)")
    return attention_ref(q, k, v, causal=causal, scale=scale)
