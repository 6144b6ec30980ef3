"""Bias-free linear layer whose weight gradient is written straight into the
flat gradient buffer of :class:`~mxk8s.parallel.ddp.FlatParamSpace`.

With stock ``nn.Linear`` autograd produces dW in a fresh tensor and
``AccumulateGrad`` adds it into the (pre-zeroed) flat ``.grad`` view: for
Llama-3-8B that is a 16 GB memset plus a 48 GB read-read-write add pass per
step (~10 ms on MI355X).  Here the dW GEMM (the hand-written layout kernel) writes its output
directly into ``weight.main_grad`` — overwrite on the first backward after
``zero_grad`` (so no memset), ``addmm_`` accumulation on later micro-batches —
and then tells the DDP bucketer that the gradient is ready (the role the
post-accumulate-grad hook plays for other parameters).
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from .gemm import gemm_bf16_ex

# dW = dy^T x has both operands token-major ("NT"): the hand-written
# layout-generic MFMA kernel beats hipBLASLt there (profiles/r1_gemm_layouts:
# +10-29 % on the Llama-3-8B wo/w13/w2 shapes); MXK_WGRAD=0 selects hipBLASLt.
_USE_MXK_WGRAD = os.environ.get("MXK_WGRAD", "1") != "0"
# dx = dy W has a K-major dy and an N-major W: the x2 schedule of the layout
# kernel runs it at 1390-1450 TF/s on the Llama-3-8B shapes (16k tokens)
# against hipBLASLt's 1350-1390 (profiles/r1_gemm_w4h/gemm_layouts_x2.log);
# MXK_DGRAD=0 selects hipBLASLt.
_USE_MXK_DGRAD = os.environ.get("MXK_DGRAD", "1") != "0"


# y = x W^T (both operands K-major) runs on the hand-written TN kernel (the
# validator's GEMM, gemm_bf16.hip) with the split tail when the last round of
# tiles is at most half full; no library GEMM in the training step.  Shapes
# that do not tile (M, N % 256, K % 64; tests, toy models) take the kernel's
# bounds-checked MFMA path; CPU tensors the PyTorch reference.
# MXK_FWD_LIB=1 (A/B measurements only, with MXK_FUSED_W13=0): the forward
# products on torch.matmul / hipBLASLt, the round-2 routing, so a same-box
# step A/B can price the hand-written forward path.
_FWD_LIB = os.environ.get("MXK_FWD_LIB", "0") == "1"


def _fwd(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    if _FWD_LIB or not x.is_cuda or x.dtype != torch.bfloat16 or weight.dtype != torch.bfloat16:
        return torch.matmul(x, weight.t())
    x2 = x.reshape(-1, x.shape[-1])
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    out = torch.empty((x2.shape[0], weight.shape[0]), device=x.device, dtype=x.dtype)
    w = weight if weight.is_contiguous() else weight.contiguous()
    if not gemm_bf16_ex(x2, w, True, True, out):
        from .gemm import gemm_bf16_tn
        gemm_bf16_tn(x2, w, out)          # bounds-checked MFMA kernel (any shape)
    return out.view(*x.shape[:-1], weight.shape[0])


def _wgrad_into(sink: torch.Tensor, dy2: torch.Tensor, x2: torch.Tensor) -> None:
    # no tail-heavy exception here: even without its split tail the 384-tile
    # wqkv wgrad (6144 x 4096, 1.5 rounds on 256 CUs) ran 1215 TF/s on the
    # layout kernel against hipBLASLt's 1150 (profiles/r1_gemm_m0/llama_*.log)
    if _USE_MXK_WGRAD and sink.is_cuda and dy2.is_contiguous() and x2.is_contiguous() and \
            gemm_bf16_ex(dy2, x2, False, False, sink):
        return
    torch.matmul(dy2.t(), x2, out=sink)


def _dgrad(dy: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    # tail-heavy outputs take the kernel's split tail (gemm_bf16_ex)
    if _USE_MXK_DGRAD and dy.is_cuda and dy.is_contiguous() and weight.is_contiguous():
        dy2 = dy.reshape(-1, dy.shape[-1])
        out = torch.empty((dy2.shape[0], weight.shape[1]), device=dy.device, dtype=dy.dtype)
        if gemm_bf16_ex(dy2, weight, True, False, out):
            return out.view(*dy.shape[:-1], weight.shape[1])
    return torch.matmul(dy, weight)


def _weight_grad(weight: torch.Tensor, dy: torch.Tensor, x: torch.Tensor):
    """dW = dy^T x: straight into weight.main_grad when the weight lives in a
    flat gradient buffer (then returns None), else returned."""
    x2 = x.reshape(-1, x.shape[-1])
    dy2 = dy.reshape(-1, dy.shape[-1])
    sink = getattr(weight, "main_grad", None)
    if sink is None:
        return torch.matmul(dy2.t(), x2)
    if weight._mxk_grad_fresh:
        _wgrad_into(sink, dy2, x2)
        weight._mxk_grad_fresh = False
    else:
        sink.addmm_(dy2.t(), x2)
    ready = getattr(weight, "_mxk_grad_ready", None)
    if ready is not None:
        ready()
    return None


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        return _fwd(x, weight)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx = _dgrad(dy, weight) if ctx.needs_input_grad[0] else None
        dw = _weight_grad(weight, dy, x) if ctx.needs_input_grad[1] else None
        return dx, dw


# ---- MXFP8 and MXFP4 (opt-in) -----------------------------------------------
# gemm_mxfp8_tn / gemm_mxfp4_tn contract over the contiguous axis of both
# operands, and an MX block lies along the contracted axis:
#   y  = x W^T      x [T, in] and W [out, in] quantised along their rows
#   dx = dy W       dy [T, out] along its rows, W along its columns: the
#                   transposed image quantize_<fmt>_t(W) [in, out]
#   dW = dy^T x     both along the token axis: quantize_<fmt>_t(dy) [out, T]
#                   and quantize_<fmt>_t(x) [in, T]
# dy is read once for both of its images (quantize_<fmt>_dual).
_MX_TILE = 256


def is_mxfp8_linear_shape(T: int, in_features: int, out_features: int) -> bool:
    """True when ``linear_mxfp8`` takes the shape: tokens, in and out features
    all positive multiples of 256, which gives M, N % 256 and K % 128 in each
    of the three products and scale rows that are whole dwords."""
    return all(n > 0 and n % _MX_TILE == 0 for n in (T, in_features, out_features))


def is_mxfp4_linear_shape(T: int, in_features: int, out_features: int) -> bool:
    """True when ``linear_mxfp4`` takes the shape: tokens, in and out features
    all positive multiples of 256, which gives M, N and K % 256 in each of the
    three products."""
    return is_mxfp8_linear_shape(T, in_features, out_features)


def _bf16_rows(t: torch.Tensor) -> torch.Tensor:
    """bf16 and unit inner stride (a row stride larger than the width stays)."""
    if t.dtype != torch.bfloat16:
        t = t.to(torch.bfloat16)
    return t if t.stride(1) == 1 else t.contiguous()


def _mx_ops(fmt: str):
    """(gemm_tn, quantize, quantize_t, quantize_dual) of "mxfp8" / "mxfp4", read
    from the format's module at every call."""
    if fmt == "mxfp8":
        from . import mxfp8 as m
    else:
        from . import mxfp4 as m
    return tuple(getattr(m, n.format(fmt)) for n in ("gemm_{}_tn", "quantize_{}", "quantize_{}_t",
                                                     "quantize_{}_dual"))


def _mx_weight_grad(weight: torch.Tensor, dyt, xt, gemm):
    """_weight_grad on an MX GEMM: dW = dequant(dy^T) dequant(x^T)^T."""
    sink = getattr(weight, "main_grad", None)
    if sink is None:
        return gemm(*dyt, *xt).to(weight.dtype)
    if weight._mxk_grad_fresh:
        if sink.dtype == torch.bfloat16:
            gemm(*dyt, *xt, out=sink)
        else:                                   # an fp32 flat buffer: the GEMM's output is bf16
            sink.copy_(gemm(*dyt, *xt))
        weight._mxk_grad_fresh = False
    else:
        sink.add_(gemm(*dyt, *xt))
    ready = getattr(weight, "_mxk_grad_ready", None)
    if ready is not None:
        ready()
    return None


GRAD_ROUNDINGS = ("nearest", "stochastic")


def _check_grad_rounding(grad_rounding, seed=None) -> None:
    from .mxfp4 import check_rounding
    if grad_rounding not in GRAD_ROUNDINGS:
        raise ValueError(f"grad_rounding must be one of {GRAD_ROUNDINGS}, got {grad_rounding!r}")
    if seed is not None:
        check_rounding(grad_rounding, seed)


def _mx_forward(fmt: str, ctx, x, weight):
    gemm, quantize, _, _ = _mx_ops(fmt)
    ctx.save_for_backward(x, weight)          # bf16, as _LinearFn: no quantised copy is held
    x2 = _bf16_rows(x.reshape(-1, x.shape[-1]))
    y = gemm(*quantize(x2), *quantize(_bf16_rows(weight)))
    return y.to(x.dtype).view(*x.shape[:-1], weight.shape[0])


def _mx_grad_images(fmt: str, dy2, need_rows: bool, need_t: bool, sr_seed=None):
    """((q, s) or None, (qt, st) or None) of an output gradient: the row image for
    the input gradient, the transposed one for the weight gradient, from one
    read when both are needed.  sr_seed (MXFP4): stochastic rounding, the row
    image with this seed and the transposed image with the next one, whichever
    of the two a call needs."""
    _, quantize, quantize_t, quantize_dual = _mx_ops(fmt)
    sr = () if sr_seed is None else ("stochastic", sr_seed)
    if need_rows and need_t:
        dq, ds, dqt, dst = quantize_dual(dy2, *sr)
        return (dq, ds), (dqt, dst)
    if need_rows:
        return quantize(dy2, *sr), None
    if need_t:
        if sr_seed is not None:
            return None, quantize_t(dy2, "stochastic", (sr_seed + 1) % 2 ** 64)
        return None, quantize_t(dy2)
    return None, None


def _mx_backward(fmt: str, ctx, dy, sr_seed=None):
    """sr_seed (MXFP4): dy is quantised with stochastic rounding
    (_mx_grad_images); W^T and x^T stay round-to-nearest."""
    gemm, _, quantize_t, _ = _mx_ops(fmt)
    x, weight = ctx.saved_tensors
    need_x, need_w = ctx.needs_input_grad[:2]
    dy2 = _bf16_rows(dy.reshape(-1, dy.shape[-1]))
    rows, cols = _mx_grad_images(fmt, dy2, need_x, need_w, sr_seed)
    dx = dw = None
    if need_x:
        dx = gemm(*rows, *quantize_t(_bf16_rows(weight)))
        dx = dx.to(x.dtype).view(x.shape)
    if need_w:
        x2 = _bf16_rows(x.reshape(-1, x.shape[-1]))
        dw = _mx_weight_grad(weight, cols, quantize_t(x2), gemm)
    return dx, dw


class _LinearMxfp8Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        return _mx_forward("mxfp8", ctx, x, weight)

    @staticmethod
    def backward(ctx, dy):
        return _mx_backward("mxfp8", ctx, dy)


class _LinearMxfp4Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight):
        return _mx_forward("mxfp4", ctx, x, weight)

    @staticmethod
    def backward(ctx, dy):
        return _mx_backward("mxfp4", ctx, dy)


class _LinearMxfp4SrFn(torch.autograd.Function):
    """_LinearMxfp4Fn whose backward quantises dy with stochastic rounding.  The
    seed is fixed at forward time: the explicit one, else the next of the seed
    source (mxfp4.sr_next), which follows the order of the module calls and not
    the autograd engine's."""

    @staticmethod
    def forward(ctx, x, weight, seed):
        if seed is None:
            from .mxfp4 import sr_next
            seed = sr_next()
        ctx.sr_seed = seed
        return _mx_forward("mxfp4", ctx, x, weight)

    @staticmethod
    def backward(ctx, dy):
        return (*_mx_backward("mxfp4", ctx, dy, ctx.sr_seed), None)


def _mx_linear(name: str, fn, x: torch.Tensor, weight: torch.Tensor, *extra) -> torch.Tensor:
    if weight.dim() != 2 or x.dim() < 1 or x.shape[-1] != weight.shape[1]:
        raise ValueError(f"{name}: x {tuple(x.shape)} does not match weight "
                         f"{tuple(weight.shape)}")
    T = x.numel() // x.shape[-1] if x.shape[-1] else 0
    if not is_mxfp8_linear_shape(T, weight.shape[1], weight.shape[0]):
        raise ValueError(f"{name} needs tokens, in_features and out_features to be positive "
                         f"multiples of {_MX_TILE}, got T={T} in={weight.shape[1]} "
                         f"out={weight.shape[0]}")
    return fn.apply(x, weight, *extra)


def linear_mxfp8(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """``x @ weight.T`` whose forward product, input gradient and weight gradient
    all run on the MXFP8 GEMM (``gemm_mxfp8_tn``), each operand quantised in
    blocks of 32 along the axis its product contracts.  ``x`` is ``[..., in]``,
    ``weight`` ``[out, in]``; tensors that are not bf16 are cast to bf16 for
    quantising and the results returned in their own dtype.  The weight
    gradient keeps the ``main_grad`` contract of :class:`Linear`.  Raises
    ``ValueError`` unless :func:`is_mxfp8_linear_shape` holds."""
    return _mx_linear("linear_mxfp8", _LinearMxfp8Fn, x, weight)


def linear_mxfp4(x: torch.Tensor, weight: torch.Tensor, grad_rounding: str = "nearest",
                 seed: int | None = None) -> torch.Tensor:
    """``x @ weight.T`` whose forward product, input gradient and weight gradient
    all run on the MXFP4 GEMM (``gemm_mxfp4_tn``), each operand quantised in
    blocks of 32 along the axis its product contracts.  ``x`` is ``[..., in]``,
    ``weight`` ``[out, in]``; tensors that are not bf16 are cast to bf16 for
    quantising and the results returned in their own dtype.  The weight
    gradient keeps the ``main_grad`` contract of :class:`Linear`.  Raises
    ``ValueError`` unless :func:`is_mxfp4_linear_shape` holds.

    By default all three products round to nearest even, like the rest of the
    MX code here.  FP4 gradients under round-to-nearest-even are biased: the
    OCP scale clamps scaled block maxima in (6, 8) to 6, and with the
    project's reference quantiser every input gradient comes out shrunk by
    about 8 % (projection of the error of ``dx`` on the exact product of the
    same operands).  ``grad_rounding="stochastic"`` quantises ``dy``, in both
    of its images, with stochastic rounding and a block scale that does not
    clip (``quantize_mxfp4*(.., "stochastic", seed)``): the error is zero in the
    mean (that of the mean of N draws falls as 1/sqrt(N)).  One draw has the
    error norm of round-to-nearest on evenly filled blocks and a larger one on
    blocks whose elements lie mostly far below the block maximum, which
    round-to-nearest sends to zero.  The forward product and the ``W^T`` / ``x^T``
    images of the backward stay round-to-nearest.  The row image of ``dy``
    draws with ``seed`` and its transposed image with ``seed + 1``, whether one
    or both gradients are needed; ``seed=None`` takes ``sr_next()`` at forward
    time.  Either way the switch changes the numerics of the step (e2m1's own
    error against the bf16 product is ~21 % per product), and no convergence
    run backs either rounding yet."""
    _check_grad_rounding(grad_rounding, seed)
    if grad_rounding == "stochastic":
        return _mx_linear("linear_mxfp4", _LinearMxfp4SrFn, x, weight, seed)
    return _mx_linear("linear_mxfp4", _LinearMxfp4Fn, x, weight)


# y = swiglu(gu) W^T with the SwiGLU backward fused into the input-gradient
# GEMM's epilogue (mxk_gemm_bf16_dgrad_swiglu): d(act) = dy W never goes to
# HBM (0.94 GB less traffic per Llama-3-8B layer, no separate element-wise
# pass, d(act) kept in fp32).  Round 1 measured it step-neutral (the 8-B
# per-lane g/u accesses made the epilogue slow); with the LDS-staged epilogue
# (whole-line g/u accesses) the kernel runs 1.52 ms against 1.71 and the step
# gains 1.1 % (profiles/r2_split_tail/).  MXK_FUSED_SWIGLU=0 runs the
# unfused pair.
_USE_FUSED_SWIGLU = os.environ.get("MXK_FUSED_SWIGLU", "1") != "0"


def _dgrad_swiglu(dy: torch.Tensor, weight: torch.Tensor, gu: torch.Tensor) -> torch.Tensor:
    from . import _lib
    from .fused import swiglu_bwd
    F = weight.shape[1]
    dy2 = dy.reshape(-1, dy.shape[-1])
    gu2 = gu.reshape(-1, 2 * F)
    if _USE_FUSED_SWIGLU and dy2.is_contiguous() and gu2.is_contiguous() and weight.is_contiguous():
        dgu = torch.empty_like(gu2)
        st = _lib.lib().mxk_gemm_bf16_dgrad_swiglu(
            dy2.data_ptr(), weight.data_ptr(), gu2.data_ptr(), dgu.data_ptr(), dy2.shape[0], F,
            dy2.shape[1], dy2.stride(0), weight.stride(0), _lib.stream_ptr(dy.device))
        if st == 0:
            return dgu.view(gu.shape)
    return swiglu_bwd(gu, _dgrad(dy, weight))


class _SwiGLULinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu, weight):
        from .fused import swiglu_fwd
        h = swiglu_fwd(gu)
        ctx.save_for_backward(gu, h, weight)
        return _fwd(h, weight)

    @staticmethod
    def backward(ctx, dy):
        gu, h, weight = ctx.saved_tensors
        dgu = _dgrad_swiglu(dy, weight, gu) if ctx.needs_input_grad[0] else None
        dw = _weight_grad(weight, dy, h) if ctx.needs_input_grad[1] else None
        return dgu, dw


# gu = x W13^T and h = silu(g) * u in ONE launch (mxk_gemm_bf16_w13_swiglu:
# the activation runs in the GEMM's epilogue from the fp32 accumulators, the
# separate element-wise pass over gu disappears).  MXK_FUSED_W13=0 runs the
# GEMM and mxk_swiglu_fwd separately.
_USE_FUSED_W13 = os.environ.get("MXK_FUSED_W13", "1") != "0"


def w13_swiglu(x2: torch.Tensor, w13: torch.Tensor):
    """(gu, h) of the MLP up-projection, or None when the fused kernel does not
    take the shape (M % 256, F % 128, K % 64, aligned, bf16 GPU tensors)."""
    from . import _lib
    if not (_USE_FUSED_W13 and x2.is_cuda and x2.dtype == torch.bfloat16 and
            w13.dtype == torch.bfloat16 and x2.is_contiguous() and w13.is_contiguous()):
        return None
    M, K = x2.shape
    F = w13.shape[0] // 2
    gu = torch.empty((M, 2 * F), device=x2.device, dtype=x2.dtype)
    h = torch.empty((M, F), device=x2.device, dtype=x2.dtype)
    st = _lib.lib().mxk_gemm_bf16_w13_swiglu(x2.data_ptr(), w13.data_ptr(), gu.data_ptr(),
                                             h.data_ptr(), M, F, K, x2.stride(0), w13.stride(0),
                                             gu.stride(0), h.stride(0), _lib.stream_ptr(x2.device))
    if st == 1:      # hipErrorInvalidValue: shape / alignment not taken
        return None
    _lib.check(st, "mxk_gemm_bf16_w13_swiglu")
    return gu, h


class _SwiGLUMLPFn(torch.autograd.Function):
    """y = swiglu(x W13^T) W2^T as one autograd node: fused up-projection +
    activation forward, fused dgrad-SwiGLU backward; both weight gradients go
    straight into the flat gradient buffer (W2's first, as autograd would
    order the two nodes)."""

    @staticmethod
    def forward(ctx, x, w13, w2):
        from .fused import swiglu_fwd
        x2 = x.reshape(-1, x.shape[-1])
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        r = w13_swiglu(x2, w13)
        if r is None:
            gu = _fwd(x2, w13)
            h = swiglu_fwd(gu)
        else:
            gu, h = r
        ctx.save_for_backward(x2, gu, h, w13, w2)
        ctx.xshape = x.shape
        return _fwd(h, w2).view(*x.shape[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, gu, h, w13, w2 = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1])
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        need_x, need_w13, need_w2 = ctx.needs_input_grad
        dgu = _dgrad_swiglu(dy2, w2, gu) if (need_x or need_w13) else None
        dw2 = _weight_grad(w2, dy2, h) if need_w2 else None
        dx = _dgrad(dgu, w13).view(ctx.xshape) if need_x else None
        dw13 = _weight_grad(w13, dgu, x2) if need_w13 else None
        return dx, dw13, dw2


def swiglu_mlp(x: torch.Tensor, w13: torch.Tensor, w2: torch.Tensor) -> torch.Tensor:
    return _SwiGLUMLPFn.apply(x, w13, w2)


# ---- the MX MLP as one node ------------------------------------------------------
# w2(swiglu(w13(x))) on an MX format as two Linear nodes writes h = swiglu(gu)
# and dgu to HBM as bf16 only for a quantiser to read them back (h twice), and
# saves h beside gu.  Here SwiGLU and its backward run inside the quantisers
# (swiglu_quantize_<fmt>, .._t, swiglu_bwd_quantize_<fmt>_dual), whose images
# equal the composition's bit for bit, so the node computes what the two
# Linear nodes compute, bit for bit, with 3 launches and one saved [T, F]
# tensor less per layer.  MXK_MX_FUSED_SWIGLU=0 runs the two nodes;
# profiles/mx_swiglu/ has the measurement the default rests on.
MX_FUSED_SWIGLU_DEFAULT = "1"


def _mx_fused_swiglu_env(environ=os.environ) -> bool:
    return environ.get("MXK_MX_FUSED_SWIGLU", MX_FUSED_SWIGLU_DEFAULT) != "0"


_USE_MX_FUSED_SWIGLU = _mx_fused_swiglu_env()


def _mx_swiglu_ops(fmt: str):
    """(swiglu_quantize, swiglu_quantize_t, swiglu_bwd_quantize_dual) of "mxfp8" /
    "mxfp4", read from the format's module at every call, as _mx_ops."""
    if fmt == "mxfp8":
        from . import mxfp8 as m
    else:
        from . import mxfp4 as m
    return tuple(getattr(m, n.format(fmt)) for n in ("swiglu_quantize_{}", "swiglu_quantize_{}_t",
                                                     "swiglu_bwd_quantize_{}_dual"))


class _SwiGLUMLPMxFn(torch.autograd.Function):
    """y = swiglu(x W13^T) W2^T with all five products on an MX GEMM: the MX twin
    of _SwiGLUMLPFn.  Saves x, gu and the weights, not h.  seeds: None for
    round-to-nearest gradients, else (w13's, w2's) of the stochastic quantisers
    of dgu and dy, or () to draw them here from mxfp4.sr_next(), w13's first,
    the order in which the two Linear calls draw them."""

    @staticmethod
    def forward(ctx, x, w13, w2, fmt, seeds):
        gemm, quantize, _, _ = _mx_ops(fmt)
        swiglu_quantize = _mx_swiglu_ops(fmt)[0]
        if seeds == ():
            from .mxfp4 import sr_next
            seeds = (sr_next(), sr_next())
        x2 = _bf16_rows(x.reshape(-1, x.shape[-1]))
        gu = gemm(*quantize(x2), *quantize(_bf16_rows(w13)))
        y = gemm(*swiglu_quantize(gu), *quantize(_bf16_rows(w2)))
        ctx.save_for_backward(x2, gu, w13, w2)
        ctx.fmt, ctx.seeds, ctx.xshape, ctx.xdtype = fmt, seeds, x.shape, x.dtype
        return y.to(x.dtype).view(*x.shape[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        fmt = ctx.fmt
        gemm, _, quantize_t, _ = _mx_ops(fmt)
        _, swiglu_quantize_t, swiglu_bwd_quantize_dual = _mx_swiglu_ops(fmt)
        x2, gu, w13, w2 = ctx.saved_tensors
        need_x, need_w13, need_w2 = ctx.needs_input_grad[:3]
        need_gu = need_x or need_w13
        seed13, seed2 = ctx.seeds or (None, None)
        dy2 = _bf16_rows(dy.reshape(-1, dy.shape[-1]))
        rows, cols = _mx_grad_images(fmt, dy2, need_gu, need_w2, seed2)
        dx = dw13 = dw2 = None
        if need_gu:
            dh = gemm(*rows, *quantize_t(_bf16_rows(w2)))
        if need_w2:                              # W2's first, as autograd orders the two nodes
            dw2 = _mx_weight_grad(w2, cols, swiglu_quantize_t(gu), gemm)
        if need_gu:
            # both images of dgu even where one gradient is not needed: each is
            # the image the one-sided quantiser would draw (seed, seed + 1)
            sr = () if seed13 is None else ("stochastic", seed13)
            gq, gs, gqt, gst = swiglu_bwd_quantize_dual(gu, dh, *sr)
            del dh
            if need_x:
                dx = gemm(gq, gs, *quantize_t(_bf16_rows(w13)))
                dx = dx.to(ctx.xdtype).view(ctx.xshape)
            if need_w13:
                dw13 = _mx_weight_grad(w13, (gqt, gst), quantize_t(x2), gemm)
        return dx, dw13, dw2, None, None


def swiglu_mlp_mx(x: torch.Tensor, w13: torch.Tensor, w2: torch.Tensor, fmt: str,
                  grad_rounding: str = "nearest", seeds=None) -> torch.Tensor:
    """``swiglu(x @ w13.T) @ w2.T`` (``w13`` ``[2F, in]`` = [gate | up], ``w2``
    ``[out, F]``) as one autograd node whose five products run on the MX GEMM of
    ``fmt`` (``"mxfp8"`` / ``"mxfp4"``): what ``Linear(compute=fmt)`` followed by
    ``SwiGLULinear(compute=fmt)`` computes, bit for bit, with SwiGLU and its
    gradient computed inside the quantisers, so neither ``swiglu(gu)`` nor
    ``d(gu)`` is written as bf16 and ``swiglu(gu)`` is not saved.  The weight
    gradients keep the ``main_grad`` contract of :class:`Linear`, ``w2``'s first.

    ``grad_rounding="stochastic"`` (MXFP4 only) rounds ``dy`` and ``d(gu)``
    stochastically; ``seeds`` is ``(w13's, w2's)``, or ``None`` to draw two from
    ``mxfp4.sr_next()`` at forward time, ``w13``'s first.  Raises ``ValueError``
    unless :func:`is_mxfp8_linear_shape` holds for both layers."""
    if fmt not in ("mxfp8", "mxfp4"):
        raise ValueError(f"fmt must be \"mxfp8\" or \"mxfp4\", got {fmt!r}")
    _check_grad_rounding(grad_rounding)
    if grad_rounding != "nearest" and fmt != "mxfp4":
        raise ValueError(f"grad_rounding={grad_rounding!r} needs fmt=\"mxfp4\", got {fmt!r}")
    if seeds is not None:
        if grad_rounding != "stochastic":
            raise ValueError("seeds are only taken with grad_rounding=\"stochastic\"")
        if not isinstance(seeds, (tuple, list)) or len(seeds) != 2:
            raise ValueError(f"seeds must be (w13's, w2's), got {seeds!r}")
        for seed in seeds:
            _check_grad_rounding(grad_rounding, seed)
        seeds = tuple(seeds)
    elif grad_rounding == "stochastic":
        seeds = ()
    if w13.dim() != 2 or w2.dim() != 2 or x.dim() < 1 or x.shape[-1] != w13.shape[1] or \
            w13.shape[0] != 2 * w2.shape[1]:
        raise ValueError(f"swiglu_mlp_mx: x {tuple(x.shape)}, w13 {tuple(w13.shape)} and w2 "
                         f"{tuple(w2.shape)} do not match")
    T = x.numel() // x.shape[-1] if x.shape[-1] else 0
    if not (is_mxfp8_linear_shape(T, w13.shape[1], w13.shape[0]) and
            is_mxfp8_linear_shape(T, w2.shape[1], w2.shape[0])):
        raise ValueError(f"swiglu_mlp_mx needs tokens, in, ffn and out features to be positive "
                         f"multiples of {_MX_TILE}, got T={T} in={w13.shape[1]} "
                         f"ffn={w2.shape[1]} out={w2.shape[0]}")
    return _SwiGLUMLPMxFn.apply(x, w13, w2, fmt, seeds)


class Linear(nn.Linear):
    """``nn.Linear(bias=False)`` with the direct-to-flat-buffer weight gradient.

    ``compute="mxfp8"`` (opt-in) runs the three products of a call on the
    MXFP8 GEMM (:func:`linear_mxfp8`) when :func:`is_mxfp8_linear_shape` holds
    for it, i.e. tokens, in and out features are multiples of 256.  Any other
    call (toy shapes, a ragged batch) silently takes the bf16 path.
    ``compute="mxfp4"`` does the same with the MXFP4 GEMM
    (:func:`linear_mxfp4`, :func:`is_mxfp4_linear_shape`);
    ``grad_rounding="stochastic"`` (MXFP4 only) quantises the output gradient
    of those calls with stochastic rounding, a seed from ``mxfp4.sr_next()`` per
    call."""

    COMPUTE = ("bf16", "mxfp8", "mxfp4")
    _MX_FN = {"mxfp8": _LinearMxfp8Fn, "mxfp4": _LinearMxfp4Fn}

    def __init__(self, in_features: int, out_features: int, compute: str = "bf16",
                 grad_rounding: str = "nearest", **kw):
        if compute not in self.COMPUTE:
            raise ValueError(f"compute must be one of {self.COMPUTE}, got {compute!r}")
        _check_grad_rounding(grad_rounding)
        if grad_rounding != "nearest" and compute != "mxfp4":
            raise ValueError(f"grad_rounding={grad_rounding!r} needs compute=\"mxfp4\", got {compute!r}")
        super().__init__(in_features, out_features, bias=False, **kw)
        self.compute = compute
        self.grad_rounding = grad_rounding
        self.weight._mxk_direct_grad = True

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        fn = self._MX_FN.get(self.compute)
        if fn is not None and is_mxfp8_linear_shape(      # one predicate for both formats
                x.numel() // self.in_features, self.in_features, self.out_features):
            if self.grad_rounding == "stochastic":
                return _LinearMxfp4SrFn.apply(x, self.weight, None)
            return fn.apply(x, self.weight)
        return _LinearFn.apply(x, self.weight)


class SwiGLULinear(Linear):
    """Down projection applied to swiglu(gu), gu = [gate | up] of width
    2 * in_features: ``w2(swiglu(gu))`` as one node whose backward fuses the
    SwiGLU gradient into the input-gradient GEMM.  CPU / non-bf16 inputs take
    the plain composition, and so does every ``compute`` but ``"bf16"``: the
    fused dgrad-SwiGLU kernel is a bf16 kernel."""

    def forward(self, gu: torch.Tensor) -> torch.Tensor:
        if gu.device.type == "cpu" or gu.dtype != torch.bfloat16 or self.compute != "bf16":
            from .fused import swiglu
            return super().forward(swiglu(gu))
        return _SwiGLULinearFn.apply(gu, self.weight)
