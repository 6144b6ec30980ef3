"""MXFP8 quantiser and block-scaled MFMA GEMM op (``native/kernels/gemm_mxfp8.hip``).

The format is OCP MX with e4m3 elements (``torch.float8_e4m3fn``: OCP, not
fnuz), blocks of 32 consecutive K elements and one E8M0 scale byte per block:

====== ============= ==========================
tensor shape         storage
====== ============= ==========================
``x``  ``[R, K]``    bf16, ``K % 32 == 0``
``q``  ``[R, K]``    ``torch.float8_e4m3fn``
``s``  ``[R, K/32]`` ``torch.uint8``, row-major
====== ============= ==========================

Per block: ``amax = max |x|`` in fp32, ``e = floor(log2(amax)) - 8`` (8 is the
emax of e4m3), scale byte ``clamp(e, -127, 127) + 127`` (127 for an all-zero
block), element ``RNE_to_e4m3(clamp(x * 2^-e, -448, 448))``: the saturation is
explicit.  Only finite inputs are in scope; Inf / NaN give unspecified bytes.

``gemm_mxfp8_tn(aq, a_s, bq, b_s)`` computes ``dequant(a) @ dequant(b).T`` with
fp32 accumulation and bf16 output on ``v_mfma_scale_f32_32x32x64_f8f6f4``.
The product of the *dequantised* operands is the reference of every check:
against the unquantised bf16 product the format's own error is about 7 %.

``quantize_mxfp8_t(x)`` and ``quantize_mxfp8_dual(x)`` give the images of the
transposed tensor, whose blocks are 32 consecutive *rows* of ``x``, without a
transposed copy: what the backward products of a linear layer contract over
(``mxk8s.ops.linear.linear_mxfp8``).

GPU tensors always run the hand-written kernels (no fallback); CPU tensors
take the pure-torch reference path.
"""
from __future__ import annotations

import torch

from . import _mx
from ._mx import BLOCK, TILE_M, TILE_N  # noqa: F401  (this module's constants, as before)

E4M3_MAX = 448.0
E4M3_EMAX = 8
TILE_K = 128


def quantize_mxfp8_ref(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Pure-torch MXFP8 quantiser (any device): the definition the kernel is
    bit-identical to.  Finite inputs only."""
    _mx.check_x(x)
    R, K = x.shape
    xb = x.float().reshape(R, K // BLOCK, BLOCK)
    e = _mx.block_exponent(xb, E4M3_EMAX)
    y = torch.ldexp(xb, -e.unsqueeze(2)).clamp(-E4M3_MAX, E4M3_MAX)
    q = y.reshape(R, K).to(torch.float8_e4m3fn)
    s = (e + 127).to(torch.uint8)
    return q, s


def quantize_mxfp8(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """bf16 ``[R, K]`` -> (e4m3 ``[R, K]``, uint8 E8M0 scales ``[R, K/32]``).
    Finite inputs only.  A row stride larger than K is fine."""
    return _mx.quantize_rows("mxfp8", 1, torch.float8_e4m3fn, quantize_mxfp8_ref, x)


def quantize_mxfp8_t(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """bf16 ``[R, C]`` -> (e4m3 ``[C, R]``, uint8 E8M0 scales ``[C, R/32]``): the
    images of ``quantize_mxfp8(x.t().contiguous())``, bit for bit, from one pass
    over ``x``.  The MX blocks are 32 consecutive *rows* of ``x`` (``R % 32 ==
    0``; any ``C``), which is what a product contracting over the row axis of
    ``x`` needs.  Finite inputs only.  A row stride larger than C is fine."""
    return _mx.quantize_t("mxfp8", 1, torch.float8_e4m3fn, quantize_mxfp8_ref, x)


def quantize_mxfp8_dual(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor,
                                                  torch.Tensor]:
    """``(q, s, qt, st)``: ``quantize_mxfp8(x)`` and ``quantize_mxfp8_t(x)`` from
    one read of ``x`` (bf16 ``[R, C]``, both multiples of 32)."""
    return _mx.quantize_dual("mxfp8", 1, torch.float8_e4m3fn, quantize_mxfp8_ref, x)


def swiglu_quantize_mxfp8(gu: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``quantize_mxfp8(h)`` of ``h = silu(g) * u`` for bf16 ``gu = [g | u]``
    ``[T, 2F]`` (``F % 32 == 0``), bit for bit, without ``h`` in memory: one kernel
    (``native/kernels/swiglu_quantize_mx.hip``) for GPU tensors with 16-byte
    aligned rows, the composition of the two ops for every other tensor."""
    return _mx.swiglu_quantize_rows("mxfp8", 1, torch.float8_e4m3fn, quantize_mxfp8, gu)


def swiglu_quantize_mxfp8_t(gu: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``quantize_mxfp8_t(h)`` of ``h = silu(g) * u`` (``T % 32 == 0`` as well); see
    :func:`swiglu_quantize_mxfp8`."""
    return _mx.swiglu_quantize_t("mxfp8", 1, torch.float8_e4m3fn, quantize_mxfp8_t, gu)


def swiglu_bwd_quantize_mxfp8_dual(gu: torch.Tensor, dh: torch.Tensor):
    """``quantize_mxfp8_dual(dgu)`` of the SwiGLU gradient ``dgu = [dg | du]``
    ``[T, 2F]`` for ``gu`` ``[T, 2F]`` and ``dh`` ``[T, F]`` (bf16, ``T`` and ``F``
    multiples of 32), bit for bit, from one read of ``gu`` and ``dh`` and without
    ``dgu`` in memory; see :func:`swiglu_quantize_mxfp8`."""
    return _mx.swiglu_bwd_quantize_dual("mxfp8", 1, torch.float8_e4m3fn, quantize_mxfp8_dual, gu, dh)


def _check_pair(q: torch.Tensor, s: torch.Tensor, qn: str, sn: str) -> None:
    _mx.check_pair(q, s, qn, sn, torch.float8_e4m3fn, "float8_e4m3fn", 1)


def dequantize_mxfp8(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """fp32 ``q * 2^(s - 127)`` per block; pure torch, any device."""
    _check_pair(q, s, "q", "s")
    R, K = q.shape
    e = s.to(torch.int32) - 127
    return torch.ldexp(q.float().reshape(R, K // BLOCK, BLOCK), e.unsqueeze(2)).reshape(R, K)


def is_fast_shape_mxfp8(M: int, N: int, K: int) -> bool:
    return _mx.is_fast_shape(M, N, K, TILE_K)


def gemm_mxfp8_tn(aq: torch.Tensor, a_s: torch.Tensor, bq: torch.Tensor, b_s: torch.Tensor,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """``dequant(aq, a_s) @ dequant(bq, b_s).T`` -> bf16 ``[M, N]``.

    ``aq`` ``[M, K]`` and ``bq`` ``[N, K]`` are e4m3, ``a_s`` / ``b_s`` their
    uint8 scales ``[., K/32]``.  Contract: M and N multiples of 256, K of 128.
    Row strides may exceed the logical widths (views into wider buffers, K
    slices of ``q`` with the matching column slice of ``s``) as long as
    element rows stay 16-byte and scale rows 4-byte aligned."""
    return _mx.gemm_tn("mxfp8", TILE_K, 1, _check_pair, dequantize_mxfp8, aq, a_s, bq, b_s, out)
