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

from . import _lib

BLOCK = 32          # elements per scale
E4M3_MAX = 448.0
E4M3_EMAX = 8
TILE_M = TILE_N = 256
TILE_K = 128


def _check_x(x: torch.Tensor) -> None:
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a tensor")
    if x.dtype != torch.bfloat16:
        raise TypeError(f"x must be bfloat16, got {x.dtype}")
    if x.dim() != 2:
        raise ValueError(f"x must be 2-D, got shape {tuple(x.shape)}")
    if x.shape[0] == 0 or x.shape[1] == 0 or x.shape[1] % BLOCK:
        raise ValueError(f"x must be [R, K] with R > 0 and K a positive multiple of {BLOCK}, "
                         f"got {tuple(x.shape)}")
    if x.stride(1) != 1:
        raise ValueError("x must be K-contiguous (stride(1) == 1)")


def quantize_mxfp8_ref(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Pure-torch MXFP8 quantiser (any device): the definition the kernel is
    bit-identical to.  Finite inputs only."""
    _check_x(x)
    R, K = x.shape
    xb = x.float().reshape(R, K // BLOCK, BLOCK)
    amax = xb.abs().amax(dim=2)
    _, ex = torch.frexp(amax)                     # amax = m 2^ex, m in [0.5, 1)
    e = (ex.to(torch.int32) - 1 - E4M3_EMAX).clamp(-127, 127)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    y = torch.ldexp(xb, -e.unsqueeze(2)).clamp(-E4M3_MAX, E4M3_MAX)
    q = y.reshape(R, K).to(torch.float8_e4m3fn)
    s = (e + 127).to(torch.uint8)
    return q, s


def quantize_mxfp8(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """bf16 ``[R, K]`` -> (e4m3 ``[R, K]``, uint8 E8M0 scales ``[R, K/32]``).
    Finite inputs only.  A row stride larger than K is fine."""
    _check_x(x)
    if x.device.type == "cpu":
        return quantize_mxfp8_ref(x)
    R, K = x.shape
    q = torch.empty((R, K), dtype=torch.float8_e4m3fn, device=x.device)
    s = torch.empty((R, K // BLOCK), dtype=torch.uint8, device=x.device)
    st = _lib.lib().mxk_quantize_mxfp8(x.data_ptr(), q.data_ptr(), s.data_ptr(), R, K, x.stride(0),
                                       q.stride(0), s.stride(0), _lib.stream_ptr(x.device))
    _lib.check(st, "mxk_quantize_mxfp8")
    return q, s


def _check_xt(x: torch.Tensor, dual: bool) -> None:
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a tensor")
    if x.dtype != torch.bfloat16:
        raise TypeError(f"x must be bfloat16, got {x.dtype}")
    if x.dim() != 2:
        raise ValueError(f"x must be 2-D, got shape {tuple(x.shape)}")
    R, C = x.shape
    if R == 0 or C == 0 or R % BLOCK or (dual and C % BLOCK):
        raise ValueError(f"x must be [R, C] with R a positive multiple of {BLOCK} and C "
                         + (f"a positive multiple of {BLOCK}" if dual else "> 0")
                         + f", got {tuple(x.shape)}")
    if x.stride(1) != 1:
        raise ValueError("x must be row-major (stride(1) == 1)")


def quantize_mxfp8_t(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """bf16 ``[R, C]`` -> (e4m3 ``[C, R]``, uint8 E8M0 scales ``[C, R/32]``): the
    images of ``quantize_mxfp8(x.t().contiguous())``, bit for bit, from one pass
    over ``x``.  The MX blocks are 32 consecutive *rows* of ``x`` (``R % 32 ==
    0``; any ``C``), which is what a product contracting over the row axis of
    ``x`` needs.  Finite inputs only.  A row stride larger than C is fine."""
    _check_xt(x, dual=False)
    if x.device.type == "cpu":
        return quantize_mxfp8_ref(x.t().contiguous())
    R, C = x.shape
    qt = torch.empty((C, R), dtype=torch.float8_e4m3fn, device=x.device)
    st = torch.empty((C, R // BLOCK), dtype=torch.uint8, device=x.device)
    rc = _lib.lib().mxk_quantize_mxfp8_t(x.data_ptr(), qt.data_ptr(), st.data_ptr(), R, C,
                                         x.stride(0), qt.stride(0), st.stride(0),
                                         _lib.stream_ptr(x.device))
    _lib.check(rc, "mxk_quantize_mxfp8_t")
    return qt, st


def quantize_mxfp8_dual(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor,
                                                  torch.Tensor]:
    """``(q, s, qt, st)``: ``quantize_mxfp8(x)`` and ``quantize_mxfp8_t(x)`` from
    one read of ``x`` (bf16 ``[R, C]``, both multiples of 32)."""
    _check_xt(x, dual=True)
    if x.device.type == "cpu":
        return quantize_mxfp8_ref(x) + quantize_mxfp8_ref(x.t().contiguous())
    R, C = x.shape
    q = torch.empty((R, C), dtype=torch.float8_e4m3fn, device=x.device)
    s = torch.empty((R, C // BLOCK), dtype=torch.uint8, device=x.device)
    qt = torch.empty((C, R), dtype=torch.float8_e4m3fn, device=x.device)
    st = torch.empty((C, R // BLOCK), dtype=torch.uint8, device=x.device)
    rc = _lib.lib().mxk_quantize_mxfp8_dual(x.data_ptr(), q.data_ptr(), s.data_ptr(), qt.data_ptr(),
                                            st.data_ptr(), R, C, x.stride(0), q.stride(0),
                                            s.stride(0), qt.stride(0), st.stride(0),
                                            _lib.stream_ptr(x.device))
    _lib.check(rc, "mxk_quantize_mxfp8_dual")
    return q, s, qt, st


def _check_pair(q: torch.Tensor, s: torch.Tensor, qn: str, sn: str) -> None:
    if q.dtype != torch.float8_e4m3fn:
        raise TypeError(f"{qn} must be float8_e4m3fn, got {q.dtype}")
    if s.dtype != torch.uint8:
        raise TypeError(f"{sn} must be uint8 (E8M0 bytes), got {s.dtype}")
    if q.dim() != 2 or s.dim() != 2:
        raise ValueError(f"{qn} and {sn} must be 2-D, got {tuple(q.shape)} and {tuple(s.shape)}")
    if q.shape[1] % BLOCK:
        raise ValueError(f"{qn}: K = {q.shape[1]} is not a multiple of {BLOCK}")
    if tuple(s.shape) != (q.shape[0], q.shape[1] // BLOCK):
        raise ValueError(f"{sn} must be [{q.shape[0]}, {q.shape[1] // BLOCK}], "
                         f"got {tuple(s.shape)}")
    if q.shape[1] and (q.stride(1) != 1 or s.stride(1) != 1):
        raise ValueError(f"{qn} and {sn} must be K-contiguous (stride(1) == 1)")
    if q.device != s.device:
        raise ValueError(f"{qn} and {sn} are on different devices")


def dequantize_mxfp8(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """fp32 ``q * 2^(s - 127)`` per block; pure torch, any device."""
    _check_pair(q, s, "q", "s")
    R, K = q.shape
    e = s.to(torch.int32) - 127
    return torch.ldexp(q.float().reshape(R, K // BLOCK, BLOCK), e.unsqueeze(2)).reshape(R, K)


def is_fast_shape_mxfp8(M: int, N: int, K: int) -> bool:
    return M > 0 and N > 0 and K > 0 and M % TILE_M == 0 and N % TILE_N == 0 and K % TILE_K == 0


def _check_layout(q: torch.Tensor, s: torch.Tensor, qn: str, sn: str) -> None:
    # the kernel stages elements in 16-B pieces and a K-tile's 4 scales as one dword
    if q.stride(0) % 16 or q.data_ptr() % 16:
        raise ValueError(f"{qn}: base and row stride must be multiples of 16 bytes")
    if s.stride(0) % 4 or s.data_ptr() % 4:
        raise ValueError(f"{sn}: base and row stride must be multiples of 4 bytes "
                         "(slice K at multiples of 128)")


def gemm_mxfp8_tn(aq: torch.Tensor, a_s: torch.Tensor, bq: torch.Tensor, b_s: torch.Tensor,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """``dequant(aq, a_s) @ dequant(bq, b_s).T`` -> bf16 ``[M, N]``.

    ``aq`` ``[M, K]`` and ``bq`` ``[N, K]`` are e4m3, ``a_s`` / ``b_s`` their
    uint8 scales ``[., K/32]``.  Contract: M and N multiples of 256, K of 128.
    Row strides may exceed the logical widths (views into wider buffers, K
    slices of ``q`` with the matching column slice of ``s``) as long as
    element rows stay 16-byte and scale rows 4-byte aligned."""
    _check_pair(aq, a_s, "aq", "a_s")
    _check_pair(bq, b_s, "bq", "b_s")
    M, K = aq.shape
    N, K2 = bq.shape
    if K != K2:
        raise ValueError(f"K mismatch: aq is {tuple(aq.shape)}, bq is {tuple(bq.shape)}")
    if not is_fast_shape_mxfp8(M, N, K):
        raise ValueError(f"gemm_mxfp8_tn needs M % {TILE_M} == 0, N % {TILE_N} == 0 and "
                         f"K % {TILE_K} == 0 (all positive), got M={M} N={N} K={K}")
    if aq.device != bq.device:
        raise ValueError("aq and bq are on different devices")
    if out is not None:
        if out.dtype != torch.bfloat16:
            raise TypeError(f"out must be bfloat16, got {out.dtype}")
        if out.dim() != 2 or tuple(out.shape) != (M, N):
            raise ValueError(f"out must be [{M}, {N}]")
        if out.stride(1) != 1:
            raise ValueError("out must be row-major (stride(1) == 1)")
        if out.device != aq.device:
            raise ValueError("out is on a different device")
    if aq.device.type == "cpu":
        ref = (dequantize_mxfp8(aq, a_s) @ dequantize_mxfp8(bq, b_s).t()).to(torch.bfloat16)
        if out is not None:
            out.copy_(ref)
            return out
        return ref
    _check_layout(aq, a_s, "aq", "a_s")
    _check_layout(bq, b_s, "bq", "b_s")
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=aq.device)
    elif out.stride(0) % 8 or out.data_ptr() % 16:
        raise ValueError("out: base must be 16-byte aligned and the row stride a multiple of 8")
    st = _lib.lib().mxk_gemm_mxfp8_tn(aq.data_ptr(), a_s.data_ptr(), bq.data_ptr(), b_s.data_ptr(),
                                      out.data_ptr(), M, N, K, aq.stride(0), a_s.stride(0),
                                      bq.stride(0), b_s.stride(0), out.stride(0),
                                      _lib.stream_ptr(aq.device))
    _lib.check(st, "mxk_gemm_mxfp8_tn")
    return out
