"""MXFP4 quantiser and block-scaled MFMA GEMM op (``native/kernels/gemm_mxfp4.hip``).

The format is OCP MX with e2m1 elements, blocks of 32 consecutive K elements
and one E8M0 scale byte per block:

====== ============= ==================================================
tensor shape         storage
====== ============= ==================================================
``x``  ``[R, K]``    bf16, ``K % 32 == 0``
``q``  ``[R, K/2]``  ``torch.uint8``: element ``2i`` in bits 3:0 of byte
                     ``i``, element ``2i+1`` in bits 7:4 (the packing of
                     ``torch.float4_e2m1fn_x2``, so ``.view()`` works)
``s``  ``[R, K/32]`` ``torch.uint8``, row-major
====== ============= ==================================================

e2m1 codes 0..7 are the magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6; bit 3 is the
sign.  Per block: ``amax = max |x|`` in fp32, ``e = floor(log2(amax)) - 2`` (2
is the emax of e2m1), scale byte ``clamp(e, -127, 127) + 127`` (127 for an
all-zero block), element ``RNE_to_e2m1(clamp(x * 2^-e, -6, 6))``: the
saturation is explicit, ties go to the even code and -0 (code 8) is never
produced.  Only finite inputs are in scope.

``gemm_mxfp4_tn(aq, a_s, bq, b_s)`` computes ``dequant(a) @ dequant(b).T`` with
fp32 accumulation and bf16 output on ``v_mfma_scale_f32_32x32x64_f8f6f4``
(e2m1 operands).  The product of the *dequantised* operands is the reference
of every check: scaled block maxima land in [4, 8) and everything above 5
becomes 6, so against the unquantised bf16 product the format's own error is
about 21 % for uniform data.

GPU tensors always run the hand-written kernels (no fallback); CPU tensors
take the pure-torch reference path.
"""
from __future__ import annotations

import torch

from . import _lib

BLOCK = 32          # elements per scale
E2M1_MAX = 6.0
E2M1_EMAX = 2
TILE_M = TILE_N = 256
TILE_K = 256

# magnitude of code 0..7
_E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
# midpoints of neighbouring magnitudes; a tie goes to the even code, so the
# midpoint itself counts only where the upper neighbour is even
_E2M1_MIDPOINTS = ((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False),
                   (3.5, True), (5.0, False))


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


def _to_e2m1(y: torch.Tensor) -> torch.Tensor:
    """fp32 with |y| <= 6 -> uint8 e2m1 codes (sign in bit 3), RNE, ties to the
    even code; what rounds to zero is code 0 whatever its sign."""
    a = y.abs()
    code = torch.zeros_like(a, dtype=torch.uint8)
    for mid, inclusive in _E2M1_MIDPOINTS:
        code += ((a >= mid) if inclusive else (a > mid)).to(torch.uint8)
    return code | ((torch.signbit(y) & (code != 0)).to(torch.uint8) << 3)


def quantize_mxfp4_ref(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Pure-torch MXFP4 quantiser (any device): the definition the kernel is
    bit-identical to.  Finite inputs only."""
    _check_x(x)
    R, K = x.shape
    xb = x.float().reshape(R, K // BLOCK, BLOCK)
    amax = xb.abs().amax(dim=2)
    _, ex = torch.frexp(amax)                     # amax = m 2^ex, m in [0.5, 1)
    e = (ex.to(torch.int32) - 1 - E2M1_EMAX).clamp(-127, 127)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    y = torch.ldexp(xb, -e.unsqueeze(2)).clamp(-E2M1_MAX, E2M1_MAX)
    code = _to_e2m1(y).reshape(R, K // 2, 2)
    q = code[:, :, 0] | (code[:, :, 1] << 4)
    s = (e + 127).to(torch.uint8)
    return q.contiguous(), s


def quantize_mxfp4(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """bf16 ``[R, K]`` -> (packed e2m1 uint8 ``[R, K/2]``, uint8 E8M0 scales
    ``[R, K/32]``).  Finite inputs only.  A row stride larger than K is fine."""
    _check_x(x)
    if x.device.type == "cpu":
        return quantize_mxfp4_ref(x)
    R, K = x.shape
    q = torch.empty((R, K // 2), dtype=torch.uint8, device=x.device)
    s = torch.empty((R, K // BLOCK), dtype=torch.uint8, device=x.device)
    st = _lib.lib().mxk_quantize_mxfp4(x.data_ptr(), q.data_ptr(), s.data_ptr(), R, K, x.stride(0),
                                       q.stride(0), s.stride(0), _lib.stream_ptr(x.device))
    _lib.check(st, "mxk_quantize_mxfp4")
    return q, s


def _check_pair(q: torch.Tensor, s: torch.Tensor, qn: str, sn: str) -> None:
    if q.dtype != torch.uint8:
        raise TypeError(f"{qn} must be uint8 (two e2m1 codes per byte), got {q.dtype}")
    if s.dtype != torch.uint8:
        raise TypeError(f"{sn} must be uint8 (E8M0 bytes), got {s.dtype}")
    if q.dim() != 2 or s.dim() != 2:
        raise ValueError(f"{qn} and {sn} must be 2-D, got {tuple(q.shape)} and {tuple(s.shape)}")
    K = 2 * q.shape[1]
    if K % BLOCK:
        raise ValueError(f"{qn}: K = {K} is not a multiple of {BLOCK}")
    if tuple(s.shape) != (q.shape[0], K // BLOCK):
        raise ValueError(f"{sn} must be [{q.shape[0]}, {K // BLOCK}], got {tuple(s.shape)}")
    if K and (q.stride(1) != 1 or s.stride(1) != 1):
        raise ValueError(f"{qn} and {sn} must be K-contiguous (stride(1) == 1)")
    if q.device != s.device:
        raise ValueError(f"{qn} and {sn} are on different devices")


def dequantize_mxfp4(q: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """fp32 ``e2m1(q) * 2^(s - 127)`` per block ``[R, K]``; pure torch, any device."""
    _check_pair(q, s, "q", "s")
    R, K = q.shape[0], 2 * q.shape[1]
    code = torch.stack((q & 0xF, q >> 4), dim=2).reshape(R, K).to(torch.int64)
    table = torch.tensor(_E2M1_VALUES + tuple(-v for v in _E2M1_VALUES), dtype=torch.float32,
                         device=q.device)
    e = s.to(torch.int32) - 127
    return torch.ldexp(table[code].reshape(R, K // BLOCK, BLOCK), e.unsqueeze(2)).reshape(R, K)


def is_fast_shape_mxfp4(M: int, N: int, K: int) -> bool:
    return M > 0 and N > 0 and K > 0 and M % TILE_M == 0 and N % TILE_N == 0 and K % TILE_K == 0


def _check_layout(q: torch.Tensor, s: torch.Tensor, qn: str, sn: str) -> None:
    # the kernel stages elements in 16-B pieces and a K-tile's 8 scales as two dwords
    if q.stride(0) % 16 or q.data_ptr() % 16:
        raise ValueError(f"{qn}: base and row stride must be multiples of 16 bytes")
    if s.stride(0) % 4 or s.data_ptr() % 4:
        raise ValueError(f"{sn}: base and row stride must be multiples of 4 bytes "
                         "(slice K at multiples of 256)")


def gemm_mxfp4_tn(aq: torch.Tensor, a_s: torch.Tensor, bq: torch.Tensor, b_s: torch.Tensor,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """``dequant(aq, a_s) @ dequant(bq, b_s).T`` -> bf16 ``[M, N]``.

    ``aq`` ``[M, K/2]`` and ``bq`` ``[N, K/2]`` are packed e2m1 (uint8), ``a_s``
    / ``b_s`` their uint8 scales ``[., K/32]``.  Contract: M, N and K multiples
    of 256.  Row strides may exceed the logical widths (views into wider
    buffers, K slices of ``q`` with the matching column slice of ``s``) as
    long as element rows stay 16-byte and scale rows 4-byte aligned."""
    _check_pair(aq, a_s, "aq", "a_s")
    _check_pair(bq, b_s, "bq", "b_s")
    M, K = aq.shape[0], 2 * aq.shape[1]
    N, K2 = bq.shape[0], 2 * bq.shape[1]
    if K != K2:
        raise ValueError(f"K mismatch: aq holds K = {K}, bq K = {K2}")
    if not is_fast_shape_mxfp4(M, N, K):
        raise ValueError(f"gemm_mxfp4_tn needs M % {TILE_M} == 0, N % {TILE_N} == 0 and "
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
        ref = (dequantize_mxfp4(aq, a_s) @ dequantize_mxfp4(bq, b_s).t()).to(torch.bfloat16)
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
    st = _lib.lib().mxk_gemm_mxfp4_tn(aq.data_ptr(), a_s.data_ptr(), bq.data_ptr(), b_s.data_ptr(),
                                      out.data_ptr(), M, N, K, aq.stride(0), a_s.stride(0),
                                      bq.stride(0), b_s.stride(0), out.stride(0),
                                      _lib.stream_ptr(aq.device))
    _lib.check(st, "mxk_gemm_mxfp4_tn")
    return out
