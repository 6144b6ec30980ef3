"""What the block-scaled (OCP MX) ops share: ``mxfp8.py`` and ``mxfp4.py`` keep
their docstrings, constants and element codecs and call into here."""
from __future__ import annotations

from typing import Callable

import torch

from . import _lib

BLOCK = 32          # elements per scale
TILE_M = TILE_N = 256


def check_x(x: torch.Tensor) -> None:
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


def check_xt(x: torch.Tensor, dual: bool) -> None:
    """The argument of a transposing quantiser: blocks of 32 along the rows."""
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


def block_exponent(xb: torch.Tensor, emax: int) -> torch.Tensor:
    """``xb`` fp32 ``[R, K/32, 32]`` -> int32 ``[R, K/32]``: ``floor(log2(amax)) -
    emax`` clamped to [-127, 127], 0 for an all-zero block."""
    amax = xb.abs().amax(dim=2)
    _, ex = torch.frexp(amax)                     # amax = m 2^ex, m in [0.5, 1)
    e = (ex.to(torch.int32) - 1 - emax).clamp(-127, 127)
    return torch.where(amax == 0, torch.zeros_like(e), e)


def _images(x: torch.Tensor, per_byte: int, dtype: torch.dtype, transposed: bool):
    """Uninitialised (codes, scales) of ``x`` ``[R, C]`` or of its transpose."""
    R, C = x.shape[::-1] if transposed else x.shape
    return (torch.empty((R, C // per_byte), dtype=dtype, device=x.device),
            torch.empty((R, C // BLOCK), dtype=torch.uint8, device=x.device))


def _sr(seed):
    """(entry-point infix, reference arguments, arguments before the stream) of
    a quantiser call: nearest rounding for ``seed`` None, else stochastic
    rounding with that seed (the entry points ``mxk_quantize_<name>_sr*``)."""
    return ("", (), ()) if seed is None else ("_sr", ("stochastic", seed), (seed,))


def quantize_rows(name: str, per_byte: int, dtype: torch.dtype, ref: Callable, x: torch.Tensor,
                  seed: int | None = None):
    """``quantize_<name>``: ``per_byte`` codes in each ``dtype`` item of ``q``,
    ``ref`` the format's pure-torch quantiser, the kernel ``mxk_quantize_<name>``."""
    check_x(x)
    sr, ref_args, seed_arg = _sr(seed)
    if x.device.type == "cpu":
        return ref(x, *ref_args)
    R, K = x.shape
    q, s = _images(x, per_byte, dtype, False)
    fn = f"mxk_quantize_{name}{sr}"
    rc = getattr(_lib.lib(), fn)(x.data_ptr(), q.data_ptr(), s.data_ptr(), R, K, x.stride(0),
                                 q.stride(0), s.stride(0), *seed_arg, _lib.stream_ptr(x.device))
    _lib.check(rc, fn)
    return q, s


def quantize_t(name: str, per_byte: int, dtype: torch.dtype, ref: Callable, x: torch.Tensor,
               seed: int | None = None):
    """``quantize_<name>_t``: the images of ``x.t()``; the kernel ``mxk_quantize_<name>_t``."""
    check_xt(x, dual=False)
    sr, ref_args, seed_arg = _sr(seed)
    if x.device.type == "cpu":
        return ref(x.t().contiguous(), *ref_args)
    R, C = x.shape
    qt, st = _images(x, per_byte, dtype, True)
    fn = f"mxk_quantize_{name}{sr}_t"
    rc = getattr(_lib.lib(), fn)(x.data_ptr(), qt.data_ptr(), st.data_ptr(), R, C, x.stride(0),
                                 qt.stride(0), st.stride(0), *seed_arg, _lib.stream_ptr(x.device))
    _lib.check(rc, fn)
    return qt, st


def quantize_dual(name: str, per_byte: int, dtype: torch.dtype, ref: Callable, x: torch.Tensor,
                  seed: int | None = None):
    """``quantize_<name>_dual``: both images from one read of ``x``; the kernel
    ``mxk_quantize_<name>_dual``.  Stochastic: the transposed image draws with
    ``seed + 1`` (mod 2^64)."""
    check_xt(x, dual=True)
    sr, ref_args, seed_arg = _sr(seed)
    if x.device.type == "cpu":
        if seed is None:
            return ref(x) + ref(x.t().contiguous())
        return ref(x, *ref_args) + ref(x.t().contiguous(), "stochastic", (seed + 1) % 2 ** 64)
    R, C = x.shape
    q, s = _images(x, per_byte, dtype, False)
    qt, st = _images(x, per_byte, dtype, True)
    fn = f"mxk_quantize_{name}{sr}_dual"
    rc = getattr(_lib.lib(), fn)(x.data_ptr(), q.data_ptr(), s.data_ptr(), qt.data_ptr(), st.data_ptr(),
                                 R, C, x.stride(0), q.stride(0), s.stride(0), qt.stride(0),
                                 st.stride(0), *seed_arg, _lib.stream_ptr(x.device))
    _lib.check(rc, fn)
    return q, s, qt, st


# ---- SwiGLU inside the quantisers (native/kernels/swiglu_quantize_mx.hip) ---------
# gu = [g | u] is [T, 2F]; the images are those of h = silu(g) * u [T, F] or of
# dgu = [dg | du] [T, 2F].  The kernels take 16-B aligned rows only; every other
# tensor (CPU tensors among them) gets the composition of the stand-alone ops,
# which the kernels equal bit for bit on the GPU.
_TR_MAX_F = 64 * 65535          # grid.y of the transposing kernels


def check_gu(gu: torch.Tensor, rows32: bool, dh=None, with_dh: bool = False) -> None:
    """The argument of a fused SwiGLU quantiser, [T, 2F]; with_dh: and dh [T, F]."""
    if not isinstance(gu, torch.Tensor):
        raise TypeError("gu must be a tensor")
    if gu.dtype != torch.bfloat16:
        raise TypeError(f"gu must be bfloat16, got {gu.dtype}")
    if gu.dim() != 2:
        raise ValueError(f"gu must be 2-D, got shape {tuple(gu.shape)}")
    T, F2 = gu.shape
    if T == 0 or F2 == 0 or F2 % (2 * BLOCK) or (rows32 and T % BLOCK):
        raise ValueError(f"gu must be [T, 2F] with F a positive multiple of {BLOCK} and T "
                         + (f"a positive multiple of {BLOCK}" if rows32 else "> 0")
                         + f", got {tuple(gu.shape)}")
    if gu.stride(1) != 1:
        raise ValueError("gu must be row-major (stride(1) == 1)")
    if not with_dh:
        return
    if not isinstance(dh, torch.Tensor):
        raise TypeError("dh must be a tensor")
    if dh.dtype != torch.bfloat16:
        raise TypeError(f"dh must be bfloat16, got {dh.dtype}")
    if dh.dim() != 2 or tuple(dh.shape) != (T, F2 // 2):
        raise ValueError(f"dh must be [{T}, {F2 // 2}], got {tuple(dh.shape)}")
    if dh.stride(1) != 1:
        raise ValueError("dh must be row-major (stride(1) == 1)")
    if dh.device != gu.device:
        raise ValueError("gu and dh are on different devices")


def _swiglu_h(gu: torch.Tensor) -> torch.Tensor:
    from .fused import swiglu_fwd, swiglu_ref
    return swiglu_ref(gu) if gu.device.type == "cpu" else swiglu_fwd(gu)


def _swiglu_dgu(gu: torch.Tensor, dh: torch.Tensor) -> torch.Tensor:
    from .fused import swiglu_bwd, swiglu_bwd_ref
    return swiglu_bwd_ref(gu, dh) if gu.device.type == "cpu" else swiglu_bwd(gu, dh)


def _ld(t: torch.Tensor) -> int:
    """The row stride handed to a kernel: that of a single row is never used and
    may be anything in torch, so its width stands for it."""
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _kernel_takes(*tensors: torch.Tensor) -> bool:
    """GPU tensors with 16-B aligned rows that do not overlap (the fused kernels
    have no by-element form, and refuse a row stride below the width, such as
    an expanded tensor's 0)."""
    return all(t.is_cuda and t.data_ptr() % 16 == 0 and _ld(t) % 8 == 0 and _ld(t) >= t.shape[1]
               for t in tensors)


def swiglu_quantize_rows(name: str, per_byte: int, dtype: torch.dtype, quantize: Callable,
                         gu: torch.Tensor):
    """``swiglu_quantize_<name>``: ``quantize`` is the format's ``quantize_<name>``."""
    check_gu(gu, rows32=False)
    if not _kernel_takes(gu):
        return quantize(_swiglu_h(gu))
    T, F = gu.shape[0], gu.shape[1] // 2
    q = torch.empty((T, F // per_byte), dtype=dtype, device=gu.device)
    s = torch.empty((T, F // BLOCK), dtype=torch.uint8, device=gu.device)
    fn = f"mxk_swiglu_quantize_{name}"
    rc = getattr(_lib.lib(), fn)(gu.data_ptr(), q.data_ptr(), s.data_ptr(), T, F, _ld(gu),
                                 q.stride(0), s.stride(0), _lib.stream_ptr(gu.device))
    _lib.check(rc, fn)
    return q, s


def swiglu_quantize_t(name: str, per_byte: int, dtype: torch.dtype, quantize_t: Callable,
                      gu: torch.Tensor):
    """``swiglu_quantize_<name>_t``: ``quantize_t`` is the format's ``quantize_<name>_t``."""
    check_gu(gu, rows32=True)
    T, F = gu.shape[0], gu.shape[1] // 2
    if not _kernel_takes(gu) or F > _TR_MAX_F:
        return quantize_t(_swiglu_h(gu))
    qt = torch.empty((F, T // per_byte), dtype=dtype, device=gu.device)
    st = torch.empty((F, T // BLOCK), dtype=torch.uint8, device=gu.device)
    fn = f"mxk_swiglu_quantize_{name}_t"
    rc = getattr(_lib.lib(), fn)(gu.data_ptr(), qt.data_ptr(), st.data_ptr(), T, F, _ld(gu),
                                 qt.stride(0), st.stride(0), _lib.stream_ptr(gu.device))
    _lib.check(rc, fn)
    return qt, st


def swiglu_bwd_quantize_dual(name: str, per_byte: int, dtype: torch.dtype, quantize_dual: Callable,
                             gu: torch.Tensor, dh: torch.Tensor, seed: int | None = None):
    """``swiglu_bwd_quantize_<name>_dual``: ``quantize_dual`` is the format's
    ``quantize_<name>_dual``; a ``seed`` selects stochastic rounding."""
    check_gu(gu, rows32=True, dh=dh, with_dh=True)
    sr, ref_args, seed_arg = _sr(seed)
    T, F = gu.shape[0], gu.shape[1] // 2
    if not _kernel_takes(gu, dh) or F > _TR_MAX_F or (seed is not None and max(T, 2 * F) >= 2 ** 32):
        return quantize_dual(_swiglu_dgu(gu, dh), *ref_args)
    q = torch.empty((T, 2 * F // per_byte), dtype=dtype, device=gu.device)
    s = torch.empty((T, 2 * F // BLOCK), dtype=torch.uint8, device=gu.device)
    qt = torch.empty((2 * F, T // per_byte), dtype=dtype, device=gu.device)
    st = torch.empty((2 * F, T // BLOCK), dtype=torch.uint8, device=gu.device)
    fn = f"mxk_swiglu_bwd_quantize_{name}{sr}_dual"
    rc = getattr(_lib.lib(), fn)(gu.data_ptr(), dh.data_ptr(), q.data_ptr(), s.data_ptr(),
                                 qt.data_ptr(), st.data_ptr(), T, F, _ld(gu), _ld(dh),
                                 q.stride(0), s.stride(0), qt.stride(0), st.stride(0), *seed_arg,
                                 _lib.stream_ptr(gu.device))
    _lib.check(rc, fn)
    return q, s, qt, st


def check_pair(q: torch.Tensor, s: torch.Tensor, qn: str, sn: str, dtype: torch.dtype, wording: str,
               per_byte: int) -> None:
    """``q`` holds ``per_byte`` elements in each item of ``dtype``; ``wording``
    names that dtype in the error."""
    if q.dtype != dtype:
        raise TypeError(f"{qn} must be {wording}, got {q.dtype}")
    if s.dtype != torch.uint8:
        raise TypeError(f"{sn} must be uint8 (E8M0 bytes), got {s.dtype}")
    if q.dim() != 2 or s.dim() != 2:
        raise ValueError(f"{qn} and {sn} must be 2-D, got {tuple(q.shape)} and {tuple(s.shape)}")
    K = per_byte * q.shape[1]
    if K % BLOCK:
        raise ValueError(f"{qn}: K = {K} is not a multiple of {BLOCK}")
    if tuple(s.shape) != (q.shape[0], K // BLOCK):
        raise ValueError(f"{sn} must be [{q.shape[0]}, {K // BLOCK}], got {tuple(s.shape)}")
    if K and (q.stride(1) != 1 or s.stride(1) != 1):
        raise ValueError(f"{qn} and {sn} must be K-contiguous (stride(1) == 1)")
    if q.device != s.device:
        raise ValueError(f"{qn} and {sn} are on different devices")


def is_fast_shape(M: int, N: int, K: int, tile_k: int) -> bool:
    return M > 0 and N > 0 and K > 0 and M % TILE_M == 0 and N % TILE_N == 0 and K % tile_k == 0


def check_layout(q: torch.Tensor, s: torch.Tensor, qn: str, sn: str, tile_k: int) -> None:
    # the kernel stages elements in 16-B pieces and 4 scales as one dword
    if q.stride(0) % 16 or q.data_ptr() % 16:
        raise ValueError(f"{qn}: base and row stride must be multiples of 16 bytes")
    if s.stride(0) % 4 or s.data_ptr() % 4:
        raise ValueError(f"{sn}: base and row stride must be multiples of 4 bytes "
                         f"(slice K at multiples of {tile_k})")


def gemm_tn(name: str, tile_k: int, per_byte: int, check: Callable, dequantize: Callable,
            aq: torch.Tensor, a_s: torch.Tensor, bq: torch.Tensor, b_s: torch.Tensor,
            out: torch.Tensor | None) -> torch.Tensor:
    """``gemm_<name>_tn``: ``check(q, s, qn, sn)`` is the format's pair check,
    ``dequantize`` its reference, the kernel ``mxk_gemm_<name>_tn``."""
    check(aq, a_s, "aq", "a_s")
    check(bq, b_s, "bq", "b_s")
    M, K = aq.shape[0], per_byte * aq.shape[1]
    N, K2 = bq.shape[0], per_byte * bq.shape[1]
    if K != K2:
        raise ValueError(f"K mismatch: aq holds K = {K}, bq K = {K2}")
    if not is_fast_shape(M, N, K, tile_k):
        raise ValueError(f"gemm_{name}_tn needs M % {TILE_M} == 0, N % {TILE_N} == 0 and "
                         f"K % {tile_k} == 0 (all positive), got M={M} N={N} K={K}")
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
        ref = (dequantize(aq, a_s) @ dequantize(bq, b_s).t()).to(torch.bfloat16)
        if out is not None:
            out.copy_(ref)
            return out
        return ref
    check_layout(aq, a_s, "aq", "a_s", tile_k)
    check_layout(bq, b_s, "bq", "b_s", tile_k)
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=aq.device)
    elif out.stride(0) % 8 or out.data_ptr() % 16:
        raise ValueError("out: base must be 16-byte aligned and the row stride a multiple of 8")
    fn = f"mxk_gemm_{name}_tn"
    st = getattr(_lib.lib(), fn)(aq.data_ptr(), a_s.data_ptr(), bq.data_ptr(), b_s.data_ptr(),
                                 out.data_ptr(), M, N, K, aq.stride(0), a_s.stride(0), bq.stride(0),
                                 b_s.stride(0), out.stride(0), _lib.stream_ptr(aq.device))
    _lib.check(st, fn)
    return out
