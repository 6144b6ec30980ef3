"""MXFP4 quantisers and block-scaled MFMA GEMM op (``native/kernels/gemm_mxfp4.hip``;
the quantiser kernels are the templates of ``native/kernels/mx_quantize.h``, shared
with MXFP8).

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

``quantize_mxfp4_t(x)`` and ``quantize_mxfp4_dual(x)`` give the images of the
transposed tensor, whose blocks are 32 consecutive *rows* of ``x`` and whose
bytes hold two row-neighbours, without a transposed copy: what the backward
products of a linear layer contract over
(``mxk8s.ops.linear.linear_mxfp4``).

Stochastic rounding (``rounding="stochastic", seed=s`` on the four quantisers;
the kernels of ``native/kernels/quantize_mxfp4_sr.hip``) is for gradients:
round-to-nearest shrinks every block (the clamp at 6 of scaled maxima in
[4, 8)), stochastic rounding with a scale that does not clip is unbiased.  The
images are ordinary MXFP4.  Definition, the same bit for bit in the host C++,
the kernels and the reference here:

* block exponent ``e_sr = e + 1`` where ``amax * 2^-e > 6``, else ``e``: scaled
  maxima land in (3, 6] and nothing is clamped;
* element ``8g + j`` of row ``i`` of the *output image* (so ``quantize_mxfp4_t``
  still equals ``quantize_mxfp4`` of the transposed copy) takes the 16 bits
  ``u = (word[j >> 1] >> 16 (j & 1)) & 0xffff`` of Philox4x32-10 with counter
  ``(g, i, 0, 0)`` and key ``(seed & 0xffffffff, seed >> 32)``; with ``lo`` the
  largest e2m1 magnitude ``<= a = |x * 2^-e_sr|`` (code ``c``) and ``gap`` the
  distance to the next one, the code is ``c + (u < (a - lo) / gap * 65536)``, so
  ``E[dequant] = x`` to within ``gap * 2^(e_sr - 16)``; sign as above;
* ``quantize_mxfp4_dual(x, "stochastic", s)`` is ``quantize_mxfp4(x, .., s)`` and
  ``quantize_mxfp4_t(x, .., (s + 1) mod 2^64)``: independent noise in the two
  images.

The generator is counter-based and stateless, so a ``(seed, element)`` pair
always gets the same bits.  ``sr_reseed`` / ``sr_next`` hand out seeds.

GPU tensors always run the hand-written kernels (no fallback); CPU tensors
take the pure-torch reference path.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _mx
from ._philox import philox4x32_10
from ._mx import BLOCK, TILE_M, TILE_N  # noqa: F401  (this module's constants, as before)

E2M1_MAX = 6.0
E2M1_EMAX = 2
TILE_K = 256

# magnitude of code 0..7
_E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
# midpoints of neighbouring magnitudes; a tie goes to the even code, so the
# midpoint itself counts only where the upper neighbour is even
_E2M1_MIDPOINTS = ((0.25, False), (0.75, True), (1.25, False), (1.75, True), (2.5, False),
                   (3.5, True), (5.0, False))


def _to_e2m1(y: torch.Tensor) -> torch.Tensor:
    """fp32 with |y| <= 6 -> uint8 e2m1 codes (sign in bit 3), RNE, ties to the
    even code; what rounds to zero is code 0 whatever its sign."""
    a = y.abs()
    code = torch.zeros_like(a, dtype=torch.uint8)
    for mid, inclusive in _E2M1_MIDPOINTS:
        code += ((a >= mid) if inclusive else (a > mid)).to(torch.uint8)
    return code | ((torch.signbit(y) & (code != 0)).to(torch.uint8) << 3)


ROUNDINGS = ("nearest", "stochastic")


def check_rounding(rounding, seed) -> int | None:
    """The seed of a stochastic call, None for ``"nearest"``; ``ValueError`` for
    an unknown rounding, a stochastic call without an int seed in [0, 2^64) and
    a seed without stochastic rounding."""
    if rounding not in ROUNDINGS:
        raise ValueError(f"rounding must be one of {ROUNDINGS}, got {rounding!r}")
    if rounding == "nearest":
        if seed is not None:
            raise ValueError("seed is only taken with rounding=\"stochastic\"")
        return None
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"rounding=\"stochastic\" needs an int seed in [0, 2^64), got {seed!r}")
    return seed


def _sr_bits(R: int, K: int, seed: int) -> torch.Tensor:
    """int32 ``[R, K]``: the 16 random bits of every element of an image (host)."""
    g = np.arange(K // 8, dtype=np.uint64)[None, :]
    i = np.arange(R, dtype=np.uint64)[:, None]
    w = philox4x32_10((g, i, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))            # [R, K/8, 4]
    u = np.stack((w & np.uint32(0xFFFF), w >> np.uint32(16)), axis=-1)           # word j >> 1, half j & 1
    return torch.from_numpy(u.reshape(R, K).astype(np.int32))


def _to_e2m1_sr(y: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """fp32 with |y| <= 6 and 16 random bits each -> uint8 e2m1 codes: one of
    the two neighbours, the upper one where u < (|y| - lo) / gap * 65536 (every
    step exact in fp32)."""
    a = y.abs()
    c = torch.zeros_like(a, dtype=torch.int64)
    for v in _E2M1_VALUES[1:]:
        c += (a >= v).to(torch.int64)
    mags = torch.tensor(_E2M1_VALUES + (8.0,), dtype=torch.float32, device=y.device)   # code 7 has no upper neighbour
    lo = mags[c]
    t = (a - lo) / (mags[c + 1] - lo) * 65536.0
    code = torch.where(c == 7, c, c + (u.to(torch.float32) < t).to(torch.int64)).to(torch.uint8)
    return code | ((torch.signbit(y) & (code != 0)).to(torch.uint8) << 3)


def quantize_mxfp4_ref(x: torch.Tensor, rounding: str = "nearest",
                       seed: int | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """Pure-torch MXFP4 quantiser (any device): the definition the kernel is
    bit-identical to.  Finite inputs only.  ``rounding="stochastic"`` with a
    ``seed``: the module docstring has the definition (the random bits are
    drawn on the host)."""
    seed = check_rounding(rounding, seed)
    _mx.check_x(x)
    R, K = x.shape
    xb = x.float().reshape(R, K // BLOCK, BLOCK)
    e = _mx.block_exponent(xb, E2M1_EMAX)
    if seed is None:
        y = torch.ldexp(xb, -e.unsqueeze(2)).clamp(-E2M1_MAX, E2M1_MAX)
        code = _to_e2m1(y)
    else:
        e = e + (torch.ldexp(xb.abs().amax(dim=2), -e) > E2M1_MAX).to(e.dtype)   # exact; e <= 125 before
        y = torch.ldexp(xb, -e.unsqueeze(2))                                     # |y| <= 6
        code = _to_e2m1_sr(y.reshape(R, K), _sr_bits(R, K, seed).to(x.device))
    code = code.reshape(R, K // 2, 2)
    q = code[:, :, 0] | (code[:, :, 1] << 4)
    s = (e + 127).to(torch.uint8)
    return q.contiguous(), s


def quantize_mxfp4(x: torch.Tensor, rounding: str = "nearest",
                   seed: int | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """bf16 ``[R, K]`` -> (packed e2m1 uint8 ``[R, K/2]``, uint8 E8M0 scales
    ``[R, K/32]``).  Finite inputs only.  A row stride larger than K is fine.
    ``rounding="stochastic"`` needs an int ``seed`` in [0, 2^64)."""
    return _mx.quantize_rows("mxfp4", 2, torch.uint8, quantize_mxfp4_ref, x,
                             check_rounding(rounding, seed))


def quantize_mxfp4_t(x: torch.Tensor, rounding: str = "nearest",
                     seed: int | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """bf16 ``[R, C]`` -> (packed e2m1 uint8 ``[C, R/2]``, uint8 E8M0 scales
    ``[C, R/32]``): the images of ``quantize_mxfp4(x.t().contiguous())``, bit for
    bit, from one pass over ``x``.  The MX blocks are 32 consecutive *rows* of
    ``x`` (``R % 32 == 0``; any ``C``) and byte ``i`` of row ``c`` holds
    ``x[2i, c]`` in bits 3:0 and ``x[2i+1, c]`` in bits 7:4, which is what a
    product contracting over the row axis of ``x`` needs.  Finite inputs only.
    A row stride larger than C is fine.  Stochastic rounding draws by the
    coordinates of the output image, so the identity holds for it too."""
    return _mx.quantize_t("mxfp4", 2, torch.uint8, quantize_mxfp4_ref, x,
                          check_rounding(rounding, seed))


def quantize_mxfp4_dual(x: torch.Tensor, rounding: str = "nearest",
                        seed: int | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor,
                                                          torch.Tensor]:
    """``(q, s, qt, st)``: ``quantize_mxfp4(x)`` and ``quantize_mxfp4_t(x)`` from
    one read of ``x`` (bf16 ``[R, C]``, both multiples of 32).  Stochastic:
    ``quantize_mxfp4(x, .., seed)`` and ``quantize_mxfp4_t(x, .., (seed + 1) mod
    2^64)``."""
    return _mx.quantize_dual("mxfp4", 2, torch.uint8, quantize_mxfp4_ref, x,
                             check_rounding(rounding, seed))


def swiglu_quantize_mxfp4(gu: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``quantize_mxfp4(h)`` of ``h = silu(g) * u`` for bf16 ``gu = [g | u]``
    ``[T, 2F]`` (``F % 32 == 0``), bit for bit, without ``h`` in memory: one kernel
    (``native/kernels/swiglu_quantize_mx.hip``) for GPU tensors with 16-byte
    aligned rows, the composition of the two ops for every other tensor."""
    return _mx.swiglu_quantize_rows("mxfp4", 2, torch.uint8, quantize_mxfp4, gu)


def swiglu_quantize_mxfp4_t(gu: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``quantize_mxfp4_t(h)`` of ``h = silu(g) * u`` (``T % 32 == 0`` as well); see
    :func:`swiglu_quantize_mxfp4`."""
    return _mx.swiglu_quantize_t("mxfp4", 2, torch.uint8, quantize_mxfp4_t, gu)


def swiglu_bwd_quantize_mxfp4_dual(gu: torch.Tensor, dh: torch.Tensor, rounding: str = "nearest",
                                   seed: int | None = None):
    """``quantize_mxfp4_dual(dgu, rounding, seed)`` of the SwiGLU gradient ``dgu =
    [dg | du]`` ``[T, 2F]`` for ``gu`` ``[T, 2F]`` and ``dh`` ``[T, F]`` (bf16, ``T``
    and ``F`` multiples of 32), bit for bit, from one read of ``gu`` and ``dh`` and
    without ``dgu`` in memory.  Stochastic rounding draws by the coordinates of
    ``dgu``'s images, the row image with ``seed`` and the transposed one with
    ``seed + 1``; see :func:`swiglu_quantize_mxfp4`."""
    return _mx.swiglu_bwd_quantize_dual("mxfp4", 2, torch.uint8, quantize_mxfp4_dual, gu, dh,
                                        check_rounding(rounding, seed))


# ---- seeds of the stochastic gradient quantisers ---------------------------------
# One seed per linear_mxfp4 call (mxk8s.ops.linear): the n-th draw after
# sr_reseed(seed, rank, step) is ((w1 << 32) | w0) & ~1 with w0, w1 the first
# two words of Philox4x32-10(counter (n, step & 0xffffffff, step >> 32, rank),
# key of seed).  Bit 0 is cleared so that the seed + 1 of a dual call is never
# another call's seed.
_sr_state = {"seed": 0, "rank": 0, "step": 0, "n": 0}


def sr_reseed(seed: int, rank: int = 0, step: int = 0) -> None:
    """Restart the seed source: ``seed`` and ``step`` in [0, 2^64), ``rank`` in
    [0, 2^32).  A trainer reseeds before every step with its global step, so a
    resumed run draws what the uninterrupted one drew."""
    for name, v, bits in (("seed", seed, 64), ("rank", rank, 32), ("step", step, 64)):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** bits:
            raise ValueError(f"{name} must be an int in [0, 2^{bits}), got {v!r}")
    _sr_state.update(seed=seed, rank=rank, step=step, n=0)


def sr_next() -> int:
    """The next seed (even, in [0, 2^64)); before any ``sr_reseed`` the source is
    in the state of ``sr_reseed(0, 0, 0)``."""
    st = _sr_state
    if st["n"] >= 2 ** 32:
        raise RuntimeError("2^32 seeds drawn since the last sr_reseed")
    w = philox4x32_10((st["n"], st["step"] & 0xFFFFFFFF, st["step"] >> 32, st["rank"]),
                      (st["seed"] & 0xFFFFFFFF, st["seed"] >> 32))
    st["n"] += 1
    return ((int(w[1]) << 32) | int(w[0])) & ~1


def _check_pair(q: torch.Tensor, s: torch.Tensor, qn: str, sn: str) -> None:
    _mx.check_pair(q, s, qn, sn, torch.uint8, "uint8 (two e2m1 codes per byte)", 2)


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
    return _mx.is_fast_shape(M, N, K, TILE_K)


def gemm_mxfp4_tn(aq: torch.Tensor, a_s: torch.Tensor, bq: torch.Tensor, b_s: torch.Tensor,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """``dequant(aq, a_s) @ dequant(bq, b_s).T`` -> bf16 ``[M, N]``.

    ``aq`` ``[M, K/2]`` and ``bq`` ``[N, K/2]`` are packed e2m1 (uint8), ``a_s``
    / ``b_s`` their uint8 scales ``[., K/32]``.  Contract: M, N and K multiples
    of 256.  Row strides may exceed the logical widths (views into wider
    buffers, K slices of ``q`` with the matching column slice of ``s``) as
    long as element rows stay 16-byte and scale rows 4-byte aligned."""
    return _mx.gemm_tn("mxfp4", TILE_K, 2, _check_pair, dequantize_mxfp4, aq, a_s, bq, b_s, out)
