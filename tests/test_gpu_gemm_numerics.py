"""Elementwise fp64 and bit-exact checks of the bf16 GEMM entry points:
``mxk_gemm_bf16_tn`` and ``_tn_variant`` (``gemm_bf16.hip``: the 256-tile
schedules and the bounds-checked generic kernel), ``mxk_gemm_bf16_ex_variant``
and ``_ex_ws`` (``gemm_bf16_layouts.hip``: the x and x2 layout kernels, the
split tail and its fixup), ``mxk_gemm_bf16_rope`` (schedule 52 with the rotary
embedding in its epilogue) and the three products of ``mxk8s.ops.linear``.
Every kernel is called through ``_lib`` into poisoned outputs, after the
exported plan (``gemm_plan.h``) of that very call was asserted.  The
references are fp64 on the CPU (``tests/kernel_refs.py``), so no GPU BLAS is
trusted.

Plain GEMM.  Products of two bf16 values are exact in fp32, so a dot product
of depth K only rounds in its K - 1 additions; with S = sum |a| |b| and the
factor 2 for MFMA's undocumented internal rounding
(``test_gpu_swiglu_gemm_numerics.py`` derives it):

    delta = K 2^-23 S
    bound = 2^-8 |d| + delta + atol

2^-8 is round-to-nearest bf16 just above a power of two, atol = 1e-30 only
matters next to zero.  The split tail accumulates two K halves in fp32 and the
fixup adds them in fp32: still at most K - 1 additions, the same bound.  The
generic kernel accumulates 32-deep MFMA steps in fp32: the same bound.

RoPE epilogue (``gemm_tn_core.h`` EPI 5, ``mx_common.h``
``store_block_lds_rope``, ``rope8_bf16``, ``rope_pair``).  The kernel packs the
fp32 accumulators to bf16 into its LDS slice, each lane reads its own 8
columns and the partner's 64 columns away, widens them to fp32, computes
x' = fma(x, c, -(y s)) and y' = fma(y, c, x s) with the fp32 table entries of
row t mod S, and rounds to bf16 again: the reading the bound below was asked
for, nothing differs.  With x~ = bf16(acc_x), |x~ - x| <= 2^-8 |x| + delta_x
(rounding of an accumulator that is itself off by delta_x; the cross term
2^-8 delta_x is inside delta's factor 2), likewise y~.  The product y~ s
rounds once (2^-24 |y s|) and the fma once (2^-24 |x'|); both are inside
2^-23 (|x c| + |y s|).  The last rounding to bf16 is 2^-8 |x'|:

    bound_x' = 2^-8 |x'| + |c| (2^-8 |x| + delta_x) + |s| (2^-8 |y| + delta_y)
               + 2^-23 (|x c| + |y s|) + atol

and bound_y' the same with x and y exchanged.  The reference is the fp64
rotation of the fp64 d with the fp32 tables as exact inputs.

Input families (``kernel_refs.gemm_inputs``, made on the CPU from a seed).
*tight* and *signed*: magnitudes in [2^-4, 1.5), power-of-two scales per row of
a (period 9) and per column of b (period 7), a zero row and a zero column in
each operand.  On tight every product of a dot product has one sign, S = |d|,
and for K <= 1216 delta is at most 3.7 % of the bf16 rounding: the bound is
bf16 rounding and little else, asserted from the reference alone as
``loose_fraction <= 10 %``.  On signed d cancels and delta carries weight.
*exact*: an entry is nonzero with probability min(1, sqrt(48 / K)), then +-1 or
+-2.  max S <= 256 is asserted on the reference before any kernel result is
looked at; then every partial sum in any order is an integer of magnitude at
most 256, exact in fp32 and in bf16, and the output must be bit-equal to the
reference rounded to bf16: one wrong k index anywhere changes bits.  For the
RoPE GEMM exact comes with a table of quarter turns picked by a hash of
(position, frequency): the rotated output is an exact signed permutation, and
a wrong partner column, position row or frequency index changes bits.
``tests/test_kernel_refs_cpu.py`` shows on a float32 emulation that the
unmutated arithmetic stays inside these checks and which family catches which
planted defect, and checks max S and loose_fraction for every shape used here.

Every test prints ``RATIO <case> <largest error / bound>`` over the variants
it ran (exact: 0, or inf on a bit mismatch) and fails only after all of them
ran, naming the worst element.  profiles/gemm_numerics/ratios.txt keeps the
lines of the recorded run.

Measured (MI355X, production library: TN schedules 1, 6, 9, 26, 47, 52, layout
variants 0-3).  Largest ratio per entry point and output C, and the case that
gave it; the exact family was bit-equal in every case (ratio 0), the linear
products and the 4 GiB test included:

    mxk_gemm_bf16_tn_variant          0.994  512x768x64, tight
    mxk_gemm_bf16_tn, narrow C        0.940  512x768x320, signed
    mxk_gemm_bf16_tn, generic kernel  0.989  255x257x63, signed
    mxk_gemm_bf16_ex_variant          0.993  tn layout, 256x512x64, tight
    mxk_gemm_bf16_ex_ws, split        0.766  tn layout, 256x256x1024, signed
    mxk_gemm_bf16_ex_ws, no split     0.774  tn layout, 256x256x960, signed
    mxk_gemm_bf16_rope                0.987  512x1536, rope_cols 1280, K 64, signed

(bf16 rounding alone reaches 0.996 of the bound.)  The file's 193 tests took
4.6 s of wall time.  Against the experiments library (MXK_KERNELS_LIB: every
non-ablation TN schedule and layout variant 4 as well) they passed in 5.2 s
with the same RATIO lines, so no K list is thinned.  No case failed, so no
kernel changed.
"""
import ctypes
import functools
import os

import pytest
import torch

import kernel_refs as R
from mxk8s.ops import _lib
from test_gpu_fused_numerics import _bits, _poison

pytestmark = pytest.mark.gpu

POISON = 0x7FC1
LAYOUTS = {"tn": (1, 1), "nn": (1, 0), "tt": (0, 1), "nt_wgrad": (0, 0)}
GEMM_TN, GEMM_X, GEMM_X2, GEMM_X2T = 0, 1, 2, 3        # gemm_plan.h GemmFamily


# ---- references, cached per (shape, family) -----------------------------------
@functools.lru_cache(maxsize=None)
def _case(M, N, K, family, seed=0):
    """-> (a [M][K], b [K][N], ref, bound).  exact: ref is the reference
    rounded to bf16 and bound is None."""
    a, b = R.gemm_inputs(M, N, K, family, seed)
    return (a, b, *_ref(a, b, family))


def _ref(a, b, family):
    d, bound, S = R.gemm_plain(a, b)
    if family == "exact":
        assert S.max().item() <= R.GEMM_EXACT_MAX_S, f"max S = {S.max().item()}"
        return d.bfloat16(), None
    if family == "tight":
        loose = R.loose_fraction(d, bound)
        assert loose <= 0.10, f"{loose:.3f} of the bounds are not bf16 rounding alone"
    return d, bound


class _Tally:
    """The checks of one case over its variants: the largest error / bound,
    the worst element, one RATIO line and one assertion at the end."""

    def __init__(self, case, ref, bound, dev):
        self.case, self.ref, self.bound = case, ref, bound
        self.want = ref.view(torch.int16).to(dev) if bound is None else None
        self.worst, self.fails, self.ran = 0.0, [], 0

    def check(self, variant, got, ref=None, bound=None):
        """got [M][N] on the device against the case's reference (or ref /
        bound given, ref in bf16 with bound None for bits)."""
        self.ran += 1
        if ref is None:
            ref, bound, want = self.ref, self.bound, self.want
        else:
            want = ref.view(torch.int16).to(got.device) if bound is None else None
        if bound is None:
            bad = got.contiguous().view(torch.int16) != want
            n = int(bad.sum())
            ratio = float("inf") if n else 0.0
            r, c = divmod(int(bad.view(-1).int().argmax()), bad.shape[1])
            why = f"{n} elements differ in bits, the first at ({r}, {c})"
        else:
            ratio, r, c = R.worst_ratio(got, ref, bound)
            why = f"error / bound = {ratio:.3g} at ({r}, {c})"
        self.worst = max(self.worst, ratio)
        if not ratio <= 1:
            self.fails.append(f"{variant}: {why}")

    def fail(self, variant, why):
        self.fails.append(f"{variant}: {why}")

    def done(self):
        assert self.ran
        print(f"RATIO {self.case} {self.worst:.3g}")
        assert not self.fails, f"{self.case}: " + "; ".join(self.fails)


# ---- operands and outputs in poisoned, padded buffers ---------------------------
class _Buf:
    """A [rows][cols] bf16 matrix of row stride ld inside a poisoned buffer,
    its first element ``skip`` elements past a 16-B boundary."""

    def __init__(self, rows, cols, dev, ld=None, skip=0, fill=None):
        self.rows, self.cols, self.ld, self.skip = rows, cols, ld or cols, skip
        self.buf = _poison((rows * self.ld + 8,), torch.bfloat16, dev)
        assert self.buf.data_ptr() % 16 == 0
        self.t = self._view(self.buf)
        if fill is not None:
            self.t.copy_(fill)
        self.ptr = self.t.data_ptr()
        assert self.ptr % 16 == 2 * skip

    def _view(self, buf):
        return buf[self.skip:self.skip + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]

    def pads_intact(self):
        chk = self.buf.clone().view(torch.int16)
        self._view(chk).fill_(POISON)
        return bool((chk == POISON).all())


def _operands(a, b, layout, dev, lda=None, ldb=None, a_skip=0):
    """a [M][K], b [K][N] as the layout stores them -> (_Buf A, _Buf B)."""
    ak, bk = LAYOUTS[layout]
    sa = a if ak else a.t()
    sb = b.t() if bk else b
    return (_Buf(*sa.shape, dev, lda, a_skip, fill=sa), _Buf(*sb.shape, dev, ldb, fill=sb))


def _stream(dev):
    return _lib.stream_ptr(dev)


def _default_schedule():
    """The resolved MXK_TN_VARIANT (gemm_bf16.hip fix_default_variant)."""
    L = _lib.lib()
    try:
        v = int(os.environ.get("MXK_TN_VARIANT", "52"))
    except ValueError:
        v = 52
    return v if L.mxk_gemm_bf16_tn_variant_built(v) and v != 1 else 52


def _tn_schedules():
    L = _lib.lib()
    built = [v for v in range(L.mxk_gemm_bf16_tn_num_variants())
             if L.mxk_gemm_bf16_tn_variant_built(v) and not L.mxk_gemm_bf16_tn_is_ablation(v)]
    assert {1, 6, 9, 26, 47, 52} <= set(built)
    return built


def _tn_plan(A, B, C, M, N, K):
    out = (ctypes.c_long * 4)()
    assert _lib.lib().mxk_gemm_bf16_tn_plan(M, N, K, A.ld, B.ld, C.ld, A.ptr % 16, B.ptr % 16,
                                            C.ptr % 16, _default_schedule(), out) == 0
    return tuple(out)


def _ex_plan(A, B, C, M, N, K, layout, variant, ws=None):
    L = _lib.lib()
    ak, bk = LAYOUTS[layout]
    out = (ctypes.c_long * 9)()
    assert L.mxk_gemm_bf16_ex_plan(M, N, K, A.ld, B.ld, C.ld, ak, bk, A.ptr % 16, B.ptr % 16,
                                   C.ptr % 16, variant, L.mxk_gemm_available_cus(), 0,
                                   L.mxk_gemm_bf16_ex_variant_built(4),
                                   ws.data_ptr() % 16 if ws is not None else 0,
                                   ws.numel() * ws.element_size() if ws is not None else 0, out) == 0
    return tuple(out)        # family, hb, order, wide, grid, tail, q_full, ws_bytes, split


def _run_tn_variant(A, B, C, M, N, K, v):
    st = _lib.lib().mxk_gemm_bf16_tn_variant(A.ptr, B.ptr, C.ptr, M, N, K, A.ld, B.ld, C.ld, v,
                                             _stream(C.t.device))
    _lib.check(st, f"mxk_gemm_bf16_tn_variant {v}")
    torch.cuda.synchronize()


def _run_tn(A, B, C, M, N, K):
    st = _lib.lib().mxk_gemm_bf16_tn(A.ptr, B.ptr, C.ptr, M, N, K, A.ld, B.ld, C.ld, _stream(C.t.device))
    _lib.check(st, "mxk_gemm_bf16_tn")
    torch.cuda.synchronize()


# ---- 1. the TN schedules ---------------------------------------------------------
def _tn_all_schedules(tally, a, b, M, N, K, dev, lda=None, ldb=None, ldc=None):
    A, B = _operands(a, b, "tn", dev, lda, ldb)
    for v in _tn_schedules():
        C = _Buf(M, N, dev, ldc)
        if v == 9:      # the layout kernel at hipBLASLt's positions, through the ex plan
            assert _ex_plan(A, B, C, M, N, K, "tn", 2)[:5] == (GEMM_X2, 1, 0, 1, (M // 256) * (N // 256))
        _run_tn_variant(A, B, C, M, N, K, v)
        tally.check(f"schedule {v}", C.t)
        if not (A.pads_intact() and B.pads_intact() and C.pads_intact()):
            tally.fail(f"schedule {v}", "padding overwritten")


@pytest.mark.parametrize("family", R.GEMM_FAMILIES)
@pytest.mark.parametrize("K", R.GEMM_TN_KS)
@pytest.mark.parametrize("M,N", R.GEMM_TN_SHAPES)
def test_tn_schedules(cuda_device, M, N, K, family):
    """Every built non-ablation schedule of the 256-tile kernel over 1-7, 13
    and 19 K-tiles (every remainder of schedule 47 / 52's 6-slot cycle), one
    tile and 2 x 3 tiles."""
    a, b, ref, bound = _case(M, N, K, family)
    tally = _Tally(f"tn_variant[{M}x{N}x{K},{family}]", ref, bound, cuda_device)
    _tn_all_schedules(tally, a, b, M, N, K, cuda_device)
    tally.done()


def test_tn_schedules_xcd_map(cuda_device):
    """16 x 16 tiles: the XCD super-block tile map, bit-equal on exact."""
    M, N, K = R.GEMM_TN_XCD_SHAPE
    a, b, ref, bound = _case(M, N, K, "exact")
    tally = _Tally(f"tn_variant[{M}x{N}x{K},exact]", ref, bound, cuda_device)
    _tn_all_schedules(tally, a, b, M, N, K, cuda_device)
    tally.done()


# ---- 2. strides and alignment on the TN kernel --------------------------------------
@pytest.mark.parametrize("family", R.GEMM_FAMILIES)
def test_tn_padded_strides(cuda_device, family):
    """lda = K + 8, ldb = K + 72, ldc = N + 8 on every schedule; the pad
    columns keep their poison."""
    M, N, K = R.GEMM_STRIDED_SHAPE
    a, b, ref, bound = _case(M, N, K, family)
    tally = _Tally(f"tn_variant[{M}x{N}x{K},{family},padded]", ref, bound, cuda_device)
    _tn_all_schedules(tally, a, b, M, N, K, cuda_device, K + 8, K + 72, N + 8)
    tally.done()


@pytest.mark.parametrize("family", R.GEMM_FAMILIES)
def test_tn_narrow_c_routes(cuda_device, family):
    """mxk_gemm_bf16_tn: ldc = N + 4, and a C that starts 8 B past a 16-B
    boundary, resolve to the 8-B-store schedule 1; the aligned call to the
    default."""
    M, N, K = R.GEMM_STRIDED_SHAPE
    a, b, ref, bound = _case(M, N, K, family)
    tally = _Tally(f"tn[{M}x{N}x{K},{family},narrow C]", ref, bound, cuda_device)
    A, B = _operands(a, b, "tn", cuda_device)
    for name, ldc, skip, sched in (("aligned", N, 0, _default_schedule()), ("ldc N+4", N + 4, 0, 1),
                                   ("C at 8 B", N, 4, 1)):
        C = _Buf(M, N, cuda_device, ldc, skip)
        assert _tn_plan(A, B, C, M, N, K) == (0, sched, 6, 1), name
        _run_tn(A, B, C, M, N, K)
        tally.check(name, C.t)
        if not C.pads_intact():
            tally.fail(name, "padding overwritten")
    tally.done()


# ---- 3. the bounds-checked generic kernel ----------------------------------------------
@pytest.mark.parametrize("family", ["signed", "exact"])
@pytest.mark.parametrize("M,N,K,lda,a_skip", [(1, 1, 1, None, 0), (17, 33, 65, None, 0),
                                              (255, 257, 63, None, 0), (256, 256, 64, None, 1),
                                              (256, 256, 64, 66, 0)])
def test_tn_generic_kernel(cuda_device, M, N, K, lda, a_skip, family):
    """Shapes that do not tile, a tiled shape whose A starts 2 B past a 16-B
    boundary and one with lda = K + 2: the plan says generic."""
    a, b, ref, bound = _case(M, N, K, family)
    tally = _Tally(f"tn generic[{M}x{N}x{K},lda{lda or K},A+{2 * a_skip}B,{family}]", ref, bound, cuda_device)
    A, B = _operands(a, b, "tn", cuda_device, lda, a_skip=a_skip)
    C = _Buf(M, N, cuda_device)
    assert _tn_plan(A, B, C, M, N, K) == (1, -1, (N + 63) // 64, (M + 63) // 64)
    _run_tn(A, B, C, M, N, K)
    tally.check("generic", C.t)
    if not C.pads_intact():
        tally.fail("generic", "padding overwritten")
    tally.done()


# ---- 4. the layout kernel ------------------------------------------------------------------
def _ex_variants(K, wide):
    L = _lib.lib()
    return [v for v in range(5) if L.mxk_gemm_bf16_ex_variant_built(v) and (v < 4 or (K >= 1152 and wide))]


def _expected_ex(layout, variant):
    """(GemmFamily, schedule bit) gemm_plan.h resolves (layout, variant) to."""
    ak, bk = LAYOUTS[layout]
    if variant == 4:
        return GEMM_X2T, int(ak == bk)
    if variant == 0:
        return GEMM_X, 0
    if variant == 1:
        return (GEMM_TN, 0) if ak and bk else (GEMM_X2, int(not ak and not bk))
    return GEMM_X2, int(variant == 2)


def _ex_all_variants(tally, a, b, M, N, K, layout, dev, lda=None, ldb=None, ldc=None):
    L = _lib.lib()
    ak, bk = LAYOUTS[layout]
    A, B = _operands(a, b, layout, dev, lda, ldb)
    wide = int((ldc or N) % 8 == 0)
    L.mxk_gemm_x2_set_order(0)
    for v in _ex_variants(K, wide):
        C = _Buf(M, N, dev, ldc)
        plan = _ex_plan(A, B, C, M, N, K, layout, v)
        tiles = (M // 256) * (N // 256)
        grid = min(tiles, L.mxk_gemm_available_cus()) if v == 4 else tiles     # x2t is persistent
        assert plan == (*_expected_ex(layout, v), 0, wide, grid, 0, tiles, 0, 0), (layout, v, plan)
        if plan[0] == GEMM_TN:      # handed to mxk_gemm_bf16_tn
            assert _tn_plan(A, B, C, M, N, K)[:2] == (0, _default_schedule() if wide else 1)
        st = L.mxk_gemm_bf16_ex_variant(A.ptr, B.ptr, C.ptr, M, N, K, A.ld, B.ld, C.ld, ak, bk, v,
                                        _stream(dev))
        _lib.check(st, f"mxk_gemm_bf16_ex_variant {layout} {v}")
        torch.cuda.synchronize()
        tally.check(f"variant {v}", C.t)
        if not (A.pads_intact() and B.pads_intact() and C.pads_intact()):
            tally.fail(f"variant {v}", "padding overwritten")


@pytest.mark.parametrize("family", R.GEMM_FAMILIES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("M,N,K", R.GEMM_EX_SHAPES)
def test_ex_variants(cuda_device, M, N, K, layout, family):
    """Variants 0-3 (and 4 where built, K >= 1152) of every operand layout:
    1, 2 and 4 K-tiles on two tiles (the prologue-only, DMA-free and first
    steady K loops), 3, 5, 7 and 19 on six."""
    a, b, ref, bound = _case(M, N, K, family)
    tally = _Tally(f"ex_variant[{layout},{M}x{N}x{K},{family}]", ref, bound, cuda_device)
    _ex_all_variants(tally, a, b, M, N, K, layout, cuda_device)
    tally.done()


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_ex_variants_xcd_map(cuda_device, layout):
    M, N, K = R.GEMM_EX_XCD_SHAPE
    a, b, ref, bound = _case(M, N, K, "exact")
    tally = _Tally(f"ex_variant[{layout},{M}x{N}x{K},exact]", ref, bound, cuda_device)
    _ex_all_variants(tally, a, b, M, N, K, layout, cuda_device)
    tally.done()


@pytest.mark.parametrize("family", R.GEMM_FAMILIES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_ex_padded_strides_narrow_c(cuda_device, layout, family):
    """Padded lda and ldb, and ldc = N + 4 (the plan's wide == 0: 8-B C
    stores; variant 1 on K-major operands hands to TN schedule 1)."""
    M, N, K = R.GEMM_STRIDED_SHAPE
    ak, bk = LAYOUTS[layout]
    a, b, ref, bound = _case(M, N, K, family)
    tally = _Tally(f"ex_variant[{layout},{M}x{N}x{K},{family},padded,ldc N+4]", ref, bound, cuda_device)
    _ex_all_variants(tally, a, b, M, N, K, layout, cuda_device, (K if ak else M) + 8, (K if bk else N) + 72,
                     N + 4)
    tally.done()


# ---- 5. the split tail -----------------------------------------------------------------------
@pytest.mark.parametrize("family", ["signed", "exact"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_ex_ws_split_tail(cuda_device, layout, family):
    """mxk_gemm_bf16_ex_ws: with all but 4 CUs reserved 512 x 768 is 4 whole
    tiles plus a tail of 2 run as K halves through the fp32 workspace and the
    fixup kernel; on the whole chip 256 x 256 x 1024 is all split; at K = 960
    nothing splits.  The workspace past the planned bytes keeps its poison."""
    L = _lib.lib()
    dev = cuda_device
    ak, bk = LAYOUTS[layout]
    hb = int(layout == "nt_wgrad")
    unsplit = _expected_ex(layout, 1)
    L.mxk_gemm_set_reserved_cus(0)
    hw = L.mxk_gemm_available_cus()
    # reserved CUs -> family, schedule bit, grid, tail, q_full, split
    wants = [(hw - 4, (GEMM_X2, hb, 4, 2, 4, 1)), (0, (GEMM_X2, hb, 0, 1, 0, 1)), (0, (*unsplit, 1, 0, 1, 0))]
    tallies = []
    try:
        L.mxk_gemm_x2_set_order(0)
        for (M, N, K), (reserved, want) in zip(R.GEMM_SPLIT_SHAPES, wants):
            a, b, ref, bound = _case(M, N, K, family)
            tally = _Tally(f"ex_ws[{layout},{M}x{N}x{K},{family},split{want[-1]}]", ref, bound, dev)
            tallies.append(tally)
            L.mxk_gemm_set_reserved_cus(reserved)
            assert L.mxk_gemm_available_cus() == hw - reserved
            A, B = _operands(a, b, layout, dev)
            C = _Buf(M, N, dev)
            ws = _poison((1 << 20,), torch.float32, dev)          # 4 MiB; a tail of 2 takes 1 MiB
            plan = _ex_plan(A, B, C, M, N, K, layout, 1, ws)
            assert (plan[0], plan[1], *plan[4:7], plan[8]) == want, (layout, M, N, K, plan)
            assert plan[2:4] == (0, 1) and plan[7] == 2 * plan[5] * 256 * 256 * 4 <= ws.numel() * 4
            split = ctypes.c_int(-1)
            st = L.mxk_gemm_bf16_ex_ws(A.ptr, B.ptr, C.ptr, M, N, K, A.ld, B.ld, C.ld, ak, bk, ws.data_ptr(),
                                       ws.numel() * 4, ctypes.byref(split), _stream(dev))
            _lib.check(st, "mxk_gemm_bf16_ex_ws")
            torch.cuda.synchronize()
            tally.check("ex_ws", C.t)
            if split.value != want[-1]:
                tally.fail("ex_ws", f"split flag {split.value}")
            if not bool((ws.view(torch.int32)[plan[7] // 4:] == 0x7FC12345).all()):
                tally.fail("ex_ws", "workspace written past the planned bytes")
            if not C.pads_intact():
                tally.fail("ex_ws", "padding overwritten")
    finally:
        L.mxk_gemm_set_reserved_cus(0)
    assert len(tallies) == len(wants)
    errors = []
    for tally in tallies:
        try:
            tally.done()
        except AssertionError as e:
            errors.append(str(e))
    assert not errors, " | ".join(errors)


# ---- 6. the RoPE-epilogue GEMM -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rope_tables(kind):
    if kind == "quarter":
        return R.quarter_turn_tables(R.GEMM_ROPE_S)
    from mxk8s.ops.fused import rope_tables
    return rope_tables(R.GEMM_ROPE_S, 128)


@functools.lru_cache(maxsize=None)
def _rope_case(N, rope_cols, K, family):
    a, b, ref, bound = _case(R.GEMM_ROPE_M, N, K, family)      # asserts max S / loose_fraction
    cos, sin = _rope_tables("quarter" if family == "exact" else "real")
    rref, rbound = R.gemm_rope(a, b, cos, sin, R.GEMM_ROPE_S, rope_cols)
    return a, b, cos, sin, (rref.bfloat16(), None) if family == "exact" else (rref, rbound)


@pytest.mark.parametrize("family", ["signed", "exact"])
@pytest.mark.parametrize("K", R.GEMM_ROPE_KS)
@pytest.mark.parametrize("N,rope_cols", R.GEMM_ROPE_COLS)
def test_rope_epilogue(cuda_device, N, rope_cols, K, family):
    """mxk_gemm_bf16_rope on two sequences of 256 tokens (row 256 sits at
    position 0): every column is roped but the last 256 / 128 (then one wave of
    the last tile's pair rotates and its sibling does not).  signed with the
    model's tables inside the bound, exact with quarter turns bit-equal; the
    columns from rope_cols on bit-equal to the plain schedule 52."""
    L = _lib.lib()
    dev = cuda_device
    M, S = R.GEMM_ROPE_M, R.GEMM_ROPE_S
    a, b, cos, sin, (ref, bound) = _rope_case(N, rope_cols, K, family)
    tally = _Tally(f"rope[{M}x{N}/{rope_cols}x{K},{family}]", ref, bound, dev)
    A, B = _operands(a, b, "tn", dev)
    C, plain = _Buf(M, N, dev), _Buf(M, N, dev)
    cos_d, sin_d = cos.to(dev), sin.to(dev)
    assert cos_d.shape == (S, 64) and cos_d.dtype == torch.float32 and cos_d.is_contiguous()
    st = L.mxk_gemm_bf16_rope(A.ptr, B.ptr, C.ptr, M, N, K, A.ld, B.ld, C.ld, cos_d.data_ptr(),
                              sin_d.data_ptr(), S, rope_cols, _stream(dev))
    _lib.check(st, "mxk_gemm_bf16_rope")
    _run_tn_variant(A, B, plain, M, N, K, 52)
    tally.check("rope", C.t)
    if not torch.equal(_bits(C.t[:, rope_cols:]), _bits(plain.t[:, rope_cols:])):
        tally.fail("rope", "columns past rope_cols differ from schedule 52")
    if torch.equal(_bits(C.t[:, :rope_cols]), _bits(plain.t[:, :rope_cols])):
        tally.fail("rope", "nothing was rotated")
    if not C.pads_intact():
        tally.fail("rope", "padding overwritten")
    tally.done()


# ---- 7. what the training step calls ------------------------------------------------------------
def test_linear_products_exact(cuda_device, monkeypatch):
    """mxk8s.ops.linear._fwd, _dgrad and _wgrad_into on exact operands (512
    tokens, 256 in, 768 out), bit-equal, with torch.matmul made to raise: a
    silent fallback to the library GEMM fails."""
    from mxk8s.ops import linear
    dev = cuda_device
    (fwd, dgrad, wgrad) = (_case(*s, "exact") for s in R.GEMM_LINEAR_SHAPES)
    tally = _Tally("linear[512 tokens,256 in,768 out,exact]", fwd[2], None, dev)

    def no_matmul(*args, **kwargs):
        raise AssertionError("torch.matmul called: the hand-written GEMM was not taken")
    monkeypatch.setattr(torch, "matmul", no_matmul)
    # y = x W^T: a = x, b = W^T
    y = linear._fwd(fwd[0].to(dev), fwd[1].t().contiguous().to(dev))
    tally.check("_fwd", y, fwd[2], None)
    # dx = dy W: a = dy, b = W
    dx = linear._dgrad(dgrad[0].to(dev), dgrad[1].to(dev))
    tally.check("_dgrad", dx, dgrad[2], None)
    # dW = dy^T x: a = dy^T, b = x
    sink = _Buf(768, 256, dev)
    linear._wgrad_into(sink.t, wgrad[0].t().contiguous().to(dev), wgrad[1].to(dev))
    torch.cuda.synchronize()
    tally.check("_wgrad_into", sink.t, wgrad[2], None)
    tally.done()


# ---- 8. operands past 4 GiB ------------------------------------------------------------------------
def test_a_and_c_past_4gib(cuda_device):
    """A and C of 4 GiB + 256 KiB (M = 2^22 + 256 rows of stride 512).  Both
    kernels address an operand through one buffer resource per 256-row panel,
    based at a 64-bit pointer to the panel, and C through 64-bit pointers, so
    nothing should wrap; this pins that reading.  Only the first and the last
    256-row tile carry data, different in the two: bit-equal on exact, the
    rows between zero, the pad columns poison.  The default TN route and the
    nn layout route."""
    L = _lib.lib()
    dev = cuda_device
    N, K, ld = 256, 64, 512
    M = (1 << 22) + 256
    if torch.cuda.mem_get_info(dev)[0] < 12 << 30:
        pytest.skip("needs 12 GiB of free device memory")
    a0, b, ref0, _ = _case(256, N, K, "exact")
    a1 = R.gemm_inputs(256, N, K, "exact", seed=1)[0]
    ref1 = _ref(a1, b, "exact")[0]
    assert not torch.equal(a0, a1) and not torch.equal(ref0, ref1)
    tally = _Tally(f"past 4 GiB[{M}x{N}x{K},lda=ldc={ld},exact]", ref0, None, dev)
    A = C = None
    try:
        A = torch.zeros((M, ld), dtype=torch.bfloat16, device=dev)
        A[:256, :K], A[M - 256:, :K] = a0.to(dev), a1.to(dev)
        C = _poison((M, ld), torch.bfloat16, dev)
        assert A.numel() * 2 > 1 << 32 and A.data_ptr() % 16 == 0 and C.data_ptr() % 16 == 0
        Bt, Bn = b.t().contiguous().to(dev), b.to(dev)
        tiles = M // 256
        plan = (ctypes.c_long * 9)()
        assert L.mxk_gemm_bf16_tn_plan(M, N, K, ld, K, ld, 0, 0, 0, _default_schedule(), plan) == 0
        assert tuple(plan[:4]) == (0, _default_schedule(), tiles, 1)
        L.mxk_gemm_x2_set_order(0)
        assert L.mxk_gemm_bf16_ex_plan(M, N, K, ld, N, ld, 1, 0, 0, 0, 0, 1, L.mxk_gemm_available_cus(), 0,
                                       L.mxk_gemm_bf16_ex_variant_built(4), 0, 0, plan) == 0
        assert tuple(plan) == (GEMM_X2, 0, 0, 1, tiles, 0, tiles, 0, 0)
        for route in ("tn", "nn"):
            C.view(torch.int16).fill_(POISON)
            if route == "tn":
                st = L.mxk_gemm_bf16_tn(A.data_ptr(), Bt.data_ptr(), C.data_ptr(), M, N, K, ld, K, ld,
                                        _stream(dev))
            else:
                st = L.mxk_gemm_bf16_ex(A.data_ptr(), Bn.data_ptr(), C.data_ptr(), M, N, K, ld, N, ld, 1, 0,
                                        _stream(dev))
            _lib.check(st, f"{route} past 4 GiB")
            torch.cuda.synchronize()
            tally.check(f"{route} first tile", C[:256, :N], ref0, None)
            tally.check(f"{route} last tile", C[M - 256:, :N], ref1, None)
            if torch.count_nonzero(C[256:M - 256, :N]).item():
                tally.fail(route, "rows between the two tiles are not zero")
            if not bool((C.view(torch.int16)[:, N:] == POISON).all()):
                tally.fail(route, "pad columns overwritten")
    finally:
        del A, C
        torch.cuda.empty_cache()
    tally.done()
