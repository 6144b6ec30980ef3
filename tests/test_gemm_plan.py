"""The GEMM round / split-tail planner under CUs taken by collectives
(VERDICT r3 #4): the Python mirror and the C planner agree, and telling the
planner about k reserved CUs never plans more rounds than ignoring them.

Runs on the CPU: ``mxk_gemm_split_plan`` is host arithmetic in the kernel
library (loaded, never launched)."""
import ctypes
import itertools

import pytest

from mxk8s.ops import _lib, gemm

pytestmark = pytest.mark.skipif(not _lib.kernels_available(), reason="kernel library not built")

# Llama-3-8B step GEMMs at 16k tokens: output tiles (M/256 * N/256) and K
STEP = {
    "wqkv fwd": (64 * 24, 4096), "wo fwd": (64 * 16, 4096), "w13 fwd": (64 * 112, 4096),
    "w2 fwd": (64 * 16, 14336), "lm_head fwd": (64 * 501, 4096),
    "w2 dgrad": (64 * 56, 4096), "wqkv wgrad": (24 * 16, 16384), "w2 wgrad": (16 * 56, 16384),
}


@pytest.mark.parametrize("nwg,K,cus", list(itertools.product(
    [1, 64, 255, 256, 257, 384, 448, 1024, 1536, 3584, 7168, 32064],
    [512, 1024, 4096, 14336, 16384], [256, 240, 224, 192, 128])))
def test_c_and_python_plans_agree(nwg, K, cus):
    q = ctypes.c_long(0)
    tail = _lib.lib().mxk_gemm_split_plan(nwg, K, cus, ctypes.byref(q))
    assert (q.value, tail) == gemm.split_plan(nwg, K, cus)


@pytest.mark.parametrize("k", [16, 32, 64])
@pytest.mark.parametrize("name", sorted(STEP))
def test_reserved_cus_never_plans_more_rounds(name, k):
    """Planning for 256 - k CUs (what is free beside RCCL) against planning
    for 256 while only 256 - k are free: the first is never worse, and the
    planned rounds stay within one half-round of the ideal nwg / (256 - k)."""
    nwg, K = STEP[name]
    free = 256 - k

    def actual(plan_cus):
        whole, tail = gemm.split_plan(nwg, K, plan_cus)
        # what runs: `whole` tiles then 2 * tail half-depth workgroups, all
        # on `free` CUs
        r = -(-whole // free)
        if tail:
            r += 0.5 * -(-2 * tail // free)
        return r

    aware, blind = actual(free), actual(256)
    assert aware <= blind, (aware, blind)
    assert aware <= nwg / free + 0.5 + 1e-9, (aware, nwg / free)


def test_set_reserved_cus_roundtrip():
    L = _lib.lib()
    try:
        gemm.set_reserved_cus(32)
        assert L.mxk_gemm_reserved_cus() == 32
        gemm.set_reserved_cus(-5)
        assert L.mxk_gemm_reserved_cus() == 0
    finally:
        gemm.set_reserved_cus(0)


# ---- staggered rounds (schedule 54) ----------------------------------------
def _simulate(T, sx, cus, dur):
    """Greedy in-order dispatch per XCD (workgroup b on XCD b % 8, the next
    one to the first free CU): finish time of the grid, and the times at
    which tiles end (C stores)."""
    import heapq
    cx = cus // 8
    free = [[0.0] * cx for _ in range(8)]
    for q in free:
        heapq.heapify(q)
    end, stores = 0.0, []
    for b in range(T + 8 * sx):
        _, part, _ = gemm.stagger_part(b, T, sx)
        t0 = heapq.heappop(free[b & 7])
        t1 = t0 + (dur if part == 0 else dur / 2)
        heapq.heappush(free[b & 7], t1)
        end = max(end, t1)
        if part != 1:
            stores.append(t1)
    return end, stores


@pytest.mark.parametrize("T,K", [(1024, 8192), (4096, 16384), (64 * 112, 4096), (64 * 56, 4096),
                                 (64 * 24, 4096), (64 * 16, 4096), (256, 8192), (1000, 4096)])
@pytest.mark.parametrize("cus", [256, 240, 192])
def test_stagger_plan_and_parts(T, K, cus):
    sx = gemm.stagger_plan(T, K, cus)
    assert sx == _lib.lib().mxk_gemm_stagger_plan(T, K, cus)
    if T % 8 or T // 8 < 2 * (cus // 8):
        assert sx == 0
        return
    assert sx == cus // 16
    out = (ctypes.c_int * 3)()
    whole, first, second = {}, {}, {}
    for b in range(T + 8 * sx):
        p = gemm.stagger_part(b, T, sx)
        _lib.lib().mxk_gemm_stagger_part(b, T, sx, out)
        assert tuple(out) == p
        v, part, slot = p
        assert v % 8 == b % 8                      # the tile map keeps the XCD
        {0: whole, 1: first, 2: second}[part].setdefault(v, []).append((b, slot))
    # every tile exactly once: whole, or a first and a second half
    assert set(whole) | set(first) == set(range(T))
    assert not set(whole) & set(first) and set(first) == set(second)
    assert all(len(v) == 1 for d in (whole, first, second) for v in d.values())
    slots = sorted(first[v][0][1] for v in first)
    assert slots == list(range(8 * sx))
    for v in first:
        (bp, sp), (bc, sc) = first[v][0], second[v][0]
        assert sp == sc and bp < bc and bp % 8 == bc % 8   # producer dispatched first, same XCD
    # whole rounds stay whole (ideal makespan) and the stores no longer
    # coincide: half of them fall half a tile out of phase
    cx = cus // 8
    if (T // 8) % cx == 0:
        end, stores = _simulate(T, sx, cus, 1.0)
        assert end == pytest.approx(T / 8 / cx)
        frac = [t % 1.0 for t in stores]
        assert sum(abs(f - 0.5) < 1e-9 for f in frac) >= len(stores) // 2 - 8 * sx


def test_set_exclusive_roundtrip():
    try:
        gemm.set_exclusive(True)
        assert gemm.exclusive()
        gemm.set_exclusive(False)
        assert not gemm.exclusive()
    finally:
        gemm.set_exclusive(False)


@pytest.mark.parametrize("T,cus", [(1024, 256), (4096, 256), (64 * 56, 256), (1024, 192)])
def test_stagger_by_xcd_parts(T, cus):
    """Schedule 57: every tile once (whole, or two halves on one XCD of 4-7,
    producer dispatched first); XCDs 0-3 and 4-7 finish together and store
    half a tile apart."""
    cx = cus // 8
    out = (ctypes.c_int * 3)()
    seen = {}
    for b in range(T + 8 * cx):
        p = gemm.stagger_part_xcd(b, T, cx)
        _lib.lib().mxk_gemm_stagger_part_xcd(b, T, cx, out)
        assert tuple(out) == p
        v, part, slot = p
        if part < 0:
            assert b & 7 < 4
            continue
        assert v % 8 == b % 8
        seen.setdefault(v, []).append((part, b, slot))
    assert set(seen) == set(range(T))
    for v, ps in seen.items():
        kinds = sorted(p for p, _, _ in ps)
        assert kinds in ([0], [1, 2])
        if kinds == [1, 2]:
            (p1, b1, s1), (p2, b2, s2) = sorted(ps)
            assert v % 8 >= 4 and s1 == s2 and b1 < b2 and b1 % 8 == b2 % 8
    # dispatch simulation (unit tile time): both XCD groups end at T / 8 / cx,
    # and group 4-7 stores half a tile out of phase with group 0-3
    import heapq
    free = [[0.0] * cx for _ in range(8)]
    ends = {0: [], 1: []}
    for b in range(T + 8 * cx):
        v, part, _ = gemm.stagger_part_xcd(b, T, cx)
        if part < 0:
            continue
        q = free[b & 7]
        t0 = heapq.heappop(q)
        t1 = t0 + (1.0 if part == 0 else 0.5)
        heapq.heappush(q, t1)
        if part != 1:
            ends[(b & 7) >= 4].append(t1)
    if (T // 8) % cx == 0:
        assert max(ends[0]) == pytest.approx(T / 8 / cx) == max(ends[1])
        assert all(abs(t % 1.0) < 1e-9 for t in ends[0])
        assert sum(abs(t % 1.0 - 0.5) < 1e-9 for t in ends[1]) >= len(ends[1]) - 2 * 4 * cx


# ---- which kernel a call runs (native/kernels/gemm_plan.h) ------------------
# The expectations below are written from the dispatcher the plan replaced
# (the if / #ifdef ladders of mxk_gemm_bf16_ex_variant, _ex_ws, _tn and
# _dgrad_swiglu), not from the header.  The exports take the build, the knobs
# and the CU count as arguments, so one library answers for both builds.
FAMILY = ["tn", "x", "x2", "x2t"]
LAYOUTS = {"tn": (1, 1), "nn": (1, 0), "tt": (0, 1), "nt_wgrad": (0, 0)}
WS = 128 << 20       # a workspace no tail of the cases below outgrows


def ex_plan(layout, variant, *, M=512, N=768, K=320, lda=None, ldb=None, ldc=None, bits=(0, 0, 0),
            cus=256, order=0, exp=0, ws_bits=0, ws_bytes=0):
    """(status, dict of the plan); tight strides unless given."""
    ak, bk = LAYOUTS[layout]
    lda = (K if ak else M) if lda is None else lda
    ldb = (K if bk else N) if ldb is None else ldb
    ldc = N if ldc is None else ldc
    out = (ctypes.c_long * 9)(*([-7] * 9))
    st = _lib.lib().mxk_gemm_bf16_ex_plan(M, N, K, lda, ldb, ldc, ak, bk, *bits, variant, cus, order,
                                          exp, ws_bits, ws_bytes, out)
    if st:
        assert list(out) == [-7] * 9
        return st, None
    return 0, dict(family=FAMILY[out[0]], hb=out[1], order=out[2], wide=out[3], grid=out[4],
                   tail=out[5], q_full=out[6], ws=out[7], split=out[8])


def route(p):
    return (p["family"], p["hb"]) if p["family"] != "tn" else ("tn", 0)


def v1_route(layout):
    return {"tn": ("tn", 0), "nt_wgrad": ("x2", 1)}.get(layout, ("x2", 0))


@pytest.mark.parametrize("exp", [0, 1])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_ex_plan_resolution_table(layout, exp):
    nwg = 2 * 3
    want = {0: ("x", 0), 1: v1_route(layout), 2: ("x2", 1), 3: ("x2", 0), 4: v1_route(layout)}
    for variant, w in want.items():
        st, p = ex_plan(layout, variant, exp=exp)         # K = 320 < 18 * 64: no x2t
        assert st == 0 and route(p) == w, (variant, p)
        assert (p["grid"], p["wide"], p["split"], p["tail"], p["q_full"]) == (nwg, 1, 0, 0, nwg)
        assert p["order"] == 0
    # x2t: experiments build, K >= 18 * 64, 16-B C stores; else as variant 1
    ak, bk = LAYOUTS[layout]
    for cus, grid in ((256, 6), (4, 4)):
        st, p = ex_plan(layout, 4, K=1152, exp=1, cus=cus)
        assert st == 0 and route(p) == ("x2t", int(ak == bk)) and p["grid"] == grid and p["wide"] == 1
    assert route(ex_plan(layout, 4, K=1152, exp=0)[1]) == v1_route(layout)
    assert route(ex_plan(layout, 4, K=1088, exp=1)[1]) == v1_route(layout)
    assert route(ex_plan(layout, 4, K=1152, exp=1, ldc=768 + 4)[1]) == v1_route(layout)
    assert route(ex_plan(layout, 4, K=1152, exp=1, bits=(0, 0, 8))[1]) == v1_route(layout)
    # narrow C: the 8-B-store instances, the route unchanged
    for kw in (dict(ldc=768 + 4), dict(bits=(0, 0, 8))):
        for variant in (1, 2, 3):
            st, p = ex_plan(layout, variant, exp=exp, **kw)
            assert st == 0 and route(p) == want[variant] and p["wide"] == 0
    # the B-outer order bit: experiments build, x2 whole-tile launches only
    for variant in range(5):
        p = ex_plan(layout, variant, exp=exp, order=1)[1]
        assert p["order"] == int(exp and p["family"] == "x2"), (variant, p)
    assert ex_plan(layout, 4, K=1152, exp=1, order=1)[1]["order"] == 0


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_ex_plan_gate(layout):
    """Each single violated condition of the argument gate is invalid, for
    every variant; an N/M-major panel of exactly 4 GiB is, one row less is not."""
    ak, bk = LAYOUTS[layout]
    assert ex_plan(layout, 1)[0] == 0
    bad = [dict(M=0), dict(N=0), dict(K=0), dict(M=-512), dict(M=500), dict(N=760), dict(K=352),
           dict(lda=(320 if ak else 512) + 4), dict(ldb=(320 if bk else 768) + 4), dict(ldc=770),
           dict(lda=(320 if ak else 512) - 8), dict(ldb=(320 if bk else 768) - 8), dict(ldc=760),
           dict(bits=(8, 0, 0)), dict(bits=(0, 8, 0)), dict(bits=(0, 0, 4))]
    for kw in bad:
        for variant in range(5):
            assert ex_plan(layout, variant, **kw)[0] == 1, (kw, variant)
        # ... and with a split tail planned (6 tiles on 4 CUs at K = 1024)
        assert ex_plan(layout, 1, ws_bytes=WS, cus=4, **{"K": 1024, **kw})[0] == 1, kw
    for variant in (-1, 5):
        assert ex_plan(layout, variant)[0] == 1
    # K rows of ld elements, 2 B each: K = 1024, ld = 2^21 is exactly 4 GiB
    big = 1 << 21
    for name, major in (("lda", ak), ("ldb", bk)):
        for variant in (0, 1, 2, 3):
            assert ex_plan(layout, variant, K=1024, **{name: big})[0] == (0 if major else 1)
            assert ex_plan(layout, variant, K=1024, **{name: big - 8})[0] == 0


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_ex_ws_plan(layout):
    split_hb = int(layout == "nt_wgrad")     # TN included: whole tiles on x2, schedule bit 0
    for tiles, q_full in ((384, 256), (896, 768), (64, 0)):
        M, N = (tiles // 16) * 256, 16 * 256
        st, p = ex_plan(layout, 1, M=M, N=N, K=1024, ws_bytes=WS)
        assert st == 0 and route(p) == ("x2", split_hb), p
        tail = tiles - q_full
        assert (p["split"], p["tail"], p["q_full"], p["grid"]) == (1, tail, q_full, q_full)
        assert p["ws"] == 2 * tail * 256 * 256 * 4
        # null (0 bytes), misaligned or too-small workspace; K = 960, K % 128 != 0: variant 1
        for kw in (dict(ws_bytes=0), dict(ws_bytes=WS, ws_bits=8), dict(ws_bytes=p["ws"] - 1),
                   dict(ws_bytes=WS, K=960), dict(ws_bytes=WS, K=1088)):
            q = ex_plan(layout, 1, **{**dict(M=M, N=N, K=1024), **kw})[1]
            assert route(q) == v1_route(layout) and (q["split"], q["tail"], q["grid"]) == (0, 0, tiles)
        assert ex_plan(layout, 1, M=M, N=N, K=1024, ws_bytes=p["ws"])[1]["split"] == 1
    # 256 tiles fill the round; 257..384 leave at most half a round
    assert ex_plan(layout, 1, M=4096, N=4096, K=1024, ws_bytes=WS)[1]["split"] == 0
    assert ex_plan(layout, 1, M=4352, N=4096, K=1024, ws_bytes=WS)[1]["tail"] == 16


def tn_plan(M, N, K, *, lda=None, ldb=None, ldc=None, bits=(0, 0, 0), default=52):
    out = (ctypes.c_long * 4)()
    st = _lib.lib().mxk_gemm_bf16_tn_plan(M, N, K, K if lda is None else lda, K if ldb is None else ldb,
                                          N if ldc is None else ldc, *bits, default, out)
    return (st, None) if st else (0, tuple(out))


def test_tn_plan():
    assert tn_plan(512, 768, 256) == (0, (0, 52, 6, 1))
    assert tn_plan(512, 768, 256, default=26) == (0, (0, 26, 6, 1))
    for kw in (dict(ldc=772), dict(bits=(0, 0, 8))):          # narrow C: schedule 1
        assert tn_plan(512, 768, 256, **kw) == (0, (0, 1, 6, 1))
    generic = (0, (1, -1, 12, 8))                             # 64 x 64 tiles over (N, M)
    for kw in (dict(lda=260), dict(ldb=260), dict(ldc=770), dict(bits=(8, 0, 0)), dict(bits=(0, 8, 0)),
               dict(bits=(0, 0, 4))):
        assert tn_plan(512, 768, 256, **kw) == generic, kw
    assert tn_plan(500, 768, 256) == generic
    assert tn_plan(512, 700, 256) == (0, (1, -1, 11, 8))
    assert tn_plan(512, 768, 200) == generic
    assert tn_plan(512, 768, 256, lda=248) == (0, (0, 52, 6, 1))   # the TN entry asks no lda >= K
    for bad in ((0, 768, 256), (512, 0, 256), (512, 768, 0), (-512, 768, 256)):
        assert tn_plan(*bad)[0] == 1


def dgrad_plan(mode, *, M=512, F=1024, K=256, ld_dy=None, ld_w2=None, bits=(0, 0, 0, 0), order=0,
               exp=0, cus=256, ws_ok=1):
    out = (ctypes.c_long * 5)()
    st = _lib.lib().mxk_gemm_bf16_dgrad_swiglu_plan(M, F, K, K if ld_dy is None else ld_dy,
                                                    F if ld_w2 is None else ld_w2, *bits, mode, order,
                                                    exp, cus, ws_ok, out)
    return (st, None) if st else (0, dict(epi=out[0], order=out[1], stag=out[2], grid=out[3], cx=out[4]))


def test_dgrad_swiglu_plan():
    nwg = 2 * 4
    plain = lambda epi, order=0: (0, dict(epi=epi, order=order, stag=0, grid=nwg, cx=0))  # noqa: E731
    for exp in (0, 1):
        assert dgrad_plan(0, exp=exp) == plain(2)
        assert dgrad_plan(3, exp=exp) == plain(3)
        assert dgrad_plan(4, exp=exp) == plain(4)
        assert dgrad_plan(7, exp=exp) == plain(4)               # any other non-zero mode
        for mode in (0, 3, 4, 5, 6, 8):
            assert dgrad_plan(mode, K=64, exp=exp) == plain(2)            # one K-tile: the 8-B form
            assert dgrad_plan(mode, bits=(0, 0, 8, 0), exp=exp) == plain(2)   # gu at 8 mod 16
            assert dgrad_plan(mode, bits=(0, 0, 0, 8), exp=exp) == plain(2)   # dgu at 8 mod 16
    # a production build runs EPI 4 for 5 / 6 / 8 and ignores the order knob
    for mode in (5, 6, 8):
        assert dgrad_plan(mode, exp=0, order=1) == plain(4)
    assert dgrad_plan(3, exp=0, order=1) == plain(3)
    # experiments build
    assert dgrad_plan(5, exp=1) == plain(5) == dgrad_plan(5, exp=1, order=1)
    assert dgrad_plan(6, exp=1) == plain(6) == dgrad_plan(6, exp=1, order=1)
    assert dgrad_plan(4, exp=1, order=1) == plain(4, 1)
    assert dgrad_plan(3, exp=1, order=1) == plain(4, 1)         # B-outer wins over mode 3
    assert dgrad_plan(0, exp=1, order=1) == plain(2)
    # mode 8: 8 tiles on 256 CUs do not fit (fewer than two rounds per XCD) -> EPI 4
    assert dgrad_plan(8, exp=1) == plain(4)
    assert dgrad_plan(8, exp=1, order=1) == plain(4, 1)
    big = dict(M=4096, F=8192, K=256)                           # 512 tiles = 2 x 32 per XCD
    assert dgrad_plan(8, exp=1, **big) == (0, dict(epi=4, order=0, stag=1, grid=512 + 256, cx=32))
    assert dgrad_plan(8, exp=1, cus=240, **big) == (0, dict(epi=4, order=0, stag=1, grid=512 + 240, cx=30))
    assert dgrad_plan(8, exp=1, ws_ok=0, **big)[1] == dict(epi=4, order=0, stag=0, grid=512, cx=0)
    assert dgrad_plan(8, exp=1, **{**big, "K": 320})[1]["stag"] == 0       # K halves not whole K-tiles
    assert dgrad_plan(8, exp=1, **{**big, "M": 4096 - 256})[1]["stag"] == 0   # 480 tiles: < 2 rounds
    # a gu of more than 2^32 - 16 bytes: the g / u prefetch (EPI 4 / 6, STAG) would wrap its
    # 32-bit offset, so those plans run EPI 3 unstaggered; the 8-B form and EPI 5 stay
    over = dict(M=1 << 20)                                      # M * 2F * 2 = 2^32 with F = 1024
    huge = lambda epi: (0, dict(epi=epi, order=0, stag=0, grid=4096 * 4, cx=0))  # noqa: E731
    for exp in (0, 1):
        for mode in (3, 4, 6, 7, 8):
            for order in (0, 1):
                assert dgrad_plan(mode, exp=exp, order=order, **over) == huge(3), (mode, exp, order)
        assert dgrad_plan(0, exp=exp, **over) == huge(2)
        assert dgrad_plan(4, K=64, exp=exp, **over) == huge(2)
        assert dgrad_plan(4, bits=(0, 0, 8, 0), exp=exp, **over) == huge(2)
        assert dgrad_plan(5, exp=exp, **over) == huge(5 if exp else 3)
        under = dgrad_plan(4, M=(1 << 20) - 256, exp=exp)       # 256 KiB short of 4 GiB: as ever
        assert under == (0, dict(epi=4, order=0, stag=0, grid=4095 * 4, cx=0))
    assert dgrad_plan(8, exp=1, M=(1 << 20) - 512)[1]["stag"] == 1
    assert dgrad_plan(4, M=(1 << 22) + 256, F=256, K=128)[1]["epi"] == 3
    assert dgrad_plan(4, M=(1 << 22) - 256, F=256, K=128)[1]["epi"] == 4
    # the gate
    for kw in (dict(M=0), dict(F=0), dict(K=0), dict(M=500), dict(F=1000), dict(K=200), dict(ld_dy=260),
               dict(ld_w2=1028), dict(ld_dy=248), dict(ld_w2=1016), dict(bits=(8, 0, 0, 0)),
               dict(bits=(0, 8, 0, 0)), dict(bits=(0, 0, 4, 0)), dict(bits=(0, 0, 0, 4)),
               dict(K=1024, ld_w2=1 << 21)):
        assert dgrad_plan(4, **kw)[0] == 1, kw
    assert dgrad_plan(4, K=1024, ld_w2=(1 << 21) - 8)[0] == 0


@pytest.mark.parametrize("cus", [256, 240, 192, 4])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_ex_plan_invariants(layout, cus):
    """Over variants x tile counts x K, with the workspace a caller allocates
    for the whole chip: a planned split fits mxk_gemm_bf16_split_workspace()'s
    formula for `cus`, q_full + tail is the tile count, every grid is >= 1."""
    ws_formula = (cus // 2) * 2 * 256 * 256 * 4
    for variant, exp, tm, tn, K in itertools.product(range(5), (0, 1), (1, 2, 3, 6, 8, 17, 24, 56),
                                                     (1, 3, 16, 17), (64, 960, 1024, 1152, 4096)):
        st, p = ex_plan(layout, variant, M=tm * 256, N=tn * 256, K=K, cus=cus, exp=exp,
                        ws_bytes=(256 // 2) * 2 * 256 * 256 * 4)
        assert st == 0
        assert p["q_full"] + p["tail"] == tm * tn
        assert p["split"] == int(p["tail"] > 0)
        if p["split"]:
            assert variant == 1 and 2 * p["tail"] * 256 * 256 * 4 == p["ws"] <= ws_formula
            assert p["grid"] == p["q_full"] and 2 * p["tail"] >= 1
            assert (p["q_full"], p["tail"]) == gemm.split_plan(tm * tn, K, cus)
        else:
            assert p["grid"] >= 1 and (p["family"] == "x2t" or p["grid"] == tm * tn)
