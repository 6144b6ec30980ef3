"""The attention backward's plan (native/kernels/attention_plan.h): which
variant a layout resolves to and which kernel instances run, in which order.

Runs on the CPU: ``mxk_attn_bwd_plan`` is host arithmetic in the kernel
library (loaded, never launched).  The stage predicates below are written
from what each kernel needs, not from the header, so the sweep also checks the
fallback arms no GPU test can afford to run (a panel past 4 GiB)."""
import ctypes
import itertools

import pytest

from mxk8s.ops import _lib

pytestmark = pytest.mark.skipif(not _lib.kernels_available(), reason="kernel library not built")

# enum AttnDq / AttnDkdv, in the header's order
DQ = ["reg", "dma", "dma_pipe", "dma_pipe_unroll", "fold", "fold_rowc", "dq256", "atomics"]
DKDV = ["head", "gqa", "gqa_dma", "gqa_dma_pipe", "k256", "onepass_f32", "onepass_bf16"]
LIMIT = 1 << 32     # bytes a buffer resource addresses


def plan(variant, *, B=2, S=2048, Hq=32, Hkv=8, q_tok=None, k_tok=None, v_tok=None, dk_tok=None,
         dv_tok=None, causal=1):
    """(status, dict of the plan) for contiguous strides unless given."""
    q_tok = Hq * 128 if q_tok is None else q_tok
    k_tok = Hkv * 128 if k_tok is None else k_tok
    v_tok = Hkv * 128 if v_tok is None else v_tok
    dk_tok = Hkv * 128 if dk_tok is None else dk_tok
    dv_tok = Hkv * 128 if dv_tok is None else dv_tok
    out = (ctypes.c_long * 7)(*([-7] * 7))
    st = _lib.lib().mxk_attn_bwd_plan(B, S, Hq, Hkv, q_tok, k_tok, v_tok, dk_tok, dv_tok, causal,
                                      variant, out)
    if st:
        return st, None
    return 0, dict(variant=out[0], delta=out[1], dq=DQ[out[2]], dkdv=DKDV[out[3]], reduce=out[4],
                   dq_first=out[5], workspace=out[6])


def stages(p):
    return {k: p[k] for k in ("variant", "delta", "dq", "dkdv", "reduce", "dq_first")}


def want(variant, dq, dkdv, *, delta=0, dq_first=0, reduce=0):
    return dict(variant=variant, delta=delta, dq=dq, dkdv=dkdv, reduce=reduce, dq_first=dq_first)


BIG = 1 << 20       # token stride whose S = 2048 panel is exactly 4 GiB

# (requested variant, layout) -> resolved variant and stages, from the
# dispatcher this plan replaced
TABLE = [
    ((9, {}), want(9, "dq256", "k256", dq_first=1)),
    ((9, dict(Hq=4, Hkv=2, S=512)), want(6, "fold_rowc", "k256", dq_first=1)),
    ((6, {}), want(6, "fold_rowc", "k256", dq_first=1)),
    ((6, dict(S=384)), want(5, "fold", "gqa_dma_pipe", dq_first=1)),
    ((9, dict(S=384)), want(5, "fold", "gqa_dma_pipe", dq_first=1)),
    ((7, dict(S=384)), want(5, "fold", "gqa_dma_pipe", dq_first=1)),
    ((8, dict(S=384)), want(5, "fold", "gqa_dma_pipe", dq_first=1)),
    ((7, {}), want(7, "atomics", "onepass_f32")),
    ((8, {}), want(8, "atomics", "onepass_bf16")),
    ((5, {}), want(5, "fold", "gqa_dma_pipe", dq_first=1)),
    # K panel of 4 GiB: no LDS-DMA of K/V, so the dQ kernel stages through
    # registers and cannot fold delta in; the Q span still fits
    ((5, dict(k_tok=BIG)), want(5, "reg", "gqa_dma_pipe", delta=1)),
    ((9, dict(k_tok=BIG)), want(5, "reg", "gqa_dma_pipe", delta=1)),
    # Q panel of 4 GiB: the dK/dV kernel stages Q / dO through registers
    ((3, dict(q_tok=BIG)), want(3, "dma_pipe", "gqa", delta=1)),
    ((3, {}), want(3, "dma_pipe", "gqa_dma_pipe", delta=1)),
    ((4, {}), want(4, "dma_pipe_unroll", "gqa_dma_pipe", delta=1)),
    # the unrolled dQ body exists causal only: a non-causal 4 runs 3's
    ((4, dict(causal=0)), want(4, "dma_pipe", "gqa_dma_pipe", delta=1)),
    ((3, dict(causal=0)), want(3, "dma_pipe", "gqa_dma_pipe", delta=1)),
    ((2, {}), want(2, "dma", "gqa_dma", delta=1)),
    ((1, {}), want(1, "reg", "gqa", delta=1)),
    ((0, {}), want(0, "reg", "head", delta=1, reduce=1)),
]


@pytest.mark.parametrize("req,expect", TABLE, ids=[f"v{r[0]}-{r[1]}" for r, _ in TABLE])
def test_resolution_table(req, expect):
    st, p = plan(req[0], **req[1])
    assert st == 0
    assert stages(p) == expect


def _workspace(B, S, Hq, variant):
    return _lib.lib().mxk_attn_bwd_workspace_variant(B, S, Hq, variant)


def test_workspace_bytes():
    B, S, Hq = 2, 2048, 32
    rows = B * Hq * S
    for v in range(10):
        exp = {0: rows * 4 + 2 * rows * 128 * 4, 6: rows * 8, 7: rows * 8 + rows * 128 * 4,
               8: rows * 8, 9: rows * 8}.get(v, rows * 4)
        assert _workspace(B, S, Hq, v) == exp, v
    assert _lib.lib().mxk_attn_bwd_onepass_workspace(B, S, Hq, 0) == _workspace(B, S, Hq, 7)
    assert _lib.lib().mxk_attn_bwd_onepass_workspace(B, S, Hq, 1) == _workspace(B, S, Hq, 8)


@pytest.mark.parametrize("variant", range(10))
def test_every_stage_takes_its_layout(variant):
    for S, grp, (kv_big, q_big), causal in itertools.product(
            [128, 256, 384, 512, 2048], [1, 2, 4, 8], itertools.product([0, 1], repeat=2), [0, 1]):
        Hkv = 2
        Hq = Hkv * grp
        big = -(-(LIMIT // 2) // S)      # smallest stride with S * stride * 2 >= 2^32 ...
        big += -big % 8                  # ... that is a multiple of 8
        q_tok = big if q_big else Hq * 128
        k_tok = v_tok = big if kv_big else Hkv * 128
        st, p = plan(variant, B=1, S=S, Hq=Hq, Hkv=Hkv, q_tok=q_tok, k_tok=k_tok, v_tok=v_tok,
                     causal=causal)
        where = (variant, S, grp, kv_big, q_big, causal, p)
        assert st == 0, where
        assert p["variant"] <= variant or (variant in (7, 8) and p["variant"] == 5), where
        assert _workspace(1, S, Hq, variant) >= p["workspace"], where
        assert p["workspace"] == _workspace(1, S, Hq, p["variant"]), where

        def fits(tok):
            return S * tok * 2 < LIMIT
        kv_span = fits(max(k_tok, v_tok))
        q_span = fits(max(q_tok, Hq * 128))
        k256 = S % 256 == 0 and fits(q_tok) and fits(k_tok) and fits(Hq * 128)
        dq, dkdv = p["dq"], p["dkdv"]
        if dq == "dq256":
            assert S % 64 == 0 and grp % 4 == 0 and fits(k_tok) and fits(v_tok), where
        if dq in ("dma", "dma_pipe", "dma_pipe_unroll", "fold", "fold_rowc"):
            assert kv_span, where
        if dq == "dma_pipe_unroll":
            assert causal, where
        if dkdv in ("gqa_dma", "gqa_dma_pipe"):
            assert q_span, where
        if dkdv in ("k256", "onepass_f32", "onepass_bf16"):
            assert k256, where
        # who writes what the dK/dV kernel reads: the rowc pairs by a dQ kernel
        # that runs first, delta by that or by the delta kernel, never both
        assert (dkdv == "k256") == (dq in ("fold_rowc", "dq256")), where
        assert (dq == "atomics") == dkdv.startswith("onepass"), where
        if dq == "atomics":
            assert not (p["delta"] or p["dq_first"] or p["reduce"]), where
        else:
            assert p["dq_first"] == (dq in ("fold", "fold_rowc", "dq256")), where
            assert p["delta"] == (not p["dq_first"]), where
            assert p["reduce"] == (dkdv == "head"), where


@pytest.mark.parametrize("bad", [
    dict(S=192), dict(S=64), dict(Hq=32, Hkv=5), dict(Hkv=0), dict(B=0), dict(q_tok=4100),
    dict(k_tok=1028), dict(v_tok=1028), dict(dk_tok=1026), dict(dv_tok=1026)],
    ids=lambda b: "-".join(f"{k}{v}" for k, v in b.items()))
def test_rejects_what_the_entry_check_rejects(bad):
    for variant in (0, 5, 9):
        assert plan(variant, **bad)[0] == 1     # hipErrorInvalidValue


def test_rejects_unknown_variants():
    assert plan(-1)[0] == 1 and plan(10)[0] == 1
