"""Stochastic rounding of the MXFP4 gradient quantisers, everything that needs
no GPU: Philox4x32-10, the reference quantiser's properties and its freedom from
bias, ``linear_mxfp4(.., "stochastic")`` against its products written out by
hand, the seed source, the model and trainer wiring, the library signatures,
the host sweep of the C++ arithmetic and build hygiene of the kernels.

Tiny Llama, reference emulation on the CPU (fp32 model, MXFP4 linears with
stochastic gradient rounding; model seeds 0-3, seed-source seeds 0 and 1)
against the fp32 model: the loss equals the round-to-nearest emulation's bit
for bit and the worst gradient cosine is 0.839-0.858 (round-to-nearest on the
same models: 0.850-0.871; ``test_mxfp4_linear_cpu.py`` quotes 0.844-0.867 and
sets its floor of 0.7, 0.144 below its lowest figure).  ``test_gpu_mxfp4_sr.py``
keeps that margin under the lowest figure here: 0.839 - 0.144 = 0.695."""
import ctypes
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import mx_gemm_checks as mx
import mx_linear_checks as lc
import mx_sr_checks as sr
from mx_linear_checks import no_library  # noqa: F401  (fixture)
from mxk8s.models.llama import Llama, LlamaConfig
from mxk8s.ops import _lib
from mxk8s.ops import mxfp4 as MX4
from mxk8s.ops._philox import philox4x32_10
from mxk8s.ops.linear import Linear, SwiGLULinear, linear_mxfp4
from mxk8s.ops.mxfp4 import (dequantize_mxfp4, quantize_mxfp4, quantize_mxfp4_dual, quantize_mxfp4_ref,
                             quantize_mxfp4_t, sr_next, sr_reseed)

REPO = mx.REPO
M64 = sr.M64


# ---- Philox ---------------------------------------------------------------------------
KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
          (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers():
    for ctr, key, want in KNOWN:
        assert philox4x32_10(ctr, key).tolist() == list(want)
    # vectorised: the three at once, and a broadcast key
    ctr = [np.array([k[0][w] for k in KNOWN]) for w in range(4)]
    key = [np.array([k[1][w] for k in KNOWN]) for w in range(2)]
    assert philox4x32_10(ctr, key).tolist() == [list(k[2]) for k in KNOWN]
    out = philox4x32_10((np.arange(5)[:, None], np.arange(3)[None, :], 0, 0), (7, 9))
    assert out.shape == (5, 3, 4) and out.dtype == np.uint32
    assert out[4, 2].tolist() == philox4x32_10((4, 2, 0, 0), (7, 9)).tolist()
    with pytest.raises(ValueError):
        philox4x32_10((2 ** 32, 0, 0, 0), (0, 0))


# ---- basic properties of the reference ------------------------------------------------
def _spread(R, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((R, K), generator=g) *
            torch.exp2(torch.randint(-8, 8, (R, K), generator=g).float())).bfloat16()


def _gap_units(q):
    """Per element, the distance between the two neighbours of its code's cell in
    units of the block scale, an upper bound (2) taken where the code is 7."""
    code = torch.stack((q & 7, (q >> 4) & 7), dim=2).reshape(q.shape[0], -1)
    return torch.tensor([0.5, 0.5, 0.5, 0.5, 1.0, 1.0, 2.0, 2.0])[code.long()]


def test_grid_input_is_fixed_for_every_seed(no_library):  # noqa: F811
    x = sr.grid_tensor(64, 96, 5)
    assert torch.equal(sr.deq(sr.ref(x)), x.double())        # on the grid of round-to-nearest too
    for seed in (0, 1, M64 - 1):
        q, s, qt, st = quantize_mxfp4_dual(x, "stochastic", seed)
        assert torch.equal(dequantize_mxfp4(q, s), x.float())
        assert torch.equal(dequantize_mxfp4(qt, st), x.t().float())
        assert not ((q & 0xF) == 8).any() and not ((q >> 4) == 8).any()   # -0 is never produced


def test_scales_are_the_non_clipping_rule_and_nothing_is_clipped(no_library):  # noqa: F811
    x = lc._wide(33, 256, 7, lo=-130, hi=125)
    x[0, :32] = 0
    x[1, 32:64] = torch.tensor([6.5] + [0.0] * 31).bfloat16()        # RNE scales 6.5 by 2^0, SR by 2^1
    want = sr.noclip_scales(x)
    assert want[0, 0] == 127 and want[1, 1] == 128 and quantize_mxfp4_ref(x)[1][1, 1] == 127
    for seed in (0, 3, M64 - 1):
        q, s = quantize_mxfp4_ref(x, "stochastic", seed)
        assert torch.equal(s, want)
        unit = torch.exp2(s.double() - 127).repeat_interleave(32, 1)
        err = (dequantize_mxfp4(q, s).double() - x.double()).abs() / unit
        assert (err < _gap_units(q)).all() and (err < 2).all()
    # always one of the two neighbours: never farther than the cell is wide, so
    # with u = 0 .. the result brackets x; checked against both neighbours of |x| / unit
    a = (x.double().abs() / unit)
    grid = torch.tensor(sr.E2M1, dtype=torch.float64)
    lo = grid[(a.unsqueeze(-1) >= grid).sum(-1) - 1]
    hi = grid[((a.unsqueeze(-1) > grid).sum(-1)).clamp(max=7)]
    got = dequantize_mxfp4(q, s).double().abs() / unit
    assert ((got == lo) | (got == hi)).all()


def test_same_seed_same_bytes_other_seed_other_bytes(no_library):  # noqa: F811
    x = _spread(64, 256, 8)
    a, b, c = (quantize_mxfp4(x, "stochastic", s) for s in (11, 11, 12))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[1], c[1]) and not torch.equal(a[0], c[0])
    assert not torch.equal(a[0], quantize_mxfp4(x)[0])


@pytest.mark.parametrize("R,C", [(32, 1), (96, 3), (64, 100), (256, 32)])
def test_t_is_the_rows_form_of_the_transposed_copy(no_library, R, C):  # noqa: F811
    x = lc._wide(R, C, 13 + R)
    for seed in (0, M64 - 1):
        qt, st = quantize_mxfp4_t(x, "stochastic", seed)
        qr, s_r = quantize_mxfp4_ref(x.t().contiguous(), "stochastic", seed)
        assert torch.equal(qt, qr) and torch.equal(st, s_r)


def test_dual_is_rows_with_the_seed_and_t_with_the_next(no_library):  # noqa: F811
    x = lc._wide(96, 64, 14)
    for seed in (4, M64 - 1):                                 # the second wraps to 0
        q, s, qt, st = quantize_mxfp4_dual(x, "stochastic", seed)
        q1, s1 = quantize_mxfp4(x, "stochastic", seed)
        q2, s2 = quantize_mxfp4_t(x, "stochastic", (seed + 1) % M64)
        assert torch.equal(q, q1) and torch.equal(s, s1) and torch.equal(qt, q2) and torch.equal(st, s2)


@pytest.mark.parametrize("dev", ["cpu", "meta"])
def test_rounding_arguments_raise_before_the_library(no_library, dev):  # noqa: F811
    x = torch.zeros((32, 32), dtype=torch.bfloat16, device=dev)
    for fn in (quantize_mxfp4_ref, quantize_mxfp4, quantize_mxfp4_t, quantize_mxfp4_dual):
        for bad in [dict(rounding="stochastic"), dict(rounding="stochastic", seed=-1),
                    dict(rounding="stochastic", seed=M64), dict(rounding="stochastic", seed=1.0),
                    dict(rounding="stochastic", seed=True), dict(rounding="random", seed=1),
                    dict(rounding="nearest", seed=1)]:
            with pytest.raises(ValueError):
                fn(x, **bad)
    assert torch.equal(quantize_mxfp4(torch.zeros((32, 32), dtype=torch.bfloat16), "nearest")[1],
                       torch.full((32, 1), 127, dtype=torch.uint8))


# ---- unbiased ---------------------------------------------------------------------------
def test_unbiased_per_element(no_library):  # noqa: F811
    """|mean over N = 1024 seeds of dequant - x| <= 6 gap_max 2^e / (2 sqrt(N)) with
    gap_max = 2: every draw lies within one cell of width <= gap_max 2^e, so this
    is Hoeffding's bound at 6 sigma, failure probability below 2 e^-18 per element
    and about 5e-4 for the 16384 elements.  Measured: max 0.09 in units of 2^e
    against the bound 0.1875; round-to-nearest on the same tensor reaches 1.0 in
    these units (those of the non-clipping scale), the clamp at 6."""
    x = _spread(64, 256, 9)
    N = 1024
    total = torch.zeros(x.shape, dtype=torch.float64)
    for seed in range(N):
        q, s = quantize_mxfp4_ref(x, "stochastic", seed)
        total += dequantize_mxfp4(q, s).double()
    unit = torch.exp2(s.double() - 127).repeat_interleave(32, 1)      # the same for every seed
    bound = 6 * 2 / (2 * N ** 0.5)
    bias = ((total / N - x.double()).abs() / unit).max().item()
    rne = ((dequantize_mxfp4(*quantize_mxfp4_ref(x)).double() - x.double()).abs() / unit).max().item()
    print("max bias / 2^e", bias, "bound", bound, "round-to-nearest", rne)
    assert bias <= bound
    assert rne > bound


def test_unbiased_gradients(no_library):  # noqa: F811
    """dx and dW from the mean of N = 16 stochastic draws of dy's images: the
    error norm falls as 1/sqrt(N) (0.25 of round-to-nearest's; asserted < 0.5)
    and its projection on the true product is noise (|.| < 0.01) where
    round-to-nearest's is a shrinkage of 7.8 % (asserted < -0.05)."""
    res = sr.gradient_errors(256, 256, 256, 31, [1000 + 2 * n for n in range(16)])
    for k, (rne_err, mean_err, rne_proj, mean_proj) in res.items():
        print(k, "error ratio", mean_err / rne_err, "projections", rne_proj, mean_proj)
        assert mean_err < 0.5 * rne_err
        assert abs(mean_proj) < 0.01
        assert rne_proj < -0.05


# ---- linear_mxfp4 on the CPU -----------------------------------------------------------
def _by_hand_sr(x, w, dy, seed):
    """y, dx, dW from reference images: dy's rows with seed, its columns with seed + 1."""
    mm = lambda a, b: (dequantize_mxfp4(*a) @ dequantize_mxfp4(*b).t()).bfloat16()   # noqa: E731
    return (mm(sr.ref(x), sr.ref(w)), mm(sr.ref(dy, seed), sr.ref(w.t())),
            mm(sr.ref(dy.t(), (seed + 1) % M64), sr.ref(x.t())))


@pytest.mark.parametrize("seed", [6, M64 - 1])
def test_linear_stochastic_equals_the_products_by_hand(no_library, seed):  # noqa: F811
    T, i, o = 256, 256, 256
    x, w, dy = lc.operands(T, i, o, 21)
    ry, rdx, rdw = _by_hand_sr(x, w, dy, seed)
    xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = linear_mxfp4(xg, wg, "stochastic", seed=seed)
    y.backward(dy)
    assert torch.equal(y.detach(), linear_mxfp4(x, w)) and torch.equal(y.detach(), ry)
    assert torch.equal(xg.grad, rdx) and torch.equal(wg.grad, rdw)
    assert not torch.equal(xg.grad, lc.by_hand(lc.MXFP4, x, w, dy)[1])
    # one gradient alone equals the dual's
    xg = x.clone().requires_grad_()
    linear_mxfp4(xg, w, "stochastic", seed=seed).backward(dy)
    assert torch.equal(xg.grad, rdx)
    wg = w.clone().requires_grad_()
    linear_mxfp4(x, wg, grad_rounding="stochastic", seed=seed).backward(dy)
    assert torch.equal(wg.grad, rdw)


def test_linear_draws_its_seed_at_forward_time_in_call_order(no_library):  # noqa: F811
    T, i, o = 256, 256, 256
    x, w, dy = lc.operands(T, i, o, 22)
    sr_reseed(77, rank=1, step=3)
    s0, s1 = sr_next(), sr_next()
    sr_reseed(77, rank=1, step=3)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    ya = linear_mxfp4(xa, w, "stochastic")                    # draw 0
    yb = linear_mxfp4(xb, w, "stochastic")                    # draw 1
    sr_reseed(5)                                              # nothing is drawn in the backward
    yb.backward(dy)                                           # and its order does not matter
    ya.backward(dy)
    assert sr_next() == _first_draw(5)
    assert torch.equal(xa.grad, _by_hand_sr(x, w, dy, s0)[1])
    assert torch.equal(xb.grad, _by_hand_sr(x, w, dy, s1)[1])
    with pytest.raises(ValueError):
        linear_mxfp4(x, w, "nearest", seed=1)
    with pytest.raises(ValueError):
        linear_mxfp4(x, w, "stochastic", seed=-1)
    with pytest.raises(ValueError):
        linear_mxfp4(x, w, "random")


def test_nearest_calls_keep_one_positional_argument(no_library, monkeypatch):  # noqa: F811
    """With grad_rounding unset the quantiser calls are what they were."""
    lc.dy_is_read_once_when_both_gradients_are_needed(lc.MXFP4, monkeypatch)


# ---- seed source ------------------------------------------------------------------------
def _first_draw(seed, rank=0, step=0, n=0):
    w = philox4x32_10((n, step & 0xFFFFFFFF, step >> 32, rank), (seed & 0xFFFFFFFF, seed >> 32))
    return ((int(w[1]) << 32) | int(w[0])) & ~1


def test_seed_source_is_deterministic_even_and_restarts():
    sr_reseed(0)
    assert sr_next() == 0xe169c58d6627e8d4                    # the first known answer, bit 0 cleared
    sr_reseed(123, rank=2, step=2 ** 40 + 5)
    a = [sr_next() for _ in range(4)]
    assert a == [_first_draw(123, 2, 2 ** 40 + 5, n) for n in range(4)]
    assert all(v % 2 == 0 and 0 <= v < M64 for v in a) and len(set(a)) == 4
    sr_reseed(123, rank=2, step=2 ** 40 + 5)
    assert [sr_next() for _ in range(4)] == a
    for bad in [(-1, 0, 0), (M64, 0, 0), (0, 2 ** 32, 0), (0, 0, M64), (0.0, 0, 0)]:
        with pytest.raises(ValueError):
            sr_reseed(*bad)
    sr_reseed(0)


def test_seed_source_draws_are_distinct_over_rank_step_and_n():
    """10^5 draws over a grid of (rank, step, n), all distinct (63 random bits
    each: a collision has probability ~5e-10)."""
    rank, step, n = np.meshgrid(np.arange(10), np.arange(100), np.arange(100), indexing="ij")
    w = philox4x32_10((n, step, 0, rank), (42, 0)).astype(np.uint64)
    draws = ((w[..., 1] << np.uint64(32)) | w[..., 0]) & ~np.uint64(1)
    assert np.unique(draws).size == 100000
    sr_reseed(42, rank=7, step=99)
    for _ in range(56):
        sr_next()
    assert sr_next() == int(draws[7, 99, 56])
    sr_reseed(0)


# ---- config, layers and trainer -----------------------------------------------------------
def test_config_and_layer_validation():
    assert LlamaConfig().grad_rounding == "nearest" and Linear(256, 256).grad_rounding == "nearest"
    assert LlamaConfig(linear_dtype="mxfp4", grad_rounding="stochastic").grad_rounding == "stochastic"
    assert Linear(256, 256, compute="mxfp4", grad_rounding="stochastic").grad_rounding == "stochastic"
    assert SwiGLULinear(256, 256, compute="mxfp4", grad_rounding="stochastic").grad_rounding == "stochastic"
    assert Linear.COMPUTE == ("bf16", "mxfp8", "mxfp4")
    for dtype in ("bf16", "mxfp8"):
        with pytest.raises(ValueError):
            LlamaConfig(linear_dtype=dtype, grad_rounding="stochastic")
        with pytest.raises(ValueError):
            Linear(256, 256, compute=dtype, grad_rounding="stochastic")
    with pytest.raises(ValueError):
        LlamaConfig(linear_dtype="mxfp4", grad_rounding="random")
    with pytest.raises(ValueError):
        Linear(256, 256, compute="mxfp4", grad_rounding="random")
    cfg = LlamaConfig.tiny()
    cfg.linear_dtype, cfg.grad_rounding = "mxfp4", "stochastic"
    for layer in Llama(cfg).layers:
        assert [m.grad_rounding for m in (layer.attn.wqkv, layer.attn.wo, layer.mlp.w13,
                                          layer.mlp.w2)] == ["stochastic"] * 4


def test_layers_draw_in_module_order_and_swiglu_passes_through(no_library):  # noqa: F811
    from mxk8s.ops.fused import swiglu
    torch.manual_seed(4)
    a = Linear(256, 256, compute="mxfp4", grad_rounding="stochastic").bfloat16()
    b = SwiGLULinear(256, 256, compute="mxfp4", grad_rounding="stochastic").bfloat16()
    x = torch.randn(256, 256).bfloat16().requires_grad_()
    gu = torch.randn(256, 512).bfloat16().requires_grad_()
    dy = torch.randn(256, 256).bfloat16()
    sr_reseed(9)
    s0, s1 = sr_next(), sr_next()
    sr_reseed(9)
    ya, yb = a(x), b(gu)
    (ya + yb).backward(dy)
    xr = x.detach().clone().requires_grad_()
    linear_mxfp4(xr, a.weight.detach(), "stochastic", seed=s0).backward(dy)
    gr = gu.detach().clone().requires_grad_()
    linear_mxfp4(swiglu(gr), b.weight.detach(), "stochastic", seed=s1).backward(dy)
    assert torch.equal(x.grad, xr.grad) and torch.equal(gu.grad, gr.grad)
    # a shape outside the MX tiling takes the bf16 path and draws nothing
    a(torch.randn(100, 256).bfloat16())
    assert sr_next() == _first_draw(9, n=2)
    sr_reseed(0)


def _trainer(monkeypatch, argv=None, env=None, ns=None):
    """(cfg, sr seed the step loop reseeds with) as the trainer resolves them."""
    import mxk8s.train.ddp_llama as D
    seen = {}

    class Stop(Exception):
        pass

    def fake_build(cfg, *a, **k):
        seen["cfg"] = cfg
        raise Stop

    monkeypatch.setattr(D, "build", fake_build)
    lc._trainer_env(monkeypatch, env)
    for k in ("MXK_GRAD_ROUNDING", "MXK_SR_SEED"):
        if k not in (env or {}):
            monkeypatch.delenv(k, raising=False)
    with pytest.raises(Stop):
        if ns is not None:
            D.run_ddp_bench(ns)
        else:
            D.main(argv)
    return seen["cfg"]


FP4 = lc.TINY_ARGV + ["--linear-dtype", "mxfp4"]


def test_trainer_flag_and_environment_precedence(monkeypatch):
    import mxk8s.train.ddp_llama as D
    assert _trainer(monkeypatch, FP4).grad_rounding == "nearest"
    assert _trainer(monkeypatch, FP4 + ["--grad-rounding", "stochastic"]).grad_rounding == "stochastic"
    assert _trainer(monkeypatch, FP4, env={"MXK_GRAD_ROUNDING": "stochastic"}).grad_rounding == "stochastic"
    assert _trainer(monkeypatch, FP4 + ["--grad-rounding", "nearest"],
                    env={"MXK_GRAD_ROUNDING": "stochastic"}).grad_rounding == "nearest"
    assert _trainer(monkeypatch, FP4 + ["--grad-rounding", "stochastic"],
                    env={"MXK_GRAD_ROUNDING": "nearest"}).grad_rounding == "stochastic"
    # bench.py's namespace has neither attribute: the environment decides
    cfg = _trainer(monkeypatch, ns=lc.bench_namespace(),
                   env={"MXK_LINEAR_DTYPE": "mxfp4", "MXK_GRAD_ROUNDING": "stochastic"})
    assert (cfg.linear_dtype, cfg.grad_rounding) == ("mxfp4", "stochastic")
    assert _trainer(monkeypatch, ns=lc.bench_namespace()).grad_rounding == "nearest"
    # stochastic without the MXFP4 layers, and unknown values, are errors
    lc._trainer_env(monkeypatch)
    for argv in (lc.TINY_ARGV + ["--grad-rounding", "stochastic"],
                 lc.TINY_ARGV + ["--linear-dtype", "mxfp8", "--grad-rounding", "stochastic"]):
        with pytest.raises(ValueError):
            D.main(argv)
    lc._trainer_env(monkeypatch, {"MXK_GRAD_ROUNDING": "random"})
    with pytest.raises(ValueError):
        D.main(FP4)
    # the seed: flag over environment over 0
    ns = lambda **k: __import__("types").SimpleNamespace(**k)   # noqa: E731
    monkeypatch.delenv("MXK_SR_SEED", raising=False)
    assert D.resolve_sr_seed(ns()) == 0
    monkeypatch.setenv("MXK_SR_SEED", "17")
    assert D.resolve_sr_seed(ns()) == 17 and D.resolve_sr_seed(ns(sr_seed=3)) == 3
    assert D.resolve_sr_seed(ns(sr_seed=0)) == 0
    with pytest.raises(ValueError):
        D.resolve_sr_seed(ns(sr_seed=-1))


SR_ARGV = ["--tiny", "--seq-len", "128", "--micro-batch", "2", "--bucket-mb", "1", "--linear-dtype",
           "mxfp4", "--grad-rounding", "stochastic", "--sr-seed", "5"]


def _params(model):
    return torch.cat([p.detach().float().flatten() for p in model.parameters()])


def test_trainer_reseeds_every_step_with_the_global_step(monkeypatch, capsys):
    """One warm-up and one timed step in one go leave the parameters of step 0,
    sr_reseed(5, 0, 1), step 1 by hand; without the second reseed they differ."""
    import mxk8s.train.ddp_llama as D
    lc._trainer_env(monkeypatch)
    made = []
    real_build = D.build
    monkeypatch.setattr(D, "build", lambda *a, **k: made.append(real_build(*a, **k)) or made[-1])
    reseeds = []
    real_reseed = MX4.sr_reseed
    monkeypatch.setattr(MX4, "sr_reseed", lambda *a: reseeds.append(a) or real_reseed(*a))
    torch.manual_seed(0)
    assert D.main(SR_ARGV + ["--steps", "1", "--warmup", "1"]) == 0
    out = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    assert out["grad_rounding"] == "stochastic" and out["linear_dtype"] == "mxfp4"
    assert out["mean_loss"] == out["mean_loss"]
    assert reseeds == [(5, 0, 0), (5, 0, 1)]
    in_one_go = _params(made[0][0])

    def by_hand(reseed_step_1):
        cfg = LlamaConfig.tiny()
        cfg.linear_dtype, cfg.grad_rounding = "mxfp4", "stochastic"
        torch.manual_seed(0)
        model, ddp, opt = real_build(cfg, torch.device("cpu"), 1.0)
        g = torch.Generator().manual_seed(1000)
        batches = [torch.randint(0, cfg.vocab_size, (2, 129), generator=g) for _ in range(4)]
        real_reseed(5, 0, 0)
        D.train_step(model, ddp, opt, batches[0])
        if reseed_step_1:
            real_reseed(5, 0, 1)
        D.train_step(model, ddp, opt, batches[1])
        return _params(model)

    assert torch.equal(in_one_go, by_hand(True))
    assert not torch.equal(in_one_go, by_hand(False))
    real_reseed(0)


def test_trainer_reports_nearest_by_default(monkeypatch, capsys):
    import mxk8s.train.ddp_llama as D
    lc._trainer_env(monkeypatch)
    monkeypatch.delenv("MXK_GRAD_ROUNDING", raising=False)
    drawn = []
    monkeypatch.setattr(MX4, "sr_next", lambda: drawn.append(1) or 0)
    assert D.main(lc.TINY_ARGV + ["--bucket-mb", "1", "--linear-dtype", "mxfp4"]) == 0
    out = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    assert out["grad_rounding"] == "nearest" and drawn == []


# ---- tiny model: the emulation's figures ---------------------------------------------------
def test_tiny_model_loss_is_the_nearest_loss_and_gradients_follow_the_fp32_model(no_library):  # noqa: F811
    """The forward is untouched, so the loss is the round-to-nearest MXFP4
    model's bit for bit; every gradient is finite with a cosine >= 0.7 against
    the fp32 model's (the module docstring has the measured figures)."""
    ref_model, tok, _ = lc.fp32_reference()
    m_sr, loss_sr = sr.sr_model_run(ref_model, tok, "cpu", "stochastic")
    _, loss_rne = sr.sr_model_run(ref_model, tok, "cpu", "nearest")
    assert torch.equal(loss_sr, loss_rne)
    worst = sr.min_cosine(ref_model, m_sr)
    print("worst cosine", worst)
    assert worst >= 0.7


# ---- library signatures ------------------------------------------------------------------
def test_library_signatures_carry_the_seed_before_the_stream():
    S = _lib._SIGNATURES
    for sfx in ("", "_t", "_dual"):
        res, args = S["mxk_quantize_mxfp4_sr" + sfx]
        rne = S["mxk_quantize_mxfp4" + sfx][1]
        assert res is ctypes.c_int
        assert args == rne[:-1] + [ctypes.c_uint64, ctypes.c_void_p] and rne[-1] is ctypes.c_void_p


# ---- host sweep and build hygiene ------------------------------------------------------------
def test_host_sweep_of_the_stochastic_arithmetic():
    """make test-mxfp4-sr: the Philox known answers, block_exp_noclip over every
    bf16 block maximum and f32_to_e2m1_sr over every bf16 in [-6, 6], under
    ASan + UBSan."""
    p = subprocess.run(["make", "-C", REPO, "test-mxfp4-sr"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert "all as defined" in p.stdout


@pytest.mark.skipif(not mx.HIPCC, reason="no hipcc")
def test_sr_kernels_are_six_without_scratch_or_spills():
    """quantize_mxfp4_sr.hip compiles to the 2 row and 4 transposing
    instantiations on E2m1Sr and nothing else; zero scratch and zero spills, read
    from the kernel metadata as mx_gemm_checks.kernel_listing reads it."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "m.s")
        subprocess.run([mx.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17",
                        "-I" + os.path.join(REPO, "native", "kernels"), "--cuda-device-only", "-S",
                        os.path.join(REPO, "native", "kernels", "quantize_mxfp4_sr.hip"), "-o", out],
                       check=True, capture_output=True)
        with open(out) as fh:
            asm = fh.read()
    by = {}
    kernels = asm[asm.index("amdhsa.kernels:"):]
    for entry in kernels[:kernels.index("\namdhsa.")].split("\n  - ")[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", entry).group(1)
        by[name] = {k: int(re.search(r"\n    \.%s:\s+(\d+)" % k, entry).group(1)) for k in mx._META}
    assert len(by) == 6 and all("E2m1Sr" in n for n in by), sorted(by)
    assert sum("quantize_rows_kernel" in n for n in by) == 2
    assert sum("quantize_tr_kernel" in n for n in by) == 4
    assert all(v == 0 for m in by.values() for v in m.values()), by
