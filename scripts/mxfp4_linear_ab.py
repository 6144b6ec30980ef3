#!/usr/bin/env python3
"""A/B of the pieces of the MXFP4 linear path, in one process (BASELINE.md
protocol): >= 2 s warm-up of every side, then blocks of event-timed calls
going round the sides, medians.  One JSON line per case; beside every median
the lowest and highest block median of that side, the run's own block-to-block
spread.

  quantiser   quantize_mxfp4_t(x) against quantize_mxfp4(x.t().contiguous()),
              quantize_mxfp4_dual(x) against quantize_mxfp4(x) +
              quantize_mxfp4(x.t().contiguous()), and quantize_mxfp8_t /
              quantize_mxfp8_dual beside them; ms and effective GB/s (the
              bytes one pass needs: 2 B read per element, 1/2 B + 1/32 B
              written per MXFP4 image, 1 B + 1/32 B per MXFP8 image).
              --variant-lib PATH adds the two MXFP4 entry points of another
              build of the kernel library (scripts/build_variant_lib.sh) as
              further sides.
  layer       forward + backward of Linear at 16384 tokens, compute="bf16",
              "mxfp8" and "mxfp4" with every quantiser launch included

    python scripts/mxfp4_linear_ab.py [--what quantiser,layer] [--iters 40] [--block 5]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mxk8s.ops import (_lib, quantize_mxfp4, quantize_mxfp4_dual, quantize_mxfp4_t,  # noqa: E402
                       quantize_mxfp8_dual, quantize_mxfp8_t)
from mxk8s.ops.linear import Linear  # noqa: E402

QUANT_SHAPES = [(16384, 4096), (16384, 14336), (14336, 4096)]
LAYER_SHAPES = [(4096, 6144), (4096, 4096), (4096, 28672), (14336, 4096)]   # in -> out
TOKENS = 16384


def timed(fn, n):
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def ab(sides, warmup_s, iters, block):
    """{name: (median ms, lowest block median, highest block median)} of the
    callables in ``sides``: warm-up of all, then blocks going round them."""
    t0 = time.time()
    while time.time() - t0 < warmup_s:
        for fn in sides.values():
            fn()
        torch.cuda.synchronize()
    ts = {k: [] for k in sides}
    blocks = {k: [] for k in sides}
    while len(next(iter(ts.values()))) < iters:
        for k, fn in sides.items():
            b = timed(fn, block)
            ts[k] += b
            blocks[k].append(statistics.median(b))
    return {k: (statistics.median(ts[k]), min(blocks[k]), max(blocks[k])) for k in sides}


def _fields(name, r, nbytes=None):
    med, lo, hi = r
    d = {name + "_ms": round(med, 4), name + "_block_ms": [round(lo, 4), round(hi, 4)]}
    if nbytes is not None:
        d[name + "_gbps"] = round(nbytes / med / 1e6, 1)
    return d


def _variant(path):
    """quantize_mxfp4_t / _dual on the entry points of another library build."""
    h = ctypes.CDLL(path)
    for name in ("mxk_quantize_mxfp4_t", "mxk_quantize_mxfp4_dual"):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _lib._SIGNATURES[name]

    def t(x):
        R, C = x.shape
        qt = torch.empty((C, R // 2), dtype=torch.uint8, device=x.device)
        st = torch.empty((C, R // 32), dtype=torch.uint8, device=x.device)
        _lib.check(h.mxk_quantize_mxfp4_t(x.data_ptr(), qt.data_ptr(), st.data_ptr(), R, C, x.stride(0),
                                          qt.stride(0), st.stride(0), _lib.stream_ptr(x.device)),
                   "variant mxk_quantize_mxfp4_t")
        return qt, st

    def dual(x):
        R, C = x.shape
        q = torch.empty((R, C // 2), dtype=torch.uint8, device=x.device)
        s = torch.empty((R, C // 32), dtype=torch.uint8, device=x.device)
        qt = torch.empty((C, R // 2), dtype=torch.uint8, device=x.device)
        st = torch.empty((C, R // 32), dtype=torch.uint8, device=x.device)
        _lib.check(h.mxk_quantize_mxfp4_dual(x.data_ptr(), q.data_ptr(), s.data_ptr(), qt.data_ptr(),
                                             st.data_ptr(), R, C, x.stride(0), q.stride(0), s.stride(0),
                                             qt.stride(0), st.stride(0), _lib.stream_ptr(x.device)),
                   "variant mxk_quantize_mxfp4_dual")
        return q, s, qt, st

    return t, dual


def quantiser(args, dev):
    var = _variant(args.variant_lib) if args.variant_lib else None
    for R, C in QUANT_SHAPES:
        g = torch.Generator(device=dev)
        g.manual_seed(R + C)
        x = (torch.rand((R, C), device=dev, generator=g) * 2 - 1).bfloat16()
        n = R * C
        img4, img8 = n // 2 + n // 32, n + n // 32
        if var is not None:                                   # the two builds agree, byte for byte
            for a, b in zip(quantize_mxfp4_dual(x), var[1](x)):
                assert torch.equal(a, b)
        sides = {"t": lambda: quantize_mxfp4_t(x),
                 "transpose_then_quantize": lambda: quantize_mxfp4(x.t().contiguous()),
                 "mxfp8_t": lambda: quantize_mxfp8_t(x)}
        if var is not None:
            sides["variant_t"] = lambda: var[0](x)
        r = ab(sides, args.warmup_s, args.iters, args.block)
        out = {"case": "quantize_t", "R": R, "C": C, "block": args.block}
        out.update(_fields("t", r["t"], 2 * n + img4))
        out.update(_fields("transpose_then_quantize", r["transpose_then_quantize"], 2 * n + img4))
        out.update(_fields("mxfp8_t", r["mxfp8_t"], 2 * n + img8))
        if var is not None:
            out.update(_fields("variant_t", r["variant_t"], 2 * n + img4))
        out["speedup"] = round(r["transpose_then_quantize"][0] / r["t"][0], 3)
        out["mxfp4_t_over_mxfp8_t"] = round(r["t"][0] / r["mxfp8_t"][0], 3)
        print(json.dumps(out), flush=True)

        sides = {"dual": lambda: quantize_mxfp4_dual(x),
                 "two_calls": lambda: (quantize_mxfp4(x), quantize_mxfp4(x.t().contiguous())),
                 "mxfp8_dual": lambda: quantize_mxfp8_dual(x)}
        if var is not None:
            sides["variant_dual"] = lambda: var[1](x)
        r = ab(sides, args.warmup_s, args.iters, args.block)
        out = {"case": "quantize_dual", "R": R, "C": C, "block": args.block}
        out.update(_fields("dual", r["dual"], 2 * n + 2 * img4))
        out.update(_fields("two_calls", r["two_calls"], 2 * n + 2 * img4))
        out.update(_fields("mxfp8_dual", r["mxfp8_dual"], 2 * n + 2 * img8))
        if var is not None:
            out.update(_fields("variant_dual", r["variant_dual"], 2 * n + 2 * img4))
        out["speedup"] = round(r["two_calls"][0] / r["dual"][0], 3)
        out["mxfp4_dual_over_mxfp8_dual"] = round(r["dual"][0] / r["mxfp8_dual"][0], 3)
        print(json.dumps(out), flush=True)
        del x
        torch.cuda.empty_cache()


def layer(args, dev):
    for fin, fout in LAYER_SHAPES:
        torch.manual_seed(fin + fout)
        mods = {c: Linear(fin, fout, compute=c, device=dev, dtype=torch.bfloat16)
                for c in Linear.COMPUTE}
        for c in ("mxfp8", "mxfp4"):
            mods[c].load_state_dict(mods["bf16"].state_dict())
        x = torch.randn((TOKENS, fin), device=dev, dtype=torch.bfloat16, requires_grad=True)
        dy = torch.randn((TOKENS, fout), device=dev, dtype=torch.bfloat16)

        # the trainer's weight-gradient route: straight into a flat-buffer view
        for m in mods.values():
            m.weight.main_grad = torch.empty_like(m.weight)

        def step(m):
            m.weight._mxk_grad_fresh = True
            m(x).backward(dy)
            x.grad = None

        r = ab({c: (lambda m=m: step(m)) for c, m in mods.items()}, args.warmup_s, args.iters,
               args.block)
        fl = 6.0 * TOKENS * fin * fout
        out = {"case": "linear_fwd_bwd", "tokens": TOKENS, "in": fin, "out": fout, "block": args.block}
        for c in mods:
            out.update(_fields(c, r[c]))
            out[c + "_tflops"] = round(fl / r[c][0] / 1e9, 1)
        out["speedup_mxfp4_over_bf16"] = round(r["bf16"][0] / r["mxfp4"][0], 3)
        out["speedup_mxfp4_over_mxfp8"] = round(r["mxfp8"][0] / r["mxfp4"][0], 3)
        print(json.dumps(out), flush=True)
        del mods, x, dy
        torch.cuda.empty_cache()


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--what", default="quantiser,layer")
    p.add_argument("--iters", type=int, default=40)
    p.add_argument("--block", type=int, default=5)
    p.add_argument("--warmup-s", type=float, default=2.0)
    p.add_argument("--variant-lib", default=None, metavar="PATH")
    a = p.parse_args()
    what = a.what.split(",")
    if not set(what) <= {"quantiser", "layer"}:
        p.error(f"--what takes quantiser and/or layer, got {a.what}")
    if not torch.cuda.is_available():
        print("mxfp4_linear_ab.py needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    if "quantiser" in what:
        quantiser(a, dev)
    if "layer" in what:
        layer(a, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
