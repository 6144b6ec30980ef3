#!/usr/bin/env python3
"""A/B of the pieces of the MXFP8 linear path, in one process (BASELINE.md
protocol): >= 2 s warm-up of both sides, then blocks of event-timed calls
alternating between the two, medians.  One JSON line per case.

  quantiser   quantize_mxfp8_t(x) against quantize_mxfp8(x.t().contiguous()),
              quantize_mxfp8_dual(x) against quantize_mxfp8(x) +
              quantize_mxfp8(x.t().contiguous()); ms and effective GB/s (the
              bytes one pass needs: 2 B read per element, 1 B + 1/32 B
              written per image)
  layer       forward + backward of Linear at 16384 tokens, compute="bf16"
              against compute="mxfp8" with every quantiser launch included

    python scripts/mxfp8_linear_ab.py [--what quantiser,layer] [--iters 40] [--block 5]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mxk8s.ops import quantize_mxfp8, quantize_mxfp8_dual, quantize_mxfp8_t  # noqa: E402
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


def ab(a, b, warmup_s, iters, block):
    """Medians (ms) of a and b: warm-up of both, then alternating blocks."""
    t0 = time.time()
    while time.time() - t0 < warmup_s:
        a()
        b()
        torch.cuda.synchronize()
    ta, tb = [], []
    while len(ta) < iters:
        ta += timed(a, block)
        tb += timed(b, block)
    return statistics.median(ta), statistics.median(tb), len(ta)


def quantiser(args, dev):
    for R, C in QUANT_SHAPES:
        g = torch.Generator(device=dev)
        g.manual_seed(R + C)
        x = (torch.rand((R, C), device=dev, generator=g) * 2 - 1).bfloat16()
        n = R * C
        img = n + n // 32
        new, old, k = ab(lambda: quantize_mxfp8_t(x), lambda: quantize_mxfp8(x.t().contiguous()),
                         args.warmup_s, args.iters, args.block)
        print(json.dumps({"case": "quantize_t", "R": R, "C": C, "launches_each": k,
                          "t_ms": round(new, 4), "t_gbps": round((2 * n + img) / new / 1e6, 1),
                          "transpose_then_quantize_ms": round(old, 4),
                          "transpose_then_quantize_gbps": round((2 * n + img) / old / 1e6, 1),
                          "speedup": round(old / new, 3)}), flush=True)
        new, old, k = ab(lambda: quantize_mxfp8_dual(x),
                         lambda: (quantize_mxfp8(x), quantize_mxfp8(x.t().contiguous())),
                         args.warmup_s, args.iters, args.block)
        print(json.dumps({"case": "quantize_dual", "R": R, "C": C, "launches_each": k,
                          "dual_ms": round(new, 4), "dual_gbps": round((2 * n + 2 * img) / new / 1e6, 1),
                          "two_calls_ms": round(old, 4),
                          "two_calls_gbps": round((2 * n + 2 * img) / old / 1e6, 1),
                          "speedup": round(old / new, 3)}), flush=True)
        del x
        torch.cuda.empty_cache()


def layer(args, dev):
    for fin, fout in LAYER_SHAPES:
        torch.manual_seed(fin + fout)
        mods = {c: Linear(fin, fout, compute=c, device=dev, dtype=torch.bfloat16)
                for c in ("bf16", "mxfp8")}
        mods["mxfp8"].load_state_dict(mods["bf16"].state_dict())
        x = torch.randn((TOKENS, fin), device=dev, dtype=torch.bfloat16, requires_grad=True)
        dy = torch.randn((TOKENS, fout), device=dev, dtype=torch.bfloat16)

        # the trainer's weight-gradient route: straight into a flat-buffer view
        for m in mods.values():
            m.weight.main_grad = torch.empty_like(m.weight)

        def step(m):
            m.weight._mxk_grad_fresh = True
            m(x).backward(dy)
            x.grad = None

        bf, mx, k = ab(lambda: step(mods["bf16"]), lambda: step(mods["mxfp8"]), args.warmup_s,
                       args.iters, args.block)
        fl = 6.0 * TOKENS * fin * fout
        print(json.dumps({"case": "linear_fwd_bwd", "tokens": TOKENS, "in": fin, "out": fout,
                          "launches_each": k, "bf16_ms": round(bf, 4),
                          "bf16_tflops": round(fl / bf / 1e9, 1), "mxfp8_ms": round(mx, 4),
                          "mxfp8_tflops": round(fl / mx / 1e9, 1),
                          "speedup_mxfp8_over_bf16": round(bf / mx, 3)}), flush=True)
        del mods, x, dy
        torch.cuda.empty_cache()


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--what", default="quantiser,layer")
    p.add_argument("--iters", type=int, default=40)
    p.add_argument("--block", type=int, default=5)
    p.add_argument("--warmup-s", type=float, default=2.0)
    a = p.parse_args()
    what = a.what.split(",")
    if not set(what) <= {"quantiser", "layer"}:
        p.error(f"--what takes quantiser and/or layer, got {a.what}")
    if not torch.cuda.is_available():
        print("mxfp8_linear_ab.py needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    if "quantiser" in what:
        quantiser(a, dev)
    if "layer" in what:
        layer(a, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
