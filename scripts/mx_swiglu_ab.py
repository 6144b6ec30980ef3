#!/usr/bin/env python3
"""A/B of SwiGLU fused into the MX quantisers against today's composition, in one
process (BASELINE.md protocol, as scripts/mxfp4_sr_ab.py): >= 2 s warm-up of
both sides, then blocks of event-timed calls going round the sides, medians.
One JSON line per case; beside every median the lowest and highest block median
of that side.  "fused_below": the highest block median of the fused form lies
below the lowest block median of the composition, the project's criterion.

  entry   each fused entry point against its composition at gu [16384, 2 * 14336]
          (Llama-3-8B's MLP at 16384 tokens), MXFP8 and MXFP4, and the stochastic
          MXFP4 dual:
            rows  swiglu_quantize_<fmt>(gu)           | quantize_<fmt>(swiglu_fwd(gu))
            t     swiglu_quantize_<fmt>_t(gu)         | quantize_<fmt>_t(swiglu_fwd(gu))
            dual  swiglu_bwd_quantize_<fmt>_dual(gu, dh) | quantize_<fmt>_dual(swiglu_bwd(gu, dh))
          "bytes": what each side moves as counted from the code (bf16 reads and
          writes plus the images), and the effective GB/s of that count
  mlp     forward + backward of the MLP 4096 -> 14336 -> 4096 at 16384 tokens with
          main_grad weight gradients: swiglu_mlp_mx against Linear -> SwiGLULinear,
          for mxfp8, mxfp4 and mxfp4 with stochastic gradient rounding; peak
          memory of one step of each side

    python scripts/mx_swiglu_ab.py [--what entry,mlp] [--iters 60] [--block 10]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from mxfp4_linear_ab import TOKENS, _fields, ab  # noqa: E402
from mxk8s.ops import mxfp4, mxfp8  # noqa: E402
from mxk8s.ops.fused import swiglu_bwd, swiglu_fwd  # noqa: E402
from mxk8s.ops.linear import Linear, SwiGLULinear, swiglu_mlp_mx  # noqa: E402

DIM, FFN = 4096, 14336
SEED = 0x9E3779B97F4A7C14


def _rand(shape, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return (torch.rand(shape, device=dev, generator=g) * 2 - 1).bfloat16()


def entry(args, dev):
    T, F = TOKENS, FFN
    gu, dh = _rand((T, 2 * F), dev, 1), _rand((T, F), dev, 2)
    n = T * F
    for name, m, bits in (("mxfp8", mxfp8, 8), ("mxfp4", mxfp4, 4)):
        op = lambda pattern: getattr(m, pattern.format(name))   # noqa: E731
        img = n * bits // 8 + n // 32                           # one image of a [T, F] tensor
        cases = [
            # (case, fused, composition, bytes fused, bytes composition)
            ("rows", lambda: op("swiglu_quantize_{}")(gu), lambda: op("quantize_{}")(swiglu_fwd(gu)),
             4 * n + img, 4 * n + 2 * n + 2 * n + img),
            ("t", lambda: op("swiglu_quantize_{}_t")(gu), lambda: op("quantize_{}_t")(swiglu_fwd(gu)),
             4 * n + img, 4 * n + 2 * n + 2 * n + img),
            ("dual", lambda: op("swiglu_bwd_quantize_{}_dual")(gu, dh),
             lambda: op("quantize_{}_dual")(swiglu_bwd(gu, dh)),
             6 * n + 4 * img, 6 * n + 4 * n + 4 * n + 4 * img),
        ]
        if name == "mxfp4":
            cases.append(("dual_sr", lambda: m.swiglu_bwd_quantize_mxfp4_dual(gu, dh, "stochastic", SEED),
                          lambda: m.quantize_mxfp4_dual(swiglu_bwd(gu, dh), "stochastic", SEED),
                          6 * n + 4 * img, 6 * n + 4 * n + 4 * n + 4 * img))
        for case, fused, comp, b_fused, b_comp in cases:
            r = ab({"fused": fused, "composition": comp}, args.warmup_s, args.iters, args.block)
            out = {"case": "entry_" + case, "fmt": name, "T": T, "F": F, "block": args.block,
                   "iters": args.iters}
            out.update(_fields("fused", r["fused"], b_fused))
            out.update(_fields("composition", r["composition"], b_comp))
            out["bytes"] = {"fused": b_fused, "composition": b_comp}
            out["fused_over_composition"] = round(r["fused"][0] / r["composition"][0], 3)
            out["fused_below"] = r["fused"][2] < r["composition"][1]
            print(json.dumps(out), flush=True)
            torch.cuda.empty_cache()


def mlp(args, dev):
    T = TOKENS
    for key, fmt, rounding in (("mxfp8", "mxfp8", "nearest"), ("mxfp4", "mxfp4", "nearest"),
                               ("mxfp4_sr", "mxfp4", "stochastic")):
        torch.manual_seed(DIM + FFN)
        kw = dict(compute=fmt, grad_rounding=rounding, device=dev, dtype=torch.bfloat16)
        w13, w2 = Linear(DIM, 2 * FFN, **kw), SwiGLULinear(FFN, DIM, **kw)
        x = torch.randn((T, DIM), device=dev, dtype=torch.bfloat16, requires_grad=True)
        dy = torch.randn((T, DIM), device=dev, dtype=torch.bfloat16)
        for layer in (w13, w2):                               # the trainer's weight-gradient route
            layer.weight.main_grad = torch.empty_like(layer.weight)
        mxfp4.sr_reseed(0)

        def step(fused):
            w13.weight._mxk_grad_fresh = w2.weight._mxk_grad_fresh = True
            if fused:
                y = swiglu_mlp_mx(x, w13.weight, w2.weight, fmt, rounding)
            else:
                y = w2(w13(x))
            y.backward(dy)
            x.grad = None

        peak = {}
        for side, fused in (("fused", True), ("composition", False)):
            step(fused)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            base = torch.cuda.memory_allocated(dev)
            step(fused)
            torch.cuda.synchronize()
            peak[side] = round((torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20, 1)
        r = ab({"fused": lambda: step(True), "composition": lambda: step(False)}, args.warmup_s,
               args.iters, args.block)
        out = {"case": "mlp_fwd_bwd", "config": key, "tokens": T, "dim": DIM, "ffn": FFN,
               "block": args.block, "iters": args.iters}
        out.update(_fields("fused", r["fused"]))
        out.update(_fields("composition", r["composition"]))
        out["fused_over_composition"] = round(r["fused"][0] / r["composition"][0], 3)
        out["fused_below"] = r["fused"][2] < r["composition"][1]
        out["step_peak_mib_above_resident"] = peak
        print(json.dumps(out), flush=True)
        del w13, w2, x, dy
        torch.cuda.empty_cache()


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--what", default="entry,mlp")
    p.add_argument("--iters", type=int, default=60)
    p.add_argument("--block", type=int, default=10)
    p.add_argument("--warmup-s", type=float, default=2.0)
    a = p.parse_args()
    what = a.what.split(",")
    if not set(what) <= {"entry", "mlp"}:
        p.error(f"--what takes entry and/or mlp, got {a.what}")
    if not torch.cuda.is_available():
        print("mx_swiglu_ab.py needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    if "entry" in what:
        entry(a, dev)
    if "mlp" in what:
        mlp(a, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
