#!/usr/bin/env python3
"""A/B of the MXFP8 scaled-MFMA GEMM against the bf16 GEMM at the same M = N = K,
in one process (BASELINE.md protocol): >= 2 s warm-up of both, then blocks of
launches alternating between the two, median of >= 50 event-timed launches
each.  Prints one JSON line per size.

    python scripts/mxfp8_ab.py [--sizes 4096,8192,16384] [--iters 60] [--block 10]
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

from mxk8s.ops import gemm_bf16_tn, gemm_mxfp8_tn, quantize_mxfp8  # noqa: E402


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


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--sizes", default="4096,8192,16384")
    p.add_argument("--iters", type=int, default=60)
    p.add_argument("--block", type=int, default=10)
    p.add_argument("--warmup-s", type=float, default=2.0)
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    for n in [int(x) for x in a.sizes.split(",")]:
        g = torch.Generator(device=dev)
        g.manual_seed(n)
        x = (torch.rand((n, n), device=dev, generator=g) * 2 - 1).bfloat16()
        y = (torch.rand((n, n), device=dev, generator=g) * 2 - 1).bfloat16()
        out = torch.empty((n, n), dtype=torch.bfloat16, device=dev)
        xq, xs = quantize_mxfp8(x)
        yq, ys = quantize_mxfp8(y)
        q_ms = statistics.median(timed(lambda: (quantize_mxfp8(x), quantize_mxfp8(y)), 10))

        def bf16():
            gemm_bf16_tn(x, y, out)

        def mx():
            gemm_mxfp8_tn(xq, xs, yq, ys, out)

        t0 = time.time()
        while time.time() - t0 < a.warmup_s:
            for _ in range(5):
                bf16()
                mx()
            torch.cuda.synchronize()
        tb, tm = [], []
        while len(tb) < a.iters:
            tb += timed(bf16, a.block)
            tm += timed(mx, a.block)
        mb, mm = statistics.median(tb), statistics.median(tm)
        fl = 2.0 * n * n * n
        print(json.dumps({"M": n, "N": n, "K": n, "launches_each": len(tb),
                          "bf16_ms": round(mb, 4), "bf16_tflops": round(fl / mb / 1e9, 1),
                          "mxfp8_ms": round(mm, 4), "mxfp8_tflops": round(fl / mm / 1e9, 1),
                          "ratio_mxfp8_over_bf16": round(mb / mm, 3),
                          "quantize_ms_both_operands": round(q_ms, 4)}), flush=True)
        del x, y, out, xq, xs, yq, ys
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
