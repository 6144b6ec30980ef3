#!/usr/bin/env python3
"""A/B of the MXFP4 scaled-MFMA GEMM against the MXFP8 and bf16 GEMMs at the same
M = N = K, in one process (BASELINE.md protocol): >= 2 s warm-up of all three,
then blocks of launches alternating between them, median of >= 60 event-timed
launches each.  The yardstick is the MXFP8 kernel of the same run: an FP4
K-tile stages the same bytes and takes the same matrix-core time as an MXFP8
K-tile of half the elements, so at equal M, N, K the FP4 kernel should take no
longer.  The spread of the per-block medians says what difference the run can
resolve.  Prints one JSON line per size.

    python scripts/mxfp4_ab.py [--sizes 4096,8192,16384] [--iters 60] [--block 10]
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

from mxk8s.ops import (gemm_bf16_tn, gemm_mxfp4_tn, gemm_mxfp8_tn, quantize_mxfp4,  # noqa: E402
                       quantize_mxfp8)


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
    p.add_argument("--quantize-size", type=int, default=8192,
                   help="the size at which the quantise time of both operands is reported")
    a = p.parse_args()
    dev = torch.device("cuda", 0)
    for n in [int(x) for x in a.sizes.split(",")]:
        g = torch.Generator(device=dev)
        g.manual_seed(n)
        x = (torch.rand((n, n), device=dev, generator=g) * 2 - 1).bfloat16()
        y = (torch.rand((n, n), device=dev, generator=g) * 2 - 1).bfloat16()
        out = torch.empty((n, n), dtype=torch.bfloat16, device=dev)
        x8, xs8 = quantize_mxfp8(x)
        y8, ys8 = quantize_mxfp8(y)
        x4, xs4 = quantize_mxfp4(x)
        y4, ys4 = quantize_mxfp4(y)
        extra = {}
        if n == a.quantize_size:
            extra = {
                "quantize_mxfp4_ms_both_operands": round(statistics.median(
                    timed(lambda: (quantize_mxfp4(x), quantize_mxfp4(y)), 10)), 4),
                "quantize_mxfp8_ms_both_operands": round(statistics.median(
                    timed(lambda: (quantize_mxfp8(x), quantize_mxfp8(y)), 10)), 4)}
        kernels = {
            "mxfp4": lambda: gemm_mxfp4_tn(x4, xs4, y4, ys4, out),
            "mxfp8": lambda: gemm_mxfp8_tn(x8, xs8, y8, ys8, out),
            "bf16": lambda: gemm_bf16_tn(x, y, out),
        }
        t0 = time.time()
        while time.time() - t0 < a.warmup_s:
            for _ in range(5):
                for fn in kernels.values():
                    fn()
            torch.cuda.synchronize()
        times = {k: [] for k in kernels}
        blocks = {k: [] for k in kernels}
        while len(times["mxfp4"]) < a.iters:
            for k, fn in kernels.items():
                t = timed(fn, a.block)
                times[k] += t
                blocks[k].append(statistics.median(t))
        fl = 2.0 * n * n * n
        row = {"M": n, "N": n, "K": n, "launches_each": len(times["mxfp4"])}
        for k in kernels:
            med = statistics.median(times[k])
            row[f"{k}_ms"] = round(med, 4)
            row[f"{k}_tflops"] = round(fl / med / 1e9, 1)
            row[f"{k}_block_medians_ms"] = [round(min(blocks[k]), 4), round(max(blocks[k]), 4)]
        row["ratio_mxfp4_over_mxfp8_time"] = round(row["mxfp4_ms"] / row["mxfp8_ms"], 3)
        row.update(extra)
        print(json.dumps(row), flush=True)
        del x, y, out, x8, xs8, y8, ys8, x4, xs4, y4, ys4
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
