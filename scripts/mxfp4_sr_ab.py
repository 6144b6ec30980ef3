#!/usr/bin/env python3
"""A/B of stochastic against nearest rounding on the MXFP4 gradient path, in one
process (BASELINE.md protocol, as scripts/mxfp4_linear_ab.py): >= 2 s warm-up of
every side, then blocks of event-timed calls going round the sides, medians.
One JSON line per case; beside every median the lowest and highest block median
of that side.

  quantiser   quantize_mxfp4_dual(x) with nearest against stochastic rounding
              (and quantize_mxfp4_t beside them) at the three gradient shapes
              of a Llama-3-8B layer; ms and effective GB/s
  layer       forward + backward of Linear at 16384 tokens, compute="bf16",
              "mxfp8", "mxfp4" and "mxfp4" with grad_rounding="stochastic",
              every quantiser launch included.  "sr_below_mxfp8": the highest
              block median of the stochastic layer lies below the lowest of
              the MXFP8 layer.
  static      VALU instruction counts of the nearest and the stochastic
              transposing kernels (vector, dual), from a device-only compile
              (needs hipcc; no GPU)

    python scripts/mxfp4_sr_ab.py [--what quantiser,layer,static] [--iters 40] [--block 5]
"""
from __future__ import annotations

import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from mxfp4_linear_ab import LAYER_SHAPES, QUANT_SHAPES, TOKENS, _fields, ab  # noqa: E402
from mxk8s.ops import quantize_mxfp4_dual, quantize_mxfp4_t  # noqa: E402
from mxk8s.ops.linear import Linear  # noqa: E402
from mxk8s.ops.mxfp4 import sr_reseed  # noqa: E402

SEED = 0x9E3779B97F4A7C14


def quantiser(args, dev):
    for R, C in QUANT_SHAPES:
        g = torch.Generator(device=dev)
        g.manual_seed(R + C)
        x = (torch.rand((R, C), device=dev, generator=g) * 2 - 1).bfloat16()
        n = R * C
        img = n // 2 + n // 32
        sides = {"dual": lambda: quantize_mxfp4_dual(x),
                 "dual_sr": lambda: quantize_mxfp4_dual(x, "stochastic", SEED),
                 "t": lambda: quantize_mxfp4_t(x),
                 "t_sr": lambda: quantize_mxfp4_t(x, "stochastic", SEED)}
        r = ab(sides, args.warmup_s, args.iters, args.block)
        out = {"case": "quantize_sr", "R": R, "C": C, "block": args.block}
        for k in sides:
            out.update(_fields(k, r[k], 2 * n + (2 if k.startswith("dual") else 1) * img))
        out["dual_sr_over_dual"] = round(r["dual_sr"][0] / r["dual"][0], 3)
        out["t_sr_over_t"] = round(r["t_sr"][0] / r["t"][0], 3)
        print(json.dumps(out), flush=True)
        del x
        torch.cuda.empty_cache()


def layer(args, dev):
    sr_reseed(0)
    for fin, fout in LAYER_SHAPES:
        torch.manual_seed(fin + fout)
        kinds = {"bf16": {}, "mxfp8": {}, "mxfp4": {}, "mxfp4_sr": {"grad_rounding": "stochastic"}}
        mods = {k: Linear(fin, fout, compute=k.split("_")[0], device=dev, dtype=torch.bfloat16, **kw)
                for k, kw in kinds.items()}
        for k in mods:
            mods[k].load_state_dict(mods["bf16"].state_dict())
        x = torch.randn((TOKENS, fin), device=dev, dtype=torch.bfloat16, requires_grad=True)
        dy = torch.randn((TOKENS, fout), device=dev, dtype=torch.bfloat16)
        for m in mods.values():                               # the trainer's weight-gradient route
            m.weight.main_grad = torch.empty_like(m.weight)

        def step(m):
            m.weight._mxk_grad_fresh = True
            m(x).backward(dy)
            x.grad = None

        r = ab({k: (lambda m=m: step(m)) for k, m in mods.items()}, args.warmup_s, args.iters,
               args.block)
        out = {"case": "linear_fwd_bwd_sr", "tokens": TOKENS, "in": fin, "out": fout, "block": args.block}
        for k in mods:
            out.update(_fields(k, r[k]))
        out["mxfp4_sr_over_mxfp4"] = round(r["mxfp4_sr"][0] / r["mxfp4"][0], 3)
        out["speedup_mxfp4_sr_over_mxfp8"] = round(r["mxfp8"][0] / r["mxfp4_sr"][0], 3)
        out["sr_below_mxfp8"] = r["mxfp4_sr"][2] < r["mxfp8"][1]
        print(json.dumps(out), flush=True)
        del mods, x, dy
        torch.cuda.empty_cache()


_VALU = re.compile(r"^\s+v_(?!mfma)\w+", re.M)


def static_counts():
    """Instructions of the vector dual transposing kernels as compiled now."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    hipcc = hipcc if os.path.exists(hipcc) else shutil.which("hipcc")
    if not hipcc:
        print(json.dumps({"case": "static", "error": "no hipcc"}), flush=True)
        return
    out = {"case": "static", "kernel": "quantize_tr_kernel<Fmt, VEC, DUAL>"}
    for name, src, struct in (("nearest", "gemm_mxfp4.hip", "E2m1E"), ("stochastic", "quantize_mxfp4_sr.hip", "E2m1SrE")):
        with tempfile.TemporaryDirectory() as tmp:
            s = os.path.join(tmp, "k.s")
            subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17",
                            "-I" + os.path.join(REPO, "native", "kernels"), "--cuda-device-only", "-S",
                            os.path.join(REPO, "native", "kernels", src), "-o", s], check=True,
                           capture_output=True)
            with open(s) as fh:
                asm = fh.read()
        for tag, flags in (("dual", "Lb1ELb1E"), ("t", "Lb1ELb0E")):
            m = re.search(r"^(_ZN3mxk2mx18quantize_tr_kernelIN12_GLOBAL__N_1\d+%s%s\w*):\s" % (struct, flags),
                          asm, re.M)
            body = asm[m.end():asm.index(".Lfunc_end", m.end())]
            valu = _VALU.findall(body)
            out[f"{name}_{tag}"] = {
                "valu": len(valu),
                "v_mul_u32": sum(any(o in v for o in ("v_mul_hi_u32", "v_mul_lo_u32", "v_mad_u64_u32"))
                                 for v in valu),
                "v_cmp": sum(v.strip().startswith("v_cmp") for v in valu),
                "salu": len(re.findall(r"^\s+s_(?!waitcnt|nop|barrier|endpgm)\w+", body, re.M))}
    print(json.dumps(out), flush=True)


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--what", default="quantiser,layer,static")
    p.add_argument("--iters", type=int, default=40)
    p.add_argument("--block", type=int, default=5)
    p.add_argument("--warmup-s", type=float, default=2.0)
    a = p.parse_args()
    what = a.what.split(",")
    if not set(what) <= {"quantiser", "layer", "static"}:
        p.error(f"--what takes quantiser, layer and/or static, got {a.what}")
    if "static" in what:
        static_counts()
    if not set(what) & {"quantiser", "layer"}:
        return 0
    if not torch.cuda.is_available():
        print("mxfp4_sr_ab.py needs a GPU for the quantiser and layer cases", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    if "quantiser" in what:
        quantiser(a, dev)
    if "layer" in what:
        layer(a, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
