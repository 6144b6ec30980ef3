#!/usr/bin/env python3
"""A/B of the per-document causal mask kernels (DocMask: mxk_attn_fwd_doc /
mxk_attn_bwd_doc) in one process, forward and backward, at the Llama-3-8B
layer shape (B 8, S 2048, 32/8 heads) and at S 8192, B 2:

  (a) the causal kernels they were built from - attn_fwd(variant=4) and
      attn_bwd(variant=5), each measured twice, interleaved with the DOC
      kernels on a single document; the spread of the two causal
      measurements is the bar for "same speed";
  (b) seeded tables of mean document length 2048, 512 and 128, with the
      table's visible_fraction and the share of the causal loops' 64-key
      tiles (per 32-row wave; dK/dV: 64-row slices per 16-key wave) that the
      DOC loops still visit;
  (c) the default backward (variant 9) for scale.

Timing as scripts/attn_mxk_bench.py: the chip warmed for >= WARM_S before the
first entry and >= 0.3 s per entry, then the median over 7 blocks of
back-to-back launches bracketed by one event pair.  One RESULT json line per
entry; SHAPES="B,S;B,S" overrides the shapes."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mxk8s.ops import attention as A  # noqa: E402
from mxk8s.ops.attention import DocMask  # noqa: E402
from mxk8s.train.ddp_llama import synthetic_doc_masks  # noqa: E402
from attn_mxk_bench import bench  # noqa: E402

HQ, HKV, D = 32, 8, 128


def visited_shares(doc: DocMask):
    """(forward / dQ, dK/dV): tiles resp. slices the DOC loops compute over
    those of the causal loops, by the kernels' own per-wave tests."""
    ds, de = doc.doc_start.cpu().long(), doc.doc_end.cpu().long()
    S = ds.shape[1]
    qw0 = torch.arange(0, S, 32)
    causal_q = qw0 // 64 + 1                                 # tiles 0 .. qw0 / 64
    doc_q = qw0 // 64 - ds[:, qw0] // 64 + 1                 # from the tile of doc_start[qw0]
    kw0 = torch.arange(0, S, 16)
    k0 = kw0 // 128 * 128
    t_lo = (kw0 - k0) // 64
    causal_k = (S - k0) // 64 - t_lo
    doc_k = (de[:, kw0 + 15] - k0 + 63) // 64 - t_lo         # up to the slice of doc_end[kw0 + 15]
    B = ds.shape[0]
    return (doc_q.sum().item() / (B * causal_q.sum().item()),
            doc_k.sum().item() / (B * causal_k.sum().item()))


def run_shape(B, S, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn(B, S, HQ, D, device=dev, generator=g).bfloat16()
    k = torch.randn(B, S, HKV, D, device=dev, generator=g).bfloat16()
    v = torch.randn(B, S, HKV, D, device=dev, generator=g).bfloat16()
    do = torch.randn(B, S, HQ, D, device=dev, generator=g).bfloat16()
    tables = {"single": DocMask.from_lengths([[S]] * B, S, device=dev)}
    for mean in (2048, 512, 128):
        tables[f"mean{mean}"] = synthetic_doc_masks(1, B, S, mean, 2000)[0].to(dev)

    def emit(**kw):
        print("RESULT " + json.dumps({"B": B, "S": S, **kw}), flush=True)

    # forward
    fwd = {}
    fwd["causal_v4_a"] = bench(lambda: A.attn_fwd(q, k, v, variant=4))
    fwd["single"] = bench(lambda: A.attn_fwd(q, k, v, doc=tables["single"]))
    fwd["causal_v4_b"] = bench(lambda: A.attn_fwd(q, k, v, variant=4))
    for name in ("mean2048", "mean512", "mean128"):
        fwd[name] = bench(lambda: A.attn_fwd(q, k, v, doc=tables[name]))
    # backward (each on the o / lse of its own forward)
    o, lse = A.attn_fwd(q, k, v, variant=4)
    bwd = {}
    bwd["causal_v5_a"] = bench(lambda: A.attn_bwd(q, k, v, o, lse, do, variant=5))
    bwd["single"] = bench(lambda: A.attn_bwd(q, k, v, o, lse, do, doc=tables["single"]))
    bwd["causal_v5_b"] = bench(lambda: A.attn_bwd(q, k, v, o, lse, do, variant=5))
    bwd["causal_v9_default"] = bench(lambda: A.attn_bwd(q, k, v, o, lse, do, variant=9))
    for name in ("mean2048", "mean512", "mean128"):
        od, ld = A.attn_fwd(q, k, v, doc=tables[name])
        bwd[name] = bench(lambda: A.attn_bwd(q, k, v, od, ld, do, doc=tables[name]))
    for kind, res, base in (("fwd", fwd, "causal_v4"), ("bwd", bwd, "causal_v5")):
        a, b = res[base + "_a"], res[base + "_b"]
        ref = (a + b) / 2
        emit(kind=kind, entry=base, ms_a=round(a, 4), ms_b=round(b, 4),
             spread_pct=round(abs(a - b) / ref * 100, 2))
        if kind == "bwd":
            emit(kind=kind, entry="causal_v9_default", ms=round(res["causal_v9_default"], 4),
                 vs_causal_v5=round(res["causal_v9_default"] / ref, 4))
        for name, doc in tables.items():
            sq, sk = visited_shares(doc)
            emit(kind=kind, entry="doc_" + name, ms=round(res[name], 4),
                 vs_causal=round(res[name] / ref, 4),
                 visible_fraction=round(doc.visible_fraction(), 4),
                 visited_tiles_fwd_dq=round(sq, 4), visited_slices_dkdv=round(sk, 4))


def main():
    dev = torch.device("cuda")
    shapes = os.environ.get("SHAPES", "8,2048;2,8192")
    for item in shapes.split(";"):
        B, S = (int(x) for x in item.split(","))
        run_shape(B, S, dev)


if __name__ == "__main__":
    main()
