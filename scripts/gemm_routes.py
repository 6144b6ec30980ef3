#!/usr/bin/env python3
"""What every bf16 GEMM entry point computes, call by call, as hashes.

    python scripts/gemm_routes.py [--lib PATH/libmxkernels.so] > routes.txt
    python scripts/gemm_routes.py --summarize routes.txt    # one line per entry point, to keep

Walks a fixed list of calls - the entry points of gemm_bf16.hip and
gemm_bf16_layouts.hip x operand layouts x variants x knob settings (through
the setters) - on fixed inputs and prints, per call, the status, the `split`
flag and the SHA-256 of the output bytes.  Two builds of the kernel library
that route every call to the same kernels print the same text; a refactor of
the host side shows it by an identical printout against the library of its
parent commit (``--lib``; default: the in-tree build or MXK_KERNELS_LIB).
Run under ``rocprofv3 --kernel-trace`` it also gives the sequence of kernel
names.  The library is bound here, by the names this script calls only, so a
library from before an export was added still loads.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mxk8s.ops import _lib  # noqa: E402

USED = ["mxk_gemm_bf16_tn", "mxk_gemm_bf16_ex", "mxk_gemm_bf16_ex_variant", "mxk_gemm_bf16_ex_ws",
        "mxk_gemm_bf16_dgrad_swiglu", "mxk_gemm_bf16_w13_swiglu", "mxk_gemm_bf16_rope",
        "mxk_gemm_bf16_tn_variant", "mxk_gemm_bf16_split_workspace", "mxk_gemm_bf16_ex_variant_built",
        "mxk_gemm_set_reserved_cus", "mxk_gemm_available_cus", "mxk_gemm_set_exclusive",
        "mxk_gemm_w13_set_sched", "mxk_gemm_swiglu_set_epi", "mxk_gemm_x2_set_order"]
LAYOUTS = {"tn": (1, 1), "nn": (1, 0), "tt": (0, 1), "nt": (0, 0)}
SHAPES = [(512, 768, 320), (512, 768, 1024), (256, 256, 1024), (256, 256, 960), (1024, 768, 1216),
          (4352, 4096, 1024)]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--lib", default=_lib.KERNEL_LIB_PATH)
    ap.add_argument("--summarize", metavar="PRINTOUT",
                    help="no GPU: condense a saved printout to one line per entry point")
    args = ap.parse_args()
    if args.summarize:
        groups: dict[str, list[str]] = {}
        for line in open(args.summarize).read().splitlines():
            groups.setdefault(line.split(" ", 1)[0], []).append(line)
        for tag, rows in groups.items():
            print(f"{tag}: {len(rows)} calls, {sum(' status=0 ' in r for r in rows)} launched, "
                  f"{sum(' split=1 ' in r for r in rows)} split, sha256 of the lines "
                  f"{hashlib.sha256(chr(10).join(rows).encode()).hexdigest()}")
        return 0
    L = ctypes.CDLL(args.lib, mode=ctypes.RTLD_GLOBAL)
    for name in USED:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _lib._SIGNATURES[name]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    gen = torch.Generator(device=dev).manual_seed(2024)

    def rnd(*shape, scale=1.0):
        return ((torch.rand(*shape, device=dev, generator=gen) * 2 - 1) * scale).bfloat16()

    def show(name, status, split, *outs):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for o in outs:
            h.update(o.cpu().contiguous().view(torch.uint8).numpy().tobytes())
        print(f"{name} status={status} split={split} sha256={h.hexdigest()}", flush=True)

    exp = bool(L.mxk_gemm_bf16_ex_variant_built(4))
    hw = L.mxk_gemm_available_cus()
    ws = torch.empty(L.mxk_gemm_bf16_split_workspace(), dtype=torch.uint8, device=dev)
    print(f"experiments={int(exp)}")

    # ---- the layout entry points -------------------------------------------
    for M, N, K in SHAPES:
        ops = {lay: (rnd(*((M, K) if ak else (K, M))), rnd(*((N, K) if bk else (K, N))))
               for lay, (ak, bk) in LAYOUTS.items()}
        wide = torch.empty(M, N + 8, device=dev, dtype=torch.bfloat16)
        for lay, (ak, bk) in LAYOUTS.items():
            a, b = ops[lay]

            def call(tag, fn, c, *tail):
                c.fill_(float("nan"))
                split = ctypes.c_int(-1)
                extra = [t if t != "split" else ctypes.byref(split) for t in tail]
                st = fn(a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, a.stride(0), b.stride(0),
                        c.stride(0), ak, bk, *extra, stream)
                show(f"{tag} {lay} {M}x{N}x{K} ldc={c.stride(0)}+{c.data_ptr() % 16}", st, split.value, c)

            full = wide[:, :N]                     # ldc = N + 8, 16-B stores
            narrow = wide[:, 4:N + 4]              # C at 8 mod 16: the 8-B-store instances
            tight = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            call("ex", L.mxk_gemm_bf16_ex, tight)
            for reserved in (0, hw - 4):
                L.mxk_gemm_set_reserved_cus(reserved)
                for c in (tight, narrow):
                    call(f"ex_ws reserved={reserved}", L.mxk_gemm_bf16_ex_ws, c, ws.data_ptr(), ws.numel(),
                         "split")
                call(f"ex_ws null-ws reserved={reserved}", L.mxk_gemm_bf16_ex_ws, tight, None, 0, "split")
                call(f"ex_ws misaligned-ws reserved={reserved}", L.mxk_gemm_bf16_ex_ws, tight,
                     ws.data_ptr() + 8, ws.numel() - 8, "split")
                call(f"ex_ws small-ws reserved={reserved}", L.mxk_gemm_bf16_ex_ws, tight, ws.data_ptr(),
                     256 * 256 * 4, "split")
                call(f"ex_variant 4 reserved={reserved}", L.mxk_gemm_bf16_ex_variant, full, 4)
            L.mxk_gemm_set_reserved_cus(0)
            if M > 1024:
                continue                            # the large shape: the split and x2t routes only
            for order in (0, 1):
                L.mxk_gemm_x2_set_order(order)
                for variant in (0, 1, 2, 3, 4, 5):
                    for c in (full, narrow):
                        call(f"ex_variant {variant} order={order}", L.mxk_gemm_bf16_ex_variant, c, variant)
                L.mxk_gemm_set_reserved_cus(hw - 4)
                call(f"ex_ws order={order} reserved={hw - 4}", L.mxk_gemm_bf16_ex_ws, tight, ws.data_ptr(),
                     ws.numel(), "split")
                L.mxk_gemm_set_reserved_cus(0)
            L.mxk_gemm_x2_set_order(0)
            L.mxk_gemm_set_exclusive(1)
            call("ex exclusive", L.mxk_gemm_bf16_ex, tight)
            L.mxk_gemm_set_exclusive(0)
    # ---- the TN entry point -------------------------------------------------
    for M, N, K in [(512, 768, 256), (500, 700, 200), (512, 768, 200)]:
        a, b = rnd(M, K), rnd(N, K)
        wide = torch.empty(M, N + 8, device=dev, dtype=torch.bfloat16)
        for tag, c in (("wide", wide[:, :N]), ("narrow", wide[:, 4:N + 4])):
            c.fill_(float("nan"))
            st = L.mxk_gemm_bf16_tn(a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, K, K, c.stride(0),
                                    stream)
            show(f"tn {tag} {M}x{N}x{K}", st, -1, c)
            for v in (1, 9, 26, 52):
                c.fill_(float("nan"))
                st = L.mxk_gemm_bf16_tn_variant(a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, K, K,
                                                c.stride(0), v, stream)
                show(f"tn_variant {v} {tag} {M}x{N}x{K}", st, -1, c)
    # ---- fused RoPE epilogue ------------------------------------------------
    M, N, K, S = 512, 768, 256, 256
    a, b = rnd(M, K), rnd(N, K)
    rc, rs = torch.rand(S, 64, device=dev, generator=gen), torch.rand(S, 64, device=dev, generator=gen)
    for cols in (0, 256, 768, 64):
        c = torch.full((M, N), float("nan"), device=dev, dtype=torch.bfloat16)
        st = L.mxk_gemm_bf16_rope(a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, K, K, N, rc.data_ptr(),
                                  rs.data_ptr(), S, cols, stream)
        show(f"rope cols={cols}", st, -1, c)
    # ---- fused up-projection ------------------------------------------------
    M, F, K = 512, 384, 256
    x, w13 = rnd(M, K), rnd(2 * F, K)
    for sched in (0, 1, 2, 3):
        L.mxk_gemm_w13_set_sched(sched)
        for Fc in (F, F - 64):
            gu = torch.full((M, 2 * F), float("nan"), device=dev, dtype=torch.bfloat16)
            h = torch.full((M, F), float("nan"), device=dev, dtype=torch.bfloat16)
            st = L.mxk_gemm_bf16_w13_swiglu(x.data_ptr(), w13.data_ptr(), gu.data_ptr(), h.data_ptr(), M, Fc,
                                            K, K, K, 2 * F, F, stream)
            show(f"w13_swiglu sched={sched} F={Fc}", st, -1, gu, h)
    L.mxk_gemm_w13_set_sched(0)
    # ---- down-projection dgrad with the SwiGLU backward ----------------------
    for (T, F, K), reserves in (((512, 1024, 256), (0,)), ((512, 1024, 64), (0,)),
                                ((4096, 8192, 1024), (0, 64))):
        # gu has dgu's row stride 2F: the 8-mod-16 view is 4 elements into a flat buffer
        dy, w2, flat = rnd(T, K), rnd(K, F, scale=0.05), rnd(T * 2 * F + 8, scale=3.0)
        dgu = torch.empty(T, 2 * F, device=dev, dtype=torch.bfloat16)
        for reserved in reserves:
            L.mxk_gemm_set_reserved_cus(reserved)
            for order in (0, 1):
                L.mxk_gemm_x2_set_order(order)
                for mode in (4, 0, 3, 5, 6, 8, 7):
                    L.mxk_gemm_swiglu_set_epi(mode)
                    for tag, g in (("gu16", flat[:T * 2 * F]), ("gu8", flat[4:T * 2 * F + 4])):
                        if tag == "gu8" and T > 512:
                            continue
                        dgu.fill_(float("nan"))
                        st = L.mxk_gemm_bf16_dgrad_swiglu(dy.data_ptr(), w2.data_ptr(), g.data_ptr(),
                                                          dgu.data_ptr(), T, F, K, K, F, stream)
                        show(f"dgrad_swiglu {T}x{F}x{K} mode={mode} order={order} reserved={reserved} {tag}",
                             st, -1, dgu)
    L.mxk_gemm_swiglu_set_epi(4)
    L.mxk_gemm_x2_set_order(0)
    L.mxk_gemm_set_reserved_cus(0)
    return 0


if __name__ == "__main__":
    sys.exit(main())
