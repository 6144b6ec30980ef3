"""What the MXFP8 and MXFP4 tests share (``test_gpu_mxfp8.py``,
``test_gpu_mxfp4.py`` and the two ``*_cpu.py`` files): one description per
format and the check bodies written once against it.  The shapes and
parametrisations stay in the test files; they differ per format on purpose
(K-tile 128 against 256).  A plain helper module, not collected.
"""
import functools
import os
import re
import shutil
import stat
import subprocess
import tempfile
from dataclasses import dataclass
from typing import Callable

import torch

import mxk8s.validate.__main__ as V
from mxk8s import ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("MXK8S_BIN", os.path.join(REPO, "bin"))
_HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HIPCC = _HIPCC if os.path.exists(_HIPCC) else shutil.which("hipcc")    # None: no compiler


def _one_hot_scales(rows, K):
    """127 + ((row + 3 block) mod 9) - 4: every (row, block) has its own scale."""
    r, blk = torch.arange(rows), torch.arange(K // 32)
    return (127 + ((r[:, None] + 3 * blk[None, :]) % 9) - 4).to(torch.uint8)


def _one_hot_mxfp8(rows, K, mult, off, code_mul, code_off, neg_every):
    """[rows, K] e4m3 bytes with one non-zero per row at k = (mult row + off)
    mod K, a distinct finite code per row."""
    q = torch.zeros((rows, K), dtype=torch.uint8)
    r = torch.arange(rows)
    code = 1 + (r * code_mul + code_off) % 126              # 0x01 .. 0x7e: finite, non-zero
    code = code | torch.where(r % neg_every == 0, 0x80, 0)
    q[r, (mult * r + off) % K] = code.to(torch.uint8)
    return q.view(torch.float8_e4m3fn), _one_hot_scales(rows, K)


def _one_hot_mxfp4(rows, K, mult, off, code_mul, code_off, neg_every):
    """Packed [rows, K/2] with one non-zero per row at k = (mult row + off) mod
    K, the code cycling through 1..7, the sign bit on every neg_every-th row."""
    r = torch.arange(rows)
    code = 1 + (r * code_mul + code_off) % 7
    code = code | torch.where(r % neg_every == 0, 8, 0)
    k = (mult * r + off) % K
    q = torch.zeros((rows, K // 2), dtype=torch.uint8)
    q[r, k // 2] = (code << (4 * (k % 2))).to(torch.uint8)
    return q, _one_hot_scales(rows, K)


@dataclass(frozen=True)
class Format:
    name: str
    struct: str              # the element format's struct in the quantiser kernels' symbols
    quantize: Callable
    quantize_ref: Callable
    dequantize: Callable
    gemm: Callable
    q_dtype: torch.dtype
    per_byte: int            # elements in a byte of q
    k_tile: int              # the GEMM's K granularity
    one_hot: Callable
    q_pad: int               # byte that fills padding of q (a NaN or the largest code; 0xFF for s)
    not_fast_k: int          # a K that *_is_fast refuses

    def row_bytes(self, K):
        return K // self.per_byte

    @property
    def quantize_entry(self):
        return "mxk_quantize_" + self.name

    @property
    def gemm_entry(self):
        return "mxk_gemm_%s_tn" % self.name


MXFP8 = Format("mxfp8", "E4m3", ops.quantize_mxfp8, ops.quantize_mxfp8_ref, ops.dequantize_mxfp8,
               ops.gemm_mxfp8_tn, torch.float8_e4m3fn, 1, 128, _one_hot_mxfp8, 0x7f, 64)
MXFP4 = Format("mxfp4", "E2m1", ops.quantize_mxfp4, ops.quantize_mxfp4_ref, ops.dequantize_mxfp4,
               ops.gemm_mxfp4_tn, torch.uint8, 2, 256, _one_hot_mxfp4, 0xFF, 128)


# ---- build hygiene ---------------------------------------------------------------
_META = ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


@functools.lru_cache(maxsize=None)
def kernel_listing(f):
    """native/kernels/gemm_<name>.hip compiled for gfx950, device only: the
    assembly and, per kernel symbol, its scratch size and spill counts."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "m.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17",
                        "-I" + os.path.join(REPO, "native", "kernels"), "--cuda-device-only", "-S",
                        os.path.join(REPO, "native", "kernels", "gemm_%s.hip" % f.name), "-o", out],
                       check=True, capture_output=True)
        with open(out) as fh:
            asm = fh.read()
    by = {}
    kernels = asm[asm.index("amdhsa.kernels:"):]
    for entry in kernels[:kernels.index("\namdhsa.")].split("\n  - ")[1:]:
        name = re.search(r"\n    \.name:\s+(\S+)", entry).group(1)    # at the entry's own depth
        by[name] = {k: int(re.search(r"\n    \.%s:\s+(\d+)" % k, entry).group(1)) for k in _META}
    return asm, by


def check_quantiser_kernels(f, by, kernel, count):
    """Exactly `count` instantiations of the shared quantiser `kernel` on this
    format's struct and none on another; each without scratch or spills: all
    3 x count metadata fields are there and zero.  Returns their symbols."""
    named = [n for n in by if kernel in n]
    mine = [n for n in named if f.struct in n]
    assert len(mine) == count and named == mine, sorted(by)
    fields = [(n, k, by[n][k]) for n in mine for k in _META]
    assert len(fields) == 3 * count and all(v == 0 for _, _, v in fields), fields
    return mine


# ---- GPU checks -----------------------------------------------------------------
def _rand(shape, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.rand(shape, device=dev, generator=g) * 2 - 1


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.uint8 if t.element_size() == 1 else torch.int16).cpu()


def _ref64(f, aq, a_s, bq, b_s):
    return f.dequantize(aq, a_s).double() @ f.dequantize(bq, b_s).double().t()


def _check(c, ref):
    """The project's bf16-output criterion: max |C - ref| <= 2^-7 max |ref|
    (bf16 rounding of the output is 2^-9 relative to the element, so at most
    0.38 of the budget; the accumulation-order difference ~1e-5 of it)."""
    assert not torch.isnan(c.float()).any()
    err = (c.double() - ref).abs().max().item()
    mx = ref.abs().max().item()
    assert mx > 0 and err <= 2 ** -7 * mx, (err, mx)


def _quantized_pair(f, dev, M, N, K, seed):
    return (*f.quantize(_rand((M, K), dev, seed).bfloat16()),
            *f.quantize(_rand((N, K), dev, seed + 1).bfloat16()))


def one_hot_lane_map(f, dev, K, pa, pb):
    M = N = 256
    aq, a_s = f.one_hot(M, K, pa[0], pa[1], 5, 0, 3)
    bq, b_s = f.one_hot(N, K, pb[0], pb[1], 11, 17, 2)
    ref = f.gemm(aq, a_s, bq, b_s)                          # CPU path: exact here
    assert torch.equal(ref.double(), _ref64(f, aq, a_s, bq, b_s))
    assert torch.count_nonzero(ref) >= 200                  # the pattern does meet
    c = f.gemm(aq.to(dev), a_s.to(dev), bq.to(dev), b_s.to(dev))
    # + 0.0 folds the sign of a zero sum, which the reference does not define
    assert torch.equal(_bits(c + 0.0), _bits(ref + 0.0))


def random_vs_dequantised(f, dev, M, N, K, seed=31):
    ops_ = _quantized_pair(f, dev, M, N, K, seed)
    _check(f.gemm(*ops_), _ref64(f, *ops_))


def padded_strides_and_untouched_padding(f, dev, M, N, K):
    """lda, ldb, ldc and both scale strides exceed the widths; then a K slice
    of q from byte 128 on with the matching column slice of s."""
    aq0, as0, bq0, bs0 = _quantized_pair(f, dev, M, N, K, 35)

    def widen(t, extra, fill):
        buf = torch.full((t.shape[0], t.shape[1] + extra), fill, dtype=torch.uint8, device=t.device)
        buf[:, :t.shape[1]] = t.view(torch.uint8)
        return buf.view(t.dtype)[:, :t.shape[1]]

    aq, bq = widen(aq0, 32, f.q_pad), widen(bq0, 48, f.q_pad)
    a_s, b_s = widen(as0, 4, 0xff), widen(bs0, 8, 0xff)
    assert aq.stride(0) > f.row_bytes(K) and a_s.stride(0) > K // 32
    cbuf = torch.full((M, N + 8), -7.0, dtype=torch.bfloat16, device=dev)
    out = f.gemm(aq, a_s, bq, b_s, out=cbuf[:, :N])
    _check(out, _ref64(f, aq0, as0, bq0, bs0))
    assert torch.all(cbuf[:, N:] == -7.0)
    qs, ss = slice(128, f.row_bytes(K)), slice(128 * f.per_byte // 32, K // 32)
    sl = f.gemm(aq0[:, qs], as0[:, ss], bq0[:, qs], bs0[:, ss])
    _check(sl, _ref64(f, aq0[:, qs].contiguous(), as0[:, ss].contiguous(),
                      bq0[:, qs].contiguous(), bs0[:, ss].contiguous()))


def block_scales_spread(f, dev):
    """bf16 data multiplied per block by 2^-6 .. 2^6: the scales differ from
    block to block and row to row."""
    M, N, K = 256, 512, 512

    def spread(rows, seed):
        x = _rand((rows, K), dev, seed)
        g = torch.Generator(device=dev)
        g.manual_seed(seed + 100)
        e = torch.randint(-6, 7, (rows, K // 32), device=dev, generator=g)
        return (x.reshape(rows, K // 32, 32) * torch.exp2(e.float()).unsqueeze(2)).reshape(rows, K).bfloat16()

    aq, a_s = f.quantize(spread(M, 37))
    bq, b_s = f.quantize(spread(N, 38))
    assert a_s.unique().numel() >= 10
    _check(f.gemm(aq, a_s, bq, b_s), _ref64(f, aq, a_s, bq, b_s))


def _quant_inputs(R, K, kind, dev):
    x = _rand((R, K), dev, 41 + R + K)
    if kind == "uniform":
        return x.bfloat16()
    if kind == "wide":
        g = torch.Generator(device=dev)
        g.manual_seed(R * 7 + K)
        e = torch.randint(-130, 125, (R, K), device=dev, generator=g)
        return torch.ldexp(x, e).bfloat16()                 # bf16 subnormals to ~2^124
    if kind == "zero_blocks":
        x = x.reshape(R, K // 32, 32).clone()
        x[:, ::2] = 0
        x[0, -1, 5] = -0.0
        return x.reshape(R, K).bfloat16()
    assert kind == "strided"
    buf = torch.zeros((R, K + 24), device=dev, dtype=torch.bfloat16)
    buf[:, 8:K + 8] = x.bfloat16()
    return buf[:, 8:K + 8]                                  # row stride K + 24


def _quantize_into_poisoned(f, x):
    """The raw entry point on 0xA5-filled buffers wider and longer than the
    result: returns (q, s) and asserts that no byte outside them changed.  The
    24 bytes of row padding are a multiple of both formats' packed store, so
    an aligned x still takes the vector kernel."""
    from mxk8s.ops import _lib
    R, K = x.shape
    qw, sw = f.row_bytes(K), K // 32
    qbuf = torch.full((R + 1, qw + 24), 0xA5, dtype=torch.uint8, device=x.device)
    sbuf = torch.full((R + 1, sw + 5), 0xA5, dtype=torch.uint8, device=x.device)
    st = getattr(_lib.lib(), f.quantize_entry)(x.data_ptr(), qbuf.data_ptr(), sbuf.data_ptr(), R, K,
                                               x.stride(0), qbuf.stride(0), sbuf.stride(0),
                                               _lib.stream_ptr(x.device))
    assert st == 0
    torch.cuda.synchronize()
    assert torch.all(qbuf[:, qw:] == 0xA5) and torch.all(qbuf[R:] == 0xA5)
    assert torch.all(sbuf[:, sw:] == 0xA5) and torch.all(sbuf[R:] == 0xA5)
    return qbuf[:R, :qw], sbuf[:R, :sw]


def quantiser_bit_equal_to_reference(f, x):
    R, K = x.shape
    qr, sr = f.quantize_ref(x.cpu())
    q, s = f.quantize(x)
    assert q.dtype == f.q_dtype and s.dtype == torch.uint8
    assert tuple(q.shape) == (R, f.row_bytes(K)) and tuple(s.shape) == (R, K // 32)
    assert torch.equal(_bits(s), _bits(sr))
    assert torch.equal(_bits(q), _bits(qr))
    qp, sp = _quantize_into_poisoned(f, x)
    assert torch.equal(_bits(sp), _bits(sr)) and torch.equal(_bits(qp), _bits(qr))


def unaligned_rows(dev):
    """A view whose rows are not 16-byte aligned: the element-wise path."""
    R, K = 5, 64
    buf = torch.zeros((R, K + 3), device=dev, dtype=torch.bfloat16)
    buf[:, 1:K + 1] = _rand((R, K), dev, 43).bfloat16()
    return buf[:, 1:K + 1]


def poisoned_output_and_run_to_run_identity(f, dev, M, N, K):
    ops_ = _quantized_pair(f, dev, M, N, K, 51)
    outs = []
    for _ in range(2):
        out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
        f.gemm(*ops_, out=out)
        outs.append(_bits(out))
    assert torch.equal(outs[0], outs[1])                    # no atomics: bit-identical
    _check(outs[0].view(torch.bfloat16).to(dev), _ref64(f, *ops_))


def contract_violation_launches_nothing(f, dev):
    """M = 128 at the smallest K the kernel takes: refused, C untouched."""
    from mxk8s.ops import _lib
    L = _lib.lib()
    is_fast = getattr(L, f.gemm_entry + "_is_fast")
    K, qw, sw = f.k_tile, f.row_bytes(f.k_tile), f.k_tile // 32
    assert is_fast(256, 256, K) == 1
    assert is_fast(256, 256, f.not_fast_k) == 0
    out = torch.full((128, 256), 3.0, dtype=torch.bfloat16, device=dev)
    q = torch.zeros((256, qw), dtype=torch.uint8, device=dev)
    s = torch.full((256, sw), 127, dtype=torch.uint8, device=dev)
    st = getattr(L, f.gemm_entry)(q.data_ptr(), s.data_ptr(), q.data_ptr(), s.data_ptr(), out.data_ptr(),
                                  128, 256, K, qw, sw, qw, sw, 256, _lib.stream_ptr(dev))
    assert st == 1                                          # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert torch.all(out == 3.0)


def _bench(f, env=None):
    return subprocess.run(["timeout", "-k", "10", "120", os.path.join(BIN, "mx-gemm-bench"),
                           "--dtype", f.name, "--sizes", "256,512", "--iters", "3",
                           "--warmup-ms", "50", "--devices", "0"],
                          capture_output=True, text=True, env=env)


def gemm_bench_self_checks(f):
    p = _bench(f)
    rs = V.results_from(p.stdout)
    assert p.returncode == 0 and len(rs) == 2, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    for r, n in zip(rs, (256, 512)):
        assert r["test"] == "gemm" and r["dtype"] == f.name and r["pass"] is True, r
        assert r["M"] == r["N"] == r["K"] == n and r["rel_err_vs_rocblas"] is None, r
        assert 0 <= r["max_abs_err"] <= r["spot_tolerance"] and r["tflops"] > 0, r
        assert r["quantize_ms"] > 0, r


def gemm_bench_fails_when_kernel_skipped(f):
    p = _bench(f, dict(os.environ, MXK_GEMM_BENCH_SKIP_KERNEL="1"))
    assert p.returncode not in (0, 124, 137), (p.returncode, p.stdout[-2000:])
    r = V.results_from(p.stdout)[-1]
    assert r["pass"] is False and "error" in r, r


# ---- validator plumbing on the CPU: a scripted mx-gemm-bench ----------------------
BF16_LINE = ('{"test":"gemm","gpu":0,"M":4096,"N":4096,"K":4096,"dtype":"bf16","median_ms":0.1,'
             '"min_ms":0.1,"tflops":1300.0,"rel_err_vs_rocblas":0.001,"spot_block":[0,0],'
             '"max_abs_err":0.1,"spot_tolerance":0.5,"pass":true}')
MX_TFLOPS = {"mxfp8": 2500.0, "mxfp4": 4000.0}


def mx_line(dtype, ok=True):
    return ('{"test":"gemm","gpu":0,"M":4096,"N":4096,"K":4096,"dtype":"%s","median_ms":0.05,'
            '"min_ms":0.05,"tflops":%s,"rel_err_vs_rocblas":null,"spot_block":[0,0],'
            '"max_abs_err":0.1,"spot_tolerance":0.5,"quantize_ms":0.1,"pass":%s}'
            % (dtype, MX_TFLOPS[dtype], "true" if ok else "false"))


def fake_bench(tmp_path, dtype=None, ok=True, rc=0):
    """An mx-gemm-bench that logs its arguments to tmp_path/calls and prints one
    recorded line for the --dtype it was given; ``dtype``'s line has "pass": ok
    and its run exits with rc."""
    cases = "".join(f"  *{d}*) echo 'RESULT {mx_line(d, ok or d != dtype)}'; exit {rc if d == dtype else 0};;\n"
                    for d in ("mxfp4", "mxfp8"))
    p = tmp_path / "mx-gemm-bench"
    p.write_text("#!/bin/sh\n"
                 f'echo "$@" >> {tmp_path}/calls\n'
                 'case "$*" in\n' + cases +
                 f"  *) echo 'RESULT {BF16_LINE}';;\n"
                 "esac\n")
    p.chmod(p.stat().st_mode | stat.S_IEXEC)


def run_validator(tmp_path, monkeypatch, capsys, argv):
    monkeypatch.setattr(V, "BIN", str(tmp_path))
    monkeypatch.setattr(V, "_extra_env", {})
    rc = V.main(argv)
    rs = V.results_from(capsys.readouterr().out)
    calls = (tmp_path / "calls").read_text().splitlines()
    return rc, rs, calls
