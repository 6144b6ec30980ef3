"""MXFP4 quantiser and scaled-MFMA GEMM on the GPU (``native/kernels/gemm_mxfp4.hip``).

Every check compares against the product of the DEQUANTISED operands: against
the unquantised bf16 product the format's own error is about 21 %.
"""
import json
import os
import subprocess

import pytest
import torch

from mxk8s.ops import (dequantize_mxfp4, gemm_mxfp4_tn, quantize_mxfp4, quantize_mxfp4_ref)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.environ.get("MXK8S_BIN", os.path.join(REPO, "bin"))


def _rand(shape, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.rand(shape, device=dev, generator=g) * 2 - 1


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.uint8 if t.element_size() == 1 else torch.int16).cpu()


def _ref64(aq, a_s, bq, b_s):
    return dequantize_mxfp4(aq, a_s).double() @ dequantize_mxfp4(bq, b_s).double().t()


def _check(c, ref):
    """The project's bf16-output criterion: max |C - ref| <= 2^-7 max |ref|
    (bf16 rounding of the output is 2^-9 relative to the element, so at most
    0.38 of the budget; the accumulation-order difference ~1e-5 of it)."""
    assert not torch.isnan(c.float()).any()
    err = (c.double() - ref).abs().max().item()
    mx = ref.abs().max().item()
    assert mx > 0 and err <= 2 ** -7 * mx, (err, mx)


# ---- 1. one-hot lane map ---------------------------------------------------
def _one_hot(rows, K, mult, off, code_mul, code_off, neg_every):
    """Packed [rows, K/2] with one non-zero per row at k = (mult row + off) mod
    K, the code cycling through 1..7, the sign bit on every neg_every-th row;
    scales 127 + ((row + 3 block) mod 9) - 4, so every (row, block) has its own."""
    r = torch.arange(rows)
    code = 1 + (r * code_mul + code_off) % 7
    code = code | torch.where(r % neg_every == 0, 8, 0)
    k = (mult * r + off) % K
    q = torch.zeros((rows, K // 2), dtype=torch.uint8)
    q[r, k // 2] = (code << (4 * (k % 2))).to(torch.uint8)
    blk = torch.arange(K // 32)
    s = (127 + ((r[:, None] + 3 * blk[None, :]) % 9) - 4).to(torch.uint8)
    return q, s


@pytest.mark.parametrize("K,pa,pb", [(256, (37, 5), (53, 11)), (256, (91, 3), (29, 7)),
                                     (256, (113, 64), (77, 130)),
                                     (512, (74, 5), (106, 11)), (512, (74, 4), (106, 10))])
def test_one_hot_lane_map(cuda_device, K, pa, pb):
    """Every product here is a single term and exactly representable in bf16
    (tests/test_mxfp4_cpu.py asserts that over all code pairs), so the kernel
    must reproduce the CPU dequantised product bit for bit.  A permuted k or
    nibble order, a scale taken from the wrong block, lane or register byte,
    swapped operand roles or a transposed store all change some element.
    K = 256 is one K-tile (every k-step, nibble and scale byte of the kernel
    and nothing else); K = 512 brings in the second stage buffer.  There an
    odd multiplier is invertible mod 512 and 256 rows would meet only 128
    times, so the multipliers are doubled: each operand's 256 rows then hit
    every odd (or, with even offsets, every even) k of both K-tiles once and
    the patterns meet 256 times."""
    M = N = 256
    aq, a_s = _one_hot(M, K, pa[0], pa[1], 5, 0, 3)
    bq, b_s = _one_hot(N, K, pb[0], pb[1], 11, 17, 2)
    ref = gemm_mxfp4_tn(aq, a_s, bq, b_s)                   # CPU path: exact here
    exact = _ref64(aq, a_s, bq, b_s)
    assert torch.equal(ref.double(), exact)
    assert torch.count_nonzero(ref) >= 200                  # the pattern does meet
    c = gemm_mxfp4_tn(aq.to(cuda_device), a_s.to(cuda_device), bq.to(cuda_device),
                      b_s.to(cuda_device))
    # + 0.0 folds the sign of a zero sum, which the reference does not define
    assert torch.equal(_bits(c + 0.0), _bits(ref + 0.0))


# ---- 2. random operands against the dequantised reference -------------------
@pytest.mark.parametrize("M,N,K", [(256, 256, 256),      # one K-tile, no DMA in the loop
                                   (256, 256, 512),      # the no-DMA tail only
                                   (512, 768, 768),      # the DMA loop runs once, 2-D tile map
                                   (768, 256, 1280),     # five K-tiles: both buffers refilled
                                   (1024, 4096, 256)])   # 64 tiles: more than one XCD round
def test_random_vs_dequantised_fp64(cuda_device, M, N, K):
    aq, a_s = quantize_mxfp4(_rand((M, K), cuda_device, 31).bfloat16())
    bq, b_s = quantize_mxfp4(_rand((N, K), cuda_device, 32).bfloat16())
    _check(gemm_mxfp4_tn(aq, a_s, bq, b_s), _ref64(aq, a_s, bq, b_s))


# ---- 3. block scales spread ---------------------------------------------------
def test_block_scales_spread(cuda_device):
    """bf16 data multiplied per block by 2^-6 .. 2^6: the scales differ from
    block to block and row to row."""
    M, N, K = 256, 512, 512

    def spread(rows, seed):
        x = _rand((rows, K), cuda_device, seed)
        g = torch.Generator(device=cuda_device)
        g.manual_seed(seed + 100)
        e = torch.randint(-6, 7, (rows, K // 32), device=cuda_device, generator=g)
        return (x.reshape(rows, K // 32, 32) * torch.exp2(e.float()).unsqueeze(2)).reshape(rows, K).bfloat16()

    aq, a_s = quantize_mxfp4(spread(M, 37))
    bq, b_s = quantize_mxfp4(spread(N, 38))
    assert a_s.unique().numel() >= 10
    _check(gemm_mxfp4_tn(aq, a_s, bq, b_s), _ref64(aq, a_s, bq, b_s))


# ---- 4. padded strides ----------------------------------------------------------
def test_padded_strides_and_untouched_padding(cuda_device):
    """Views into wider buffers whose padding holds 0xFF bytes (two -6 codes,
    the E8M0 NaN): lda, ldb, ldc and both scale strides exceed the widths."""
    M, N, K = 512, 256, 768
    aq0, as0 = quantize_mxfp4(_rand((M, K), cuda_device, 35).bfloat16())
    bq0, bs0 = quantize_mxfp4(_rand((N, K), cuda_device, 36).bfloat16())

    def widen(t, extra):
        buf = torch.full((t.shape[0], t.shape[1] + extra), 0xFF, dtype=torch.uint8, device=t.device)
        buf[:, :t.shape[1]] = t
        return buf[:, :t.shape[1]]

    aq, bq = widen(aq0, 32), widen(bq0, 48)
    a_s, b_s = widen(as0, 4), widen(bs0, 8)
    assert aq.stride(0) > K // 2 and a_s.stride(0) > K // 32
    cbuf = torch.full((M, N + 8), -7.0, dtype=torch.bfloat16, device=cuda_device)
    out = gemm_mxfp4_tn(aq, a_s, bq, b_s, out=cbuf[:, :N])
    _check(out, _ref64(aq0, as0, bq0, bs0))
    assert torch.all(cbuf[:, N:] == -7.0)
    # a K slice of q (k = 256 .. 767: bytes 128 .. 383) with the matching column slice of s
    sl = gemm_mxfp4_tn(aq0[:, 128:384], as0[:, 8:24], bq0[:, 128:384], bs0[:, 8:24])
    _check(sl, _ref64(aq0[:, 128:384].contiguous(), as0[:, 8:24].contiguous(),
                      bq0[:, 128:384].contiguous(), bs0[:, 8:24].contiguous()))


# ---- 5. quantiser ------------------------------------------------------------
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


def _quantize_into_poisoned(x):
    """The raw entry point on 0xA5-filled buffers wider and longer than the
    result: returns (q, s) and asserts that no byte outside them changed."""
    from mxk8s.ops import _lib
    R, K = x.shape
    qbuf = torch.full((R + 1, K // 2 + 12), 0xA5, dtype=torch.uint8, device=x.device)
    sbuf = torch.full((R + 1, K // 32 + 5), 0xA5, dtype=torch.uint8, device=x.device)
    st = _lib.lib().mxk_quantize_mxfp4(x.data_ptr(), qbuf.data_ptr(), sbuf.data_ptr(), R, K,
                                       x.stride(0), qbuf.stride(0), sbuf.stride(0),
                                       _lib.stream_ptr(x.device))
    assert st == 0
    torch.cuda.synchronize()
    assert torch.all(qbuf[:, K // 2:] == 0xA5) and torch.all(qbuf[R:] == 0xA5)
    assert torch.all(sbuf[:, K // 32:] == 0xA5) and torch.all(sbuf[R:] == 0xA5)
    return qbuf[:R, :K // 2], sbuf[:R, :K // 32]


@pytest.mark.parametrize("kind", ["uniform", "wide", "zero_blocks", "strided"])
@pytest.mark.parametrize("K", [32, 96, 1152])
@pytest.mark.parametrize("R", [1, 3, 256])
def test_quantiser_bit_equal_to_reference(cuda_device, R, K, kind):
    x = _quant_inputs(R, K, kind, cuda_device)
    qr, sr = quantize_mxfp4_ref(x.cpu())
    q, s = quantize_mxfp4(x)
    assert q.dtype == torch.uint8 and s.dtype == torch.uint8
    assert tuple(q.shape) == (R, K // 2) and tuple(s.shape) == (R, K // 32)
    assert torch.equal(_bits(s), _bits(sr))
    assert torch.equal(_bits(q), _bits(qr))
    qp, sp = _quantize_into_poisoned(x)
    assert torch.equal(_bits(sp), _bits(sr)) and torch.equal(_bits(qp), _bits(qr))


def test_quantiser_unaligned_rows(cuda_device):
    """A view whose rows are not 16-byte aligned takes the element-wise path."""
    R, K = 5, 64
    buf = torch.zeros((R, K + 3), device=cuda_device, dtype=torch.bfloat16)
    buf[:, 1:K + 1] = _rand((R, K), cuda_device, 43).bfloat16()
    x = buf[:, 1:K + 1]
    qr, sr = quantize_mxfp4_ref(x.cpu())
    q, s = quantize_mxfp4(x)
    assert torch.equal(_bits(s), _bits(sr)) and torch.equal(_bits(q), _bits(qr))
    qp, sp = _quantize_into_poisoned(x)
    assert torch.equal(_bits(sp), _bits(sr)) and torch.equal(_bits(qp), _bits(qr))


# ---- 6. poisoned output, run-to-run identity ----------------------------------
def test_poisoned_output_and_run_to_run_identity(cuda_device):
    M, N, K = 512, 512, 1280
    aq, a_s = quantize_mxfp4(_rand((M, K), cuda_device, 51).bfloat16())
    bq, b_s = quantize_mxfp4(_rand((N, K), cuda_device, 52).bfloat16())
    outs = []
    for _ in range(2):
        out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=cuda_device)
        gemm_mxfp4_tn(aq, a_s, bq, b_s, out=out)
        outs.append(_bits(out))
    assert torch.equal(outs[0], outs[1])                    # no atomics: bit-identical
    _check(outs[0].view(torch.bfloat16).to(cuda_device), _ref64(aq, a_s, bq, b_s))


# ---- 7. contract violation ------------------------------------------------------
def test_contract_violation_launches_nothing(cuda_device):
    from mxk8s.ops import _lib
    L = _lib.lib()
    assert L.mxk_gemm_mxfp4_tn_is_fast(256, 256, 256) == 1
    assert L.mxk_gemm_mxfp4_tn_is_fast(256, 256, 128) == 0
    out = torch.full((128, 256), 3.0, dtype=torch.bfloat16, device=cuda_device)
    q = torch.zeros((256, 128), dtype=torch.uint8, device=cuda_device)
    s = torch.full((256, 8), 127, dtype=torch.uint8, device=cuda_device)
    st = L.mxk_gemm_mxfp4_tn(q.data_ptr(), s.data_ptr(), q.data_ptr(), s.data_ptr(), out.data_ptr(),
                             128, 256, 256, 128, 8, 128, 8, 256, _lib.stream_ptr(cuda_device))
    assert st == 1                                          # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert torch.all(out == 3.0)


# ---- 8. mx-gemm-bench --dtype mxfp4 -------------------------------------------
def _bench(env=None):
    return subprocess.run(["timeout", "-k", "10", "120", os.path.join(BIN, "mx-gemm-bench"),
                           "--dtype", "mxfp4", "--sizes", "256,512", "--iters", "3",
                           "--warmup-ms", "50", "--devices", "0"],
                          capture_output=True, text=True, env=env)


def _results(stdout):
    return [json.loads(ln[7:]) for ln in stdout.splitlines() if ln.startswith("RESULT ")]


def test_gemm_bench_mxfp4_self_checks():
    p = _bench()
    rs = _results(p.stdout)
    assert p.returncode == 0 and len(rs) == 2, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    for r, n in zip(rs, (256, 512)):
        assert r["test"] == "gemm" and r["dtype"] == "mxfp4" and r["pass"] is True, r
        assert r["M"] == r["N"] == r["K"] == n and r["rel_err_vs_rocblas"] is None, r
        assert 0 <= r["max_abs_err"] <= r["spot_tolerance"] and r["tflops"] > 0, r
        assert r["quantize_ms"] > 0, r


def test_gemm_bench_mxfp4_fails_when_kernel_skipped():
    p = _bench(dict(os.environ, MXK_GEMM_BENCH_SKIP_KERNEL="1"))
    assert p.returncode not in (0, 124, 137), (p.returncode, p.stdout[-2000:])
    r = _results(p.stdout)[-1]
    assert r["pass"] is False and "error" in r, r
