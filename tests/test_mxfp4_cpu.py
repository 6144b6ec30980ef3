"""MXFP4 (block-scaled e2m1) path, everything that needs no GPU: the reference
quantiser, the op's contract, validator plumbing, build hygiene of
``native/kernels/gemm_mxfp4.hip`` and the host sweep of ``mxfp4_format.h``."""
import os
import re
import subprocess

import pytest
import torch

import mx_gemm_checks as mx
import mxk8s.validate.__main__ as V
from mx_gemm_checks import fake_bench, run_validator
from mxk8s.ops import _lib
from mxk8s.ops.mxfp4 import (dequantize_mxfp4, gemm_mxfp4_tn, is_fast_shape_mxfp4, quantize_mxfp4,
                             quantize_mxfp4_ref)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAGNITUDES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _wide(rows, K, seed, lo=-40, hi=40):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, K), generator=g)
    e = torch.randint(lo, hi, (rows, K), generator=g)
    return torch.ldexp(x, e).bfloat16()


def _codes(q):
    """[R, K/2] packed bytes -> [R, K] codes, element 2i from the low nibble."""
    return torch.stack((q & 0xF, q >> 4), dim=2).reshape(q.shape[0], -1)


def _brute(v: float) -> int:
    """Nearest of the eight magnitudes to min(|v|, 6), ties to the even code;
    what rounds to zero is code 0."""
    a = min(abs(v), 6.0)
    best = 0
    for c in range(1, 8):
        d, db = abs(a - MAGNITUDES[c]), abs(a - MAGNITUDES[best])
        if d < db or (d == db and c % 2 == 0):
            best = c
    return (best | 8) if (best and v < 0) else best


# ---- reference quantiser ------------------------------------------------------
def test_rounding_is_nearest_with_ties_to_the_even_code():
    """A bf16 grid of step 1/32 over [-6.5, 6.5] holds every midpoint (0.25,
    0.75, 1.25, 1.75, 2.5, 3.5, 5); each value sits in a block whose maximum
    is 6, so e = 0 and the element is converted unscaled."""
    vals = torch.arange(-208, 209, dtype=torch.float32) / 32
    assert torch.equal(vals.bfloat16().float(), vals)
    for m in (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0):
        assert (vals == m).any() and (vals == -m).any()
    x = torch.zeros((vals.numel(), 32))
    x[:, 0] = 6.0
    x[:, 1] = vals
    q, s = quantize_mxfp4_ref(x.bfloat16())
    assert torch.all(s == 127)
    got = _codes(q)[:, 1].tolist()
    want = [_brute(v) for v in vals.tolist()]
    assert got == want
    # the ties, spelled out: the even neighbour wins
    tie = dict(zip(vals.tolist(), got))
    assert [tie[m] for m in (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)] == [0, 2, 2, 4, 4, 6, 6]
    assert tie[-0.25] == 0 and tie[-0.75] == 10 and tie[-5.0] == 14 and tie[-6.5] == 15


def test_even_k_lands_in_the_low_nibble_and_odd_k_in_the_high_one():
    x = torch.zeros((2, 32))
    x[0, 0], x[0, 1] = 6.0, 1.0                              # codes 7 and 2
    x[1, 30], x[1, 31] = -3.0, 6.0                           # codes 13 and 7
    q, _ = quantize_mxfp4_ref(x.bfloat16())
    assert q.dtype == torch.uint8 and tuple(q.shape) == (2, 16)
    assert q[0, 0].item() == 0x27 and q[1, 15].item() == 0x7D
    assert q[0, 1:].abs().sum().item() == 0 and q[1, :15].abs().sum().item() == 0
    if hasattr(torch, "float4_e2m1fn_x2"):
        assert q.view(torch.float4_e2m1fn_x2).shape == q.shape   # the packing torch names


def test_block_maxima_land_in_4_8_before_clamping():
    x = _wide(64, 1152, 1)
    _, s = quantize_mxfp4_ref(x)
    e = s.to(torch.int32) - 127
    amax = x.float().reshape(64, -1, 32).abs().amax(dim=2)
    scaled = torch.ldexp(amax, -e)
    assert torch.all((scaled >= 4) & (scaled < 8))


def test_zero_block_gives_byte_127_and_zero_codes():
    x = (torch.rand(4, 96) + 0.5).bfloat16()
    x[1, 32:64] = 0
    x[2, 64:96] = -0.0
    q, s = quantize_mxfp4_ref(x)
    assert s[1, 1].item() == 127 and s[2, 2].item() == 127
    assert torch.all(q[1, 16:32] == 0) and torch.all(q[2, 32:48] == 0)
    assert not (s == 255).any()


@pytest.mark.parametrize("e", [-100, -9, 0, 7, 100])
def test_6_survives_and_7_saturates(e):
    x = torch.zeros(2, 32)
    x[0, 3], x[0, 4] = 6.0, -6.0
    x[1, 3], x[1, 4] = 7.0, -7.0
    x = torch.ldexp(x, torch.tensor(e)).bfloat16()
    q, s = quantize_mxfp4_ref(x)
    assert s[0, 0].item() == e + 127 and s[1, 0].item() == e + 127
    d = dequantize_mxfp4(q, s)
    want = torch.ldexp(torch.tensor(6.0), torch.tensor(e))
    assert d[0, 3] == want and d[0, 4] == -want
    assert d[1, 3] == want and d[1, 4] == -want


def test_scale_exponent_clamps_and_subnormal_input():
    x = torch.zeros(2, 32, dtype=torch.bfloat16)
    x[0, 0] = 2.0 ** -133                                   # smallest bf16 subnormal
    x[1, 0] = 2.0 ** 127
    q, s = quantize_mxfp4_ref(x)
    assert s[0, 0].item() == 0 and s[1, 0].item() == 127 + 125
    # 2^-133 2^127 = 2^-6 rounds to 0; 2^127 2^-125 = 4
    assert _codes(q)[0, 0].item() == 0 and _codes(q)[1, 0].item() == 6
    x[0, 0] = 2.0 ** -128                                   # 2^-128 2^127 = 0.5
    q, s = quantize_mxfp4_ref(x)
    assert s[0, 0].item() == 0 and _codes(q)[0, 0].item() == 1


def test_round_trip_of_a_tensor_on_the_mx_grid_is_the_identity():
    """A tensor on the MX grid is a dequantised quantiser output: its block
    maxima are 4 x 2^e or 6 x 2^e, so the same exponent is chosen again and
    every element is kept."""
    for x0 in (_wide(32, 256, 3), (torch.rand(32, 256) * 2 - 1).bfloat16()):
        q0, s0 = quantize_mxfp4_ref(x0)
        x = dequantize_mxfp4(q0, s0)
        assert torch.equal(x.bfloat16().float(), x)         # the MX grid is inside bf16
        q, s = quantize_mxfp4_ref(x.bfloat16())
        assert torch.equal(s, s0) and torch.equal(q, q0)
        assert torch.equal(dequantize_mxfp4(q, s), x)


def test_cpu_quantize_is_the_reference():
    x = _wide(8, 64, 4)
    q, s = quantize_mxfp4(x)
    qr, sr = quantize_mxfp4_ref(x)
    assert q.dtype == torch.uint8 and torch.equal(q, qr) and torch.equal(s, sr)


def test_product_of_any_two_e2m1_values_is_exact_in_bf16():
    """2 + 2 significand bits fit bf16's 8 and the exponents are tiny: the
    one-hot GPU test's bit-equality rests on this (the block scales only move
    the exponent)."""
    q = torch.arange(256, dtype=torch.int32).to(torch.uint8).reshape(16, 16)
    v = dequantize_mxfp4(q, torch.full((16, 1), 127, dtype=torch.uint8)).reshape(-1)
    assert sorted(set(v.abs().tolist())) == list(MAGNITUDES)
    p = v[:, None].double() * v[None, :].double()
    assert torch.equal(p.float().bfloat16().double(), p)


# ---- shape and dtype contract (nothing here may load the library) ---------------
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the kernel library was loaded")
    monkeypatch.setattr(_lib, "lib", boom)


def _pair(rows, K, dev="cpu"):
    q = torch.zeros((rows, K // 2), dtype=torch.uint8, device=dev)
    s = torch.full((rows, K // 32), 127, dtype=torch.uint8, device=dev)
    return q, s


@pytest.mark.parametrize("dev", ["cpu", "meta"])
def test_gemm_contract_raises_before_the_library(no_library, dev):
    a, a_s = _pair(256, 256, dev)
    b, b_s = _pair(256, 256, dev)
    with pytest.raises(ValueError, match="M % 256"):
        gemm_mxfp4_tn(*_pair(128, 256, dev), b, b_s)            # M = 128
    with pytest.raises(ValueError, match="K % 256"):
        gemm_mxfp4_tn(*_pair(256, 128, dev), *_pair(256, 128, dev))   # K = 128
    with pytest.raises(ValueError, match="K mismatch"):
        gemm_mxfp4_tn(a, a_s, *_pair(256, 512, dev))
    with pytest.raises(ValueError, match="multiple of 32"):
        gemm_mxfp4_tn(torch.zeros((256, 24), dtype=torch.uint8, device=dev), a_s, b, b_s)   # K = 48
    with pytest.raises(TypeError):
        gemm_mxfp4_tn(a.view(torch.int8), a_s, b, b_s)          # wrong element dtype
    with pytest.raises(TypeError):
        gemm_mxfp4_tn(a, a_s.to(torch.int8), b, b_s)            # wrong scale dtype
    with pytest.raises(TypeError):
        gemm_mxfp4_tn(a, a_s, b, b_s, out=torch.empty((256, 256), dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="2-D"):
        gemm_mxfp4_tn(a.reshape(-1), a_s, b, b_s)
    wide, _ = _pair(256, 512, dev)
    with pytest.raises(ValueError, match="K-contiguous"):
        gemm_mxfp4_tn(wide[:, ::2], a_s, b, b_s)                # non-unit inner stride
    with pytest.raises(ValueError, match=r"a_s must be \[256, 8\]"):
        gemm_mxfp4_tn(a, torch.full((256, 7), 127, dtype=torch.uint8, device=dev), b, b_s)
    with pytest.raises(ValueError, match=r"b_s must be \[256, 8\]"):
        gemm_mxfp4_tn(a, a_s, b, torch.full((128, 8), 127, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="out must be"):
        gemm_mxfp4_tn(a, a_s, b, b_s, out=torch.empty((256, 128), dtype=torch.bfloat16, device=dev))
    with pytest.raises(ValueError, match="row-major"):
        gemm_mxfp4_tn(a, a_s, b, b_s,
                      out=torch.empty((256, 512), dtype=torch.bfloat16, device=dev)[:, ::2])


@pytest.mark.parametrize("dev", ["cpu", "meta"])
def test_quantize_contract_raises_before_the_library(no_library, dev):
    with pytest.raises(TypeError):
        quantize_mxfp4(torch.zeros((4, 32), device=dev))                       # fp32
    with pytest.raises(ValueError):
        quantize_mxfp4(torch.zeros((4, 48), dtype=torch.bfloat16, device=dev))  # K % 32
    with pytest.raises(ValueError):
        quantize_mxfp4(torch.zeros((4, 64), dtype=torch.bfloat16, device=dev)[:, ::2])
    with pytest.raises(ValueError):
        quantize_mxfp4(torch.zeros((32,), dtype=torch.bfloat16, device=dev))


def test_gpu_layout_limits_raise_before_the_library(no_library):
    """Element rows 16-byte, scale rows 4-byte aligned, out rows 16-byte
    (checked for device tensors only; 'meta' stands in for one here)."""
    a, a_s = _pair(256, 256, "meta")
    odd = torch.zeros((256, 136), dtype=torch.uint8, device="meta")[:, :128]
    with pytest.raises(ValueError, match="16 bytes"):
        gemm_mxfp4_tn(odd, a_s, a, a_s)
    s_odd = torch.zeros((256, 10), dtype=torch.uint8, device="meta")[:, :8]
    with pytest.raises(ValueError, match="4 bytes"):
        gemm_mxfp4_tn(a, s_odd, a, a_s)
    out = torch.empty((256, 260), dtype=torch.bfloat16, device="meta")[:, :256]
    with pytest.raises(ValueError, match="out: base"):
        gemm_mxfp4_tn(a, a_s, a, a_s, out=out)


def test_is_fast_shape():
    assert is_fast_shape_mxfp4(256, 512, 256) and is_fast_shape_mxfp4(8192, 8192, 8192)
    assert not is_fast_shape_mxfp4(256, 256, 128) and not is_fast_shape_mxfp4(128, 256, 256)
    assert not is_fast_shape_mxfp4(0, 256, 256)


def test_cpu_path_is_the_dequantised_fp32_product_rounded_to_bf16():
    g = torch.Generator().manual_seed(5)
    aq, a_s = quantize_mxfp4((torch.rand((256, 768), generator=g) * 2 - 1).bfloat16())
    bq, b_s = quantize_mxfp4(_wide(512, 768, 6, -6, 6))
    want = (dequantize_mxfp4(aq, a_s) @ dequantize_mxfp4(bq, b_s).t()).bfloat16()
    got = gemm_mxfp4_tn(aq, a_s, bq, b_s)
    assert got.dtype == torch.bfloat16 and torch.equal(got, want)
    # views: a K slice of q (K = 256.., bytes 128..) with the matching column slice of s, and out=
    out = torch.empty((256, 520), dtype=torch.bfloat16)[:, :512]
    r = gemm_mxfp4_tn(aq[:, 128:], a_s[:, 8:], bq[:, 128:], b_s[:, 8:], out=out)
    assert r is out
    want2 = (dequantize_mxfp4(aq[:, 128:], a_s[:, 8:]) @
             dequantize_mxfp4(bq[:, 128:], b_s[:, 8:]).t()).bfloat16()
    assert torch.equal(out, want2)


def test_fp4_error_against_the_bf16_product_is_the_formats_own():
    """~21 % in Frobenius norm for uniform [-1, 1) (scaled block maxima land in
    [4, 8) and everything above 5 becomes 6): why no check compares against the
    unquantised product."""
    g = torch.Generator().manual_seed(7)
    x = (torch.rand((256, 256), generator=g) * 2 - 1).bfloat16()
    y = (torch.rand((256, 256), generator=g) * 2 - 1).bfloat16()
    qx, sx = quantize_mxfp4(x)
    c = gemm_mxfp4_tn(qx, sx, *quantize_mxfp4(y)).float()
    ref = x.float() @ y.float().t()
    rel = ((c - ref).norm() / ref.norm()).item()
    sat = ((_codes(qx) & 7) == 7).float().mean().item()
    print(f"mxfp4 vs bf16 product: rel Frobenius error {rel:.4f}, {100 * sat:.1f} % of elements on |6|")
    assert 0.15 < rel < 0.30, rel


# ---- validator plumbing ---------------------------------------------------------
def test_validator_three_dtypes_three_runs_two_tagged_summaries(tmp_path, monkeypatch, capsys):
    fake_bench(tmp_path)
    rc, rs, calls = run_validator(tmp_path, monkeypatch, capsys,
                                  ["--tests", "gemm", "--gemm-dtypes", "bf16,mxfp8,mxfp4",
                                   "--gemm-sizes", "4096"])
    assert rc == 0
    assert calls == ["--sizes 4096 --devices all", "--sizes 4096 --devices all --dtype mxfp8",
                     "--sizes 4096 --devices all --dtype mxfp4"]
    summ = [r for r in rs if r["test"] == "gemm_summary"]
    assert len(summ) == 3 and "dtype" not in summ[0]
    assert [s["dtype"] for s in summ[1:]] == ["mxfp8", "mxfp4"]
    assert summ[2]["aggregate_tflops"] == {"4096": 4000.0} and summ[2]["pass"] is True
    lines = [r for r in rs if r["test"] == "gemm"]
    assert [r["dtype"] for r in lines] == ["bf16", "mxfp8", "mxfp4"] and "quantize_ms" in lines[2]
    assert rs[-1] == {**rs[-1], "test": "validator", "pass": True, "results": {"gemm": True}}


@pytest.mark.parametrize("fp4_rc", [0, 1])
def test_validator_fails_on_a_failing_mxfp4_line(tmp_path, monkeypatch, capsys, fp4_rc):
    fake_bench(tmp_path, "mxfp4", ok=False, rc=fp4_rc)
    rc, rs, _ = run_validator(tmp_path, monkeypatch, capsys,
                              ["--tests", "gemm", "--gemm-dtypes", "bf16,mxfp8,mxfp4"])
    assert rc == 1
    assert rs[-1]["test"] == "validator" and rs[-1]["pass"] is False
    summ = {r.get("dtype"): r for r in rs if r["test"] == "gemm_summary"}
    assert summ["mxfp4"]["pass"] is False and summ["mxfp8"]["pass"] is True


def test_validator_fails_on_a_nonzero_exit_with_a_passing_line(tmp_path, monkeypatch, capsys):
    fake_bench(tmp_path, "mxfp4", ok=True, rc=3)
    rc, rs, _ = run_validator(tmp_path, monkeypatch, capsys,
                              ["--tests", "gemm", "--gemm-dtypes", "mxfp4"])
    assert rc == 1 and rs[-1]["pass"] is False


def test_validator_mxfp4_alone(tmp_path, monkeypatch, capsys):
    fake_bench(tmp_path)
    rc, rs, calls = run_validator(tmp_path, monkeypatch, capsys,
                                  ["--tests", "gemm", "--gemm-dtypes", "mxfp4", "--gemm-sizes", "4096"])
    assert rc == 0 and calls == ["--sizes 4096 --devices all --dtype mxfp4"]
    assert [r["test"] for r in rs] == ["gemm", "gemm_summary", "validator"]
    assert rs[1]["dtype"] == "mxfp4"


def test_validator_still_rejects_fp4_without_the_mx_prefix(capsys):
    with pytest.raises(SystemExit) as ei:
        V.main(["--tests", "gemm", "--gemm-dtypes", "bf16,fp4"])
    assert ei.value.code != 0
    assert V.parse_gemm_dtypes("bf16,mxfp8,mxfp4") == ["bf16", "mxfp8", "mxfp4"]
    with pytest.raises(ValueError):
        V.parse_gemm_dtypes("mxfp4,mxfp4")


# ---- build hygiene ----------------------------------------------------------------
@pytest.mark.skipif(not mx.HIPCC, reason="no hipcc")
def test_gemm_kernel_has_no_scratch_and_uses_the_scaled_mfma_on_e2m1():
    asm, by = mx.kernel_listing(mx.MXFP4)
    mfma = re.findall(r"v_mfma_scale_f32_32x32x64_f8f6f4[^\n]*", asm)
    assert mfma and all("cbsz:4" in m and "blgp:4" in m for m in mfma), mfma[:3]
    gemm = [n for n in by if "gemm" in n]
    assert len(gemm) == 1 and "mxk_gemm_mxfp4_tn_kernel" in gemm[0], by
    rows = mx.check_quantiser_kernels(mx.MXFP4, by, "quantize_rows_kernel", 2)   # vector, element-wise
    tr = mx.check_quantiser_kernels(mx.MXFP4, by, "quantize_tr_kernel", 4)
    assert sorted(by) == sorted(gemm + rows + tr)            # 7 kernels and no other
    assert all(v == 0 for m in by.values() for v in m.values()), by


def test_host_sweep_of_the_format_header():
    """make test-mxfp4-format: every finite bf16 at every admissible block
    exponent against a brute-force search, under ASan + UBSan."""
    p = subprocess.run(["make", "-C", REPO, "test-mxfp4-format"], capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert "all equal to the brute-force search" in p.stdout
