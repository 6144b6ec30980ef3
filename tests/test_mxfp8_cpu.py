"""MXFP8 (block-scaled e4m3) path, everything that needs no GPU: the reference
quantiser, the op's contract, validator and chart plumbing, build hygiene of
``native/kernels/gemm_mxfp8.hip``."""
import json
import os

import pytest
import torch

import mx_gemm_checks as mx
import mxk8s.validate.__main__ as V
from mx_gemm_checks import BF16_LINE, fake_bench, run_validator
from mxk8s import config
from mxk8s.chart import render
from mxk8s.ops import _lib
from mxk8s.ops.mxfp8 import (dequantize_mxfp8, gemm_mxfp8_tn, is_fast_shape_mxfp8, quantize_mxfp8,
                             quantize_mxfp8_ref)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wide(rows, K, seed, lo=-40, hi=40):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, K), generator=g)
    e = torch.randint(lo, hi, (rows, K), generator=g)
    return torch.ldexp(x, e).bfloat16()


# ---- reference quantiser ------------------------------------------------------
def test_block_maxima_land_in_256_512_before_clamping():
    x = _wide(64, 1152, 1)
    _, s = quantize_mxfp8_ref(x)
    e = s.to(torch.int32) - 127
    amax = x.float().reshape(64, -1, 32).abs().amax(dim=2)
    scaled = torch.ldexp(amax, -e)
    assert torch.all((scaled >= 256) & (scaled < 512))


def test_no_nan_and_about_one_percent_saturates_on_wide_range_data():
    q, _ = quantize_mxfp8_ref(_wide(64, 1152, 2))
    f = q.float()
    assert not torch.isnan(f).any()
    assert f.abs().max().item() == 448.0
    assert 0 < (f.abs() == 448).float().mean().item() < 0.03
    assert (q.view(torch.uint8) & 0x7f).max().item() <= 0x7e       # never the NaN code


def test_zero_block_gives_byte_127_and_zero_elements():
    x = (torch.rand(4, 96) + 0.5).bfloat16()
    x[1, 32:64] = 0
    x[2, 64:96] = -0.0
    q, s = quantize_mxfp8_ref(x)
    assert s[1, 1].item() == 127 and s[2, 2].item() == 127
    assert torch.all(q[1, 32:64].float() == 0) and torch.all(q[2, 64:96].float() == 0)
    assert s[0, 0].item() != 127 or x[0, :32].float().abs().max() >= 256


@pytest.mark.parametrize("e", [-100, -9, 0, 7, 100])
def test_448_survives_and_500_saturates(e):
    x = torch.zeros(2, 32)
    x[0, 3], x[0, 4] = 448.0, -448.0
    x[1, 3], x[1, 4] = 500.0, -500.0
    x = torch.ldexp(x, torch.tensor(e)).bfloat16()
    q, s = quantize_mxfp8_ref(x)
    assert s[0, 0].item() == e + 127 and s[1, 0].item() == e + 127
    d = dequantize_mxfp8(q, s)
    want = torch.ldexp(torch.tensor(448.0), torch.tensor(e))
    assert d[0, 3] == want and d[0, 4] == -want
    assert d[1, 3] == want and d[1, 4] == -want


def test_scale_exponent_clamps_and_subnormal_input():
    x = torch.zeros(2, 32, dtype=torch.bfloat16)
    x[0, 0] = 2.0 ** -133                                   # smallest bf16 subnormal
    x[1, 0] = 2.0 ** 127
    q, s = quantize_mxfp8_ref(x)
    assert s[0, 0].item() == 0 and s[1, 0].item() == 127 + 119
    assert q[0, 0].float().item() == 2.0 ** -6 and q[1, 0].float().item() == 256.0   # 2^-133 2^127


def test_round_trip_of_a_tensor_on_the_mx_grid_is_the_identity():
    """A tensor on the MX grid is a dequantised quantiser output: its block
    maxima sit in [256, 448] x 2^e, so the same scale is chosen again and every
    element is kept.  (Arbitrary code / scale pairs are not on that grid: a
    block whose largest code is 240 is re-scaled to 480 and saturates.)"""
    for x0 in (_wide(32, 256, 3), (torch.rand(32, 256) * 2 - 1).bfloat16()):
        q0, s0 = quantize_mxfp8_ref(x0)
        x = dequantize_mxfp8(q0, s0)
        assert torch.equal(x.bfloat16().float(), x)         # the MX grid is inside bf16
        q, s = quantize_mxfp8_ref(x.bfloat16())
        assert torch.equal(s, s0) and torch.equal(q.view(torch.uint8), q0.view(torch.uint8))
        assert torch.equal(dequantize_mxfp8(q, s), x)


def test_cpu_quantize_is_the_reference():
    x = _wide(8, 64, 4)
    q, s = quantize_mxfp8(x)
    qr, sr = quantize_mxfp8_ref(x)
    assert torch.equal(q.view(torch.uint8), qr.view(torch.uint8)) and torch.equal(s, sr)


def test_product_of_any_two_e4m3_values_is_exact_in_bf16():
    """4 + 4 significand bits fit bf16's 8, and the exponent range is far
    inside bf16's: the one-hot GPU test's bit-equality rests on this."""
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    v = codes.view(torch.float8_e4m3fn).float()
    v = v[torch.isfinite(v)]
    assert v.numel() == 254
    p = v[:, None].double() * v[None, :].double()
    assert torch.equal(p.float().bfloat16().double(), p)


# ---- shape and dtype contract (nothing here may load the library) ---------------
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the kernel library was loaded")
    monkeypatch.setattr(_lib, "lib", boom)


def _pair(rows, K, dev="cpu"):
    q = torch.zeros((rows, K), dtype=torch.uint8, device=dev).view(torch.float8_e4m3fn)
    s = torch.full((rows, K // 32), 127, dtype=torch.uint8, device=dev)
    return q, s


@pytest.mark.parametrize("dev", ["cpu", "meta"])
def test_gemm_contract_raises_before_the_library(no_library, dev):
    a, a_s = _pair(256, 128, dev)
    b, b_s = _pair(256, 128, dev)
    with pytest.raises(ValueError, match="M % 256"):
        gemm_mxfp8_tn(*_pair(128, 128, dev), b, b_s)            # M = 128
    with pytest.raises(ValueError, match="K % 128"):
        gemm_mxfp8_tn(*_pair(256, 64, dev), *_pair(256, 64, dev))   # K = 64
    with pytest.raises(ValueError, match="K mismatch"):
        gemm_mxfp8_tn(a, a_s, *_pair(256, 256, dev))
    with pytest.raises(TypeError):
        gemm_mxfp8_tn(a.view(torch.uint8), a_s, b, b_s)         # wrong element dtype
    with pytest.raises(TypeError):
        gemm_mxfp8_tn(a, a_s.to(torch.int8), b, b_s)            # wrong scale dtype
    with pytest.raises(TypeError):
        gemm_mxfp8_tn(a, a_s, b, b_s, out=torch.empty((256, 256), dtype=torch.float32, device=dev))
    wide, _ = _pair(256, 256, dev)
    with pytest.raises(ValueError, match="K-contiguous"):
        gemm_mxfp8_tn(wide[:, ::2], a_s, b, b_s)                # non-unit inner stride
    with pytest.raises(ValueError, match=r"a_s must be \[256, 4\]"):
        gemm_mxfp8_tn(a, torch.full((256, 3), 127, dtype=torch.uint8, device=dev), b, b_s)
    with pytest.raises(ValueError, match=r"b_s must be \[256, 4\]"):
        gemm_mxfp8_tn(a, a_s, b, torch.full((128, 4), 127, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="out must be"):
        gemm_mxfp8_tn(a, a_s, b, b_s, out=torch.empty((256, 128), dtype=torch.bfloat16, device=dev))


@pytest.mark.parametrize("dev", ["cpu", "meta"])
def test_quantize_contract_raises_before_the_library(no_library, dev):
    with pytest.raises(TypeError):
        quantize_mxfp8(torch.zeros((4, 32), device=dev))                       # fp32
    with pytest.raises(ValueError):
        quantize_mxfp8(torch.zeros((4, 48), dtype=torch.bfloat16, device=dev))  # K % 32
    with pytest.raises(ValueError):
        quantize_mxfp8(torch.zeros((4, 64), dtype=torch.bfloat16, device=dev)[:, ::2])
    with pytest.raises(ValueError):
        quantize_mxfp8(torch.zeros((32,), dtype=torch.bfloat16, device=dev))


def test_gpu_layout_limits_raise_before_the_library(no_library):
    """Element rows 16-byte, scale rows 4-byte aligned (checked for device
    tensors only; 'meta' stands in for one here)."""
    a, a_s = _pair(256, 128, "meta")
    odd = torch.zeros((256, 136), dtype=torch.uint8, device="meta").view(torch.float8_e4m3fn)[:, :128]
    with pytest.raises(ValueError, match="16 bytes"):
        gemm_mxfp8_tn(odd, a_s, a, a_s)
    s_odd = torch.zeros((256, 6), dtype=torch.uint8, device="meta")[:, :4]
    with pytest.raises(ValueError, match="4 bytes"):
        gemm_mxfp8_tn(a, s_odd, a, a_s)


def test_is_fast_shape():
    assert is_fast_shape_mxfp8(256, 512, 128) and is_fast_shape_mxfp8(8192, 8192, 8192)
    assert not is_fast_shape_mxfp8(256, 256, 64) and not is_fast_shape_mxfp8(128, 256, 128)
    assert not is_fast_shape_mxfp8(0, 256, 128)


def test_cpu_path_is_the_dequantised_fp32_product_rounded_to_bf16():
    g = torch.Generator().manual_seed(5)
    aq, a_s = quantize_mxfp8((torch.rand((256, 384), generator=g) * 2 - 1).bfloat16())
    bq, b_s = quantize_mxfp8(_wide(512, 384, 6, -6, 6))
    want = (dequantize_mxfp8(aq, a_s) @ dequantize_mxfp8(bq, b_s).t()).bfloat16()
    got = gemm_mxfp8_tn(aq, a_s, bq, b_s)
    assert got.dtype == torch.bfloat16 and torch.equal(got, want)
    # views: a K slice of q with the matching column slice of s, and out=
    out = torch.empty((256, 520), dtype=torch.bfloat16)[:, :512]
    r = gemm_mxfp8_tn(aq[:, 128:], a_s[:, 4:], bq[:, 128:], b_s[:, 4:], out=out)
    assert r is out
    want2 = (dequantize_mxfp8(aq[:, 128:], a_s[:, 4:]) @
             dequantize_mxfp8(bq[:, 128:], b_s[:, 4:]).t()).bfloat16()
    assert torch.equal(out, want2)


def test_fp8_error_against_the_bf16_product_is_the_formats_own():
    """~7 % in Frobenius norm for uniform [-1, 1): why no check compares
    against the unquantised product."""
    g = torch.Generator().manual_seed(7)
    x = (torch.rand((256, 256), generator=g) * 2 - 1).bfloat16()
    y = (torch.rand((256, 256), generator=g) * 2 - 1).bfloat16()
    c = gemm_mxfp8_tn(*quantize_mxfp8(x), *quantize_mxfp8(y)).float()
    ref = x.float() @ y.float().t()
    rel = ((c - ref).norm() / ref.norm()).item()
    assert 0.03 < rel < 0.12, rel


# ---- validator plumbing ---------------------------------------------------------
def test_validator_default_runs_bf16_once_with_todays_lines(tmp_path, monkeypatch, capsys):
    fake_bench(tmp_path)
    rc, rs, calls = run_validator(tmp_path, monkeypatch, capsys, ["--tests", "gemm"])
    assert rc == 0
    assert calls == ["--sizes 4096,8192,16384 --devices all"]
    assert rs[0] == json.loads(BF16_LINE)
    assert rs[1] == {"test": "gemm_summary", "gpus": 1, "aggregate_tflops": {"4096": 1300.0},
                     "pass": True}
    assert [r["test"] for r in rs] == ["gemm", "gemm_summary", "validator"]
    assert rs[2]["results"] == {"gemm": True}


def test_validator_two_dtypes_two_runs_two_summaries(tmp_path, monkeypatch, capsys):
    fake_bench(tmp_path)
    rc, rs, calls = run_validator(tmp_path, monkeypatch, capsys,
                                  ["--tests", "gemm", "--gemm-dtypes", "bf16,mxfp8",
                                   "--gemm-sizes", "4096"])
    assert rc == 0
    assert calls == ["--sizes 4096 --devices all", "--sizes 4096 --devices all --dtype mxfp8"]
    summ = [r for r in rs if r["test"] == "gemm_summary"]
    assert len(summ) == 2 and "dtype" not in summ[0]
    assert summ[1]["dtype"] == "mxfp8" and summ[1]["aggregate_tflops"] == {"4096": 2500.0}
    assert summ[1]["pass"] is True
    lines = [r for r in rs if r["test"] == "gemm"]
    assert [r["dtype"] for r in lines] == ["bf16", "mxfp8"] and "quantize_ms" in lines[1]


@pytest.mark.parametrize("mx_rc", [0, 1])
def test_validator_fails_on_a_failing_mxfp8_line(tmp_path, monkeypatch, capsys, mx_rc):
    fake_bench(tmp_path, "mxfp8", ok=False, rc=mx_rc)
    rc, rs, _ = run_validator(tmp_path, monkeypatch, capsys,
                              ["--tests", "gemm", "--gemm-dtypes", "bf16,mxfp8"])
    assert rc == 1
    assert rs[-1]["test"] == "validator" and rs[-1]["pass"] is False
    assert [r for r in rs if r.get("dtype") == "mxfp8" and r["test"] == "gemm_summary"][0]["pass"] is False


def test_validator_rejects_unknown_dtype(capsys):
    with pytest.raises(SystemExit):
        V.main(["--tests", "gemm", "--gemm-dtypes", "bf16,fp4"])
    assert V.parse_gemm_dtypes("mxfp8") == ["mxfp8"]
    with pytest.raises(ValueError):
        V.parse_gemm_dtypes("bf16,bf16")


# ---- chart ----------------------------------------------------------------------
def _validator_args(sets=()):
    docs = render.manifests(render.render(render.load_values(sets=list(sets))))
    job = next(d for d in docs if d["kind"] == "Job" and d["metadata"]["name"].endswith("validator"))
    return job["spec"]["template"]["spec"]["containers"][0]["args"]


def test_chart_default_render_has_no_gemm_dtypes_argument():
    assert not [a for a in _validator_args() if a.startswith("--gemm-dtypes")]
    assert not [a for a in _validator_args(["validator.gemm.dtypes={bf16}"])
                if a.startswith("--gemm-dtypes")]
    with open(os.path.join(REPO, "deploy", "amd-gpu-stack.yaml")) as f:
        assert "--gemm-dtypes" not in f.read()


def test_chart_set_dtypes_adds_the_argument():
    args = _validator_args(["validator.gemm.dtypes={bf16,mxfp8}"])
    assert "--gemm-dtypes=bf16,mxfp8" in args
    assert args.index("--gemm-dtypes=bf16,mxfp8") == args.index("--gemm-sizes=4096,8192,16384") + 1
    assert "--gemm-dtypes=mxfp8" in _validator_args(["validator.gemm.dtypes={mxfp8}"])


def test_chart_schema_rejects_unknown_dtype():
    assert config.validate_values(render.load_values(sets=["validator.gemm.dtypes={bf16,mxfp8}"])) == []
    errs = config.validate_values(render.load_values(sets=["validator.gemm.dtypes={bf16,fp4}"]))
    assert errs and any("dtypes" in e for e in errs), errs
    with open(os.path.join(REPO, "charts", "amd-gpu-stack", "values.schema.json")) as f:
        schema = json.load(f)
    dt = schema["properties"]["validator"]["properties"]["gemm"]["properties"]["dtypes"]
    assert dt["items"]["enum"] == ["bf16", "mxfp8"]


# ---- build hygiene ----------------------------------------------------------------
@pytest.mark.skipif(not mx.HIPCC, reason="no hipcc")
def test_gemm_kernel_has_no_scratch_and_uses_the_scaled_mfma():
    asm, by = mx.kernel_listing(mx.MXFP8)
    assert "v_mfma_scale_f32_32x32x64_f8f6f4" in asm
    gemm = [n for n in by if "mxk_gemm_mxfp8_tn_kernel" in n]
    assert len(gemm) == 1, by
    assert by[gemm[0]]["private_segment_fixed_size"] == 0, by
    mx.check_quantiser_kernels(mx.MXFP8, by, "quantize_rows_kernel", 2)   # vector, element-wise
    assert all(v["vgpr_spill_count"] == 0 for v in by.values()), by
