"""MXFP8 linear layers, everything that needs no GPU: the transposing
quantiser's reference path and contract, ``linear_mxfp8`` against its three
products written out by hand, the ``main_grad`` protocol, the shape fallback of
``Linear(compute="mxfp8")``, the model and trainer wiring, build hygiene of the
quantiser kernels.  The bodies are ``mx_linear_checks``', shared with MXFP4."""
import pytest

import mx_gemm_checks as mx
import mx_linear_checks as lc
from mx_linear_checks import no_library  # noqa: F401  (fixture)

F = lc.MXFP8


# ---- transposed quantiser: reference path and contract -----------------------------
@pytest.mark.parametrize("R,C", [(32, 1), (96, 3), (64, 100), (256, 32)])
def test_cpu_quantize_t_is_the_reference_of_the_transposed_copy(no_library, R, C):  # noqa: F811
    lc.cpu_quantize_t_is_the_reference_of_the_transposed_copy(F, R, C)


def test_cpu_quantize_dual_is_both_references(no_library):  # noqa: F811
    lc.cpu_quantize_dual_is_both_references(F)


@pytest.mark.parametrize("dev", ["cpu", "meta"])
def test_quantize_t_contract_raises_before_the_library(no_library, dev):  # noqa: F811
    lc.quantize_t_contract_raises_before_the_library(F, dev)


# ---- linear_mxfp8 on the CPU ------------------------------------------------------
@pytest.mark.parametrize("T,i,o", [(256, 256, 256), (256, 512, 256), (512, 256, 768)])
def test_linear_mxfp8_cpu_equals_the_products_by_hand(no_library, T, i, o):  # noqa: F811
    lc.linear_cpu_equals_the_products_by_hand(F, T, i, o)


def test_linear_mxfp8_casts_other_dtypes_and_strided_dy(no_library):  # noqa: F811
    lc.linear_casts_other_dtypes_and_strided_dy(F)


def test_only_the_needed_gradients_are_computed(no_library, monkeypatch):  # noqa: F811
    lc.only_the_needed_gradients_are_computed(F, monkeypatch)


def test_dy_is_read_once_when_both_gradients_are_needed(no_library, monkeypatch):  # noqa: F811
    lc.dy_is_read_once_when_both_gradients_are_needed(F, monkeypatch)


# ---- main_grad protocol -----------------------------------------------------------
def test_main_grad_fresh_overwrites_then_accumulates(no_library):  # noqa: F811
    lc.main_grad_fresh_overwrites_then_accumulates(F)


def test_without_main_grad_the_weight_gradient_is_returned(no_library):  # noqa: F811
    lc.without_main_grad_the_weight_gradient_is_returned(F)


# ---- shape fallback ---------------------------------------------------------------
def test_is_mxfp8_linear_shape():
    lc.is_linear_shape(F)


@pytest.mark.parametrize("T,i", [(100, 256), (256, 384)])
def test_linear_falls_back_to_bf16_on_other_shapes(no_library, monkeypatch, T, i):  # noqa: F811
    lc.linear_falls_back_to_bf16_on_other_shapes(F, monkeypatch, T, i)


def test_linear_compute_argument():
    lc.linear_compute_argument(F)


def test_swiglu_linear_mxfp8_is_the_plain_composition(no_library):  # noqa: F811
    lc.swiglu_linear_is_the_plain_composition(F)


# ---- model wiring -----------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_pair():
    return lc.tiny_pair(F)


def test_model_routes_24_products_and_none_by_default(tiny_pair):
    lc.model_routes_24_products_and_none_by_default(F, tiny_pair)


def test_model_loss_and_gradients_against_the_fp32_model(tiny_pair):
    """Conditions that catch a wrong axis or transposition, not accuracy claims:
    |loss - loss_fp32| < 0.05 and every gradient finite with a cosine >= 0.9
    against the fp32 model.  The reference emulation alone is within 0.001 in
    the loss and 0.14 relative (a cosine of about 0.99) in the worst gradient."""
    assert (F.loss_tol, F.min_cos) == (0.05, 0.9)
    lc.model_loss_and_gradients_against_the_fp32_model(F, tiny_pair)


# ---- trainer switch -----------------------------------------------------------------
def test_trainer_switch_reaches_the_config(monkeypatch):
    lc.trainer_switch_reaches_the_config(F, monkeypatch)


def test_trainer_rejects_an_unknown_value(monkeypatch, capsys):
    import mxk8s.train.ddp_llama as D
    with pytest.raises(SystemExit):
        D.main(["--tiny", "--linear-dtype", "fp4"])
    capsys.readouterr()
    monkeypatch.setenv("MXK_LINEAR_DTYPE", "fp4")
    with pytest.raises(ValueError, match="fp4"):
        D.run_ddp_bench(lc.bench_namespace())


def test_trainer_tiny_step_on_the_cpu_reports_linear_dtype(monkeypatch, capsys):
    """One CPU step of the tiny model through FlatDDP with MXFP8 linears: the
    weight gradients go into the flat buffer through out=."""
    lc.trainer_tiny_step_on_the_cpu_reports_linear_dtype(F, monkeypatch, capsys)


# ---- build hygiene ------------------------------------------------------------------
@pytest.mark.skipif(not mx.HIPCC, reason="no hipcc")
def test_transposing_quantiser_kernels_have_no_scratch():
    lc.transposing_quantiser_kernels_have_no_scratch(F)
