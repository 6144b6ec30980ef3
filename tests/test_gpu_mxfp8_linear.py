"""Transposing MXFP8 quantiser and ``linear_mxfp8`` on the GPU
(``native/kernels/mx_quantize.h`` on the format of ``native/kernels/gemm_mxfp8.hip``,
``mxk8s/ops/linear.py``).  The bodies are ``mx_linear_checks``', shared with MXFP4.

The quantisers are bit-equal to the reference, so the products are compared
with the fp64 product of the dequantised *reference-quantised* operands under
the project's bf16-output criterion (``mx_gemm_checks._check``).
"""
import pytest

import mx_linear_checks as lc

pytestmark = pytest.mark.gpu

F = lc.MXFP8


# ---- 1. quantisers ------------------------------------------------------------
KINDS = ["uniform", "wide", "zero_blocks", "strided"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [1, 3, 32, 100, 256])
@pytest.mark.parametrize("R", [32, 96, 256, 1152])
def test_quantize_t_bit_equal_to_reference(cuda_device, R, C, kind):
    lc.quantize_t_bit_equal_to_reference(F, cuda_device, R, C, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [32, 256])
@pytest.mark.parametrize("R", [32, 96, 256, 1152])
def test_quantize_dual_bit_equal_to_reference(cuda_device, R, C, kind):
    lc.quantize_dual_bit_equal_to_reference(F, cuda_device, R, C, kind)


@pytest.mark.parametrize("R,C", [(32, 1), (160, 72), (96, 64)])
def test_quantisers_unaligned_views(cuda_device, R, C):
    """Rows of x that are not 16-byte aligned, and output rows that are not
    8-byte aligned (3 bytes of padding for qt alone, 5 for qt and q of the dual
    kernel), take the element-wise path."""
    lc.quantisers_unaligned_views(F, cuda_device, R, C)


def test_contract_violation_launches_nothing(cuda_device):
    """R % 32, ldqt < R, and for the dual entry C % 32."""
    lc.contract_violation_launches_nothing(F, cuda_device)


# ---- 2. the three products -------------------------------------------------------
SHAPES = [(256, 256, 256), (512, 256, 768), (256, 1024, 512), (256, 512, 1024)]


@pytest.mark.parametrize("T,i,o", SHAPES)
def test_products_against_dequantised_fp64(cuda_device, T, i, o):
    lc.products_against_dequantised_fp64(F, cuda_device, T, i, o)


def test_main_grad_fresh_then_accumulate(cuda_device):
    lc.main_grad_fresh_then_accumulate(F, cuda_device)


def test_run_to_run_identity(cuda_device):
    lc.run_to_run_identity(F, cuda_device)


# ---- 3. model ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def fp32_reference():
    return lc.fp32_reference()


def test_tiny_llama_mxfp8_against_fp32_cpu(cuda_device, fp32_reference, monkeypatch):
    """Plumbing conditions, not accuracy claims (the CPU file's docstring has the
    figures of the reference emulation alone): |loss - loss_fp32| < 0.05, every
    gradient finite with a cosine >= 0.9 against the fp32 model."""
    assert (F.loss_tol, F.min_cos) == (0.05, 0.9)
    lc.tiny_llama_against_fp32_cpu(F, cuda_device, fp32_reference, monkeypatch)


def test_three_train_steps_leave_finite_parameters(cuda_device):
    lc.three_train_steps_leave_finite_parameters(F, cuda_device)
