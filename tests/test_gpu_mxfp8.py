"""MXFP8 quantiser and scaled-MFMA GEMM on the GPU (``native/kernels/gemm_mxfp8.hip``).

Every check compares against the product of the DEQUANTISED operands: against
the unquantised bf16 product the format's own error is about 7 %.  The check
bodies are shared with the MXFP4 file (``tests/mx_gemm_checks.py``); the shapes
here are this kernel's (K-tile 128).
"""
import pytest

import mx_gemm_checks as mx

pytestmark = pytest.mark.gpu

F = mx.MXFP8


# ---- 1. one-hot lane map ---------------------------------------------------
@pytest.mark.parametrize("pa,pb", [((37, 5), (53, 11)), ((91, 3), (29, 7)), ((113, 64), (77, 130))])
def test_one_hot_lane_map(cuda_device, pa, pb):
    """Every product here is a single term and exactly representable in bf16
    (tests/test_mxfp8_cpu.py asserts that over all code pairs), so the kernel
    must reproduce the CPU dequantised product bit for bit.  A permuted k
    order, a scale taken from the wrong block, row or register byte, swapped
    operand roles or a transposed store all change some element."""
    mx.one_hot_lane_map(F, cuda_device, 256, pa, pb)


# ---- 2. random operands against the dequantised reference -------------------
@pytest.mark.parametrize("M,N,K", [(256, 256, 128), (256, 256, 256), (512, 768, 384),
                                   (768, 256, 512), (512, 512, 640), (256, 512, 1152)])
def test_random_vs_dequantised_fp32(cuda_device, M, N, K):
    mx.random_vs_dequantised(F, cuda_device, M, N, K)


def test_more_than_one_xcd_round(cuda_device):
    """64 tiles: more than one XCD's 32 CUs' worth, a non-square tile map."""
    mx.random_vs_dequantised(F, cuda_device, 1024, 4096, 256, seed=33)


def test_padded_strides_and_untouched_padding(cuda_device):
    """Views into wider buffers whose padding holds NaN bytes (0x7f e4m3,
    0xff E8M0): lda, ldb, ldc and both scale strides exceed the widths.  Then
    a K slice of q (k = 128 .. 383) with the matching column slice of s."""
    mx.padded_strides_and_untouched_padding(F, cuda_device, 512, 256, 384)


def test_block_scales_spread(cuda_device):
    """bf16 data multiplied per block by 2^-6 .. 2^6: the scales differ from
    block to block and row to row."""
    mx.block_scales_spread(F, cuda_device)


# ---- 3. quantiser ------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "wide", "zero_blocks", "strided"])
@pytest.mark.parametrize("K", [32, 96, 1152])
@pytest.mark.parametrize("R", [1, 3, 256])
def test_quantiser_bit_equal_to_reference(cuda_device, R, K, kind):
    mx.quantiser_bit_equal_to_reference(F, mx._quant_inputs(R, K, kind, cuda_device))


def test_quantiser_unaligned_rows(cuda_device):
    """A view whose rows are not 16-byte aligned takes the element-wise path."""
    mx.quantiser_bit_equal_to_reference(F, mx.unaligned_rows(cuda_device))


# ---- 4. poisoned output, run-to-run identity ----------------------------------
def test_poisoned_output_and_run_to_run_identity(cuda_device):
    mx.poisoned_output_and_run_to_run_identity(F, cuda_device, 512, 512, 640)


def test_contract_violation_launches_nothing(cuda_device):
    mx.contract_violation_launches_nothing(F, cuda_device)


# ---- 5. mx-gemm-bench --dtype mxfp8 -------------------------------------------
def test_gemm_bench_mxfp8_self_checks():
    mx.gemm_bench_self_checks(F)


def test_gemm_bench_mxfp8_fails_when_kernel_skipped():
    mx.gemm_bench_fails_when_kernel_skipped(F)
