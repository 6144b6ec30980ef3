"""MXFP4 quantiser and scaled-MFMA GEMM on the GPU (``native/kernels/gemm_mxfp4.hip``).

Every check compares against the product of the DEQUANTISED operands: against
the unquantised bf16 product the format's own error is about 21 %.  The check
bodies are shared with the MXFP8 file (``tests/mx_gemm_checks.py``); the shapes
here are this kernel's (K-tile 256).
"""
import pytest

import mx_gemm_checks as mx

pytestmark = pytest.mark.gpu

F = mx.MXFP4


# ---- 1. one-hot lane map ---------------------------------------------------
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
    mx.one_hot_lane_map(F, cuda_device, K, pa, pb)


# ---- 2. random operands against the dequantised reference -------------------
@pytest.mark.parametrize("M,N,K", [(256, 256, 256),      # one K-tile, no DMA in the loop
                                   (256, 256, 512),      # the no-DMA tail only
                                   (512, 768, 768),      # the DMA loop runs once, 2-D tile map
                                   (768, 256, 1280),     # five K-tiles: both buffers refilled
                                   (1024, 4096, 256)])   # 64 tiles: more than one XCD round
def test_random_vs_dequantised_fp64(cuda_device, M, N, K):
    mx.random_vs_dequantised(F, cuda_device, M, N, K)


# ---- 3. block scales spread ---------------------------------------------------
def test_block_scales_spread(cuda_device):
    """bf16 data multiplied per block by 2^-6 .. 2^6: the scales differ from
    block to block and row to row."""
    mx.block_scales_spread(F, cuda_device)


# ---- 4. padded strides ----------------------------------------------------------
def test_padded_strides_and_untouched_padding(cuda_device):
    """Views into wider buffers whose padding holds 0xFF bytes (two -6 codes,
    the E8M0 NaN): lda, ldb, ldc and both scale strides exceed the widths.
    Then a K slice of q (k = 256 .. 767: bytes 128 .. 383) with the matching
    column slice of s."""
    mx.padded_strides_and_untouched_padding(F, cuda_device, 512, 256, 768)


# ---- 5. quantiser ------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "wide", "zero_blocks", "strided"])
@pytest.mark.parametrize("K", [32, 96, 1152])
@pytest.mark.parametrize("R", [1, 3, 256])
def test_quantiser_bit_equal_to_reference(cuda_device, R, K, kind):
    mx.quantiser_bit_equal_to_reference(F, mx._quant_inputs(R, K, kind, cuda_device))


def test_quantiser_unaligned_rows(cuda_device):
    """A view whose rows are not 16-byte aligned takes the element-wise path."""
    mx.quantiser_bit_equal_to_reference(F, mx.unaligned_rows(cuda_device))


# ---- 6. poisoned output, run-to-run identity ----------------------------------
def test_poisoned_output_and_run_to_run_identity(cuda_device):
    mx.poisoned_output_and_run_to_run_identity(F, cuda_device, 512, 512, 1280)


# ---- 7. contract violation ------------------------------------------------------
def test_contract_violation_launches_nothing(cuda_device):
    mx.contract_violation_launches_nothing(F, cuda_device)


# ---- 8. mx-gemm-bench --dtype mxfp4 -------------------------------------------
def test_gemm_bench_mxfp4_self_checks():
    mx.gemm_bench_self_checks(F)


def test_gemm_bench_mxfp4_fails_when_kernel_skipped():
    mx.gemm_bench_fails_when_kernel_skipped(F)
