"""Hand-written CDNA4 (gfx950) HIP kernels exposed as torch ops.

* :func:`gemm_bf16_tn`  — bf16 MFMA GEMM (validator config 3)
* :func:`quantize_mxfp8`, :func:`gemm_mxfp8_tn` — MXFP8 (block-scaled e4m3) quantiser
  and scaled-MFMA GEMM (validator config 3, ``--gemm-dtypes mxfp8``);
  :func:`quantize_mxfp8_t`, :func:`quantize_mxfp8_dual` — the transposing quantiser,
  :func:`linear_mxfp8` — a linear layer's three products on that GEMM (opt-in)
* :func:`quantize_mxfp4`, :func:`gemm_mxfp4_tn` — MXFP4 (block-scaled e2m1, two codes per
  byte) quantiser and scaled-MFMA GEMM (validator config 3, ``--gemm-dtypes mxfp4``);
  :func:`quantize_mxfp4_t`, :func:`quantize_mxfp4_dual` — the transposing quantiser,
  :func:`linear_mxfp4` — a linear layer's three products on that GEMM (opt-in);
  ``rounding="stochastic"`` on the quantisers and ``grad_rounding="stochastic"`` on the
  layer round the output gradient stochastically, seeds from :func:`sr_reseed` /
  :func:`sr_next`
* :func:`swiglu_mlp_mx` — the SwiGLU MLP of the MX routes as one node: SwiGLU and its
  gradient computed inside the quantisers (``swiglu_quantize_<fmt>``, ``.._t``,
  ``swiglu_bwd_quantize_<fmt>_dual`` of :mod:`mxk8s.ops.mxfp8` / :mod:`mxk8s.ops.mxfp4`)
* :func:`vector_add`    — smoke-test payload (config 2)
* :func:`rmsnorm`, :func:`swiglu`, :func:`rope` — fused training ops (config 5)
"""
from .gemm import gemm_bf16_tn, gemm_flops, is_fast_shape
from .mxfp8 import (quantize_mxfp8, quantize_mxfp8_ref, quantize_mxfp8_t, quantize_mxfp8_dual,
                    dequantize_mxfp8, gemm_mxfp8_tn, is_fast_shape_mxfp8)
from .mxfp4 import (quantize_mxfp4, quantize_mxfp4_ref, quantize_mxfp4_t, quantize_mxfp4_dual,
                    dequantize_mxfp4, gemm_mxfp4_tn, is_fast_shape_mxfp4, sr_reseed, sr_next)
from .linear import (linear_mxfp8, is_mxfp8_linear_shape, linear_mxfp4, is_mxfp4_linear_shape,
                     swiglu_mlp_mx)
from .vector_add import vector_add
from .fused import rmsnorm, swiglu, rope, rope_tables
from ._lib import kernels_available, KERNEL_LIB_PATH

__all__ = ["gemm_bf16_tn", "gemm_flops", "is_fast_shape", "quantize_mxfp8", "quantize_mxfp8_ref",
           "quantize_mxfp8_t", "quantize_mxfp8_dual", "linear_mxfp8", "is_mxfp8_linear_shape",
           "dequantize_mxfp8", "gemm_mxfp8_tn", "is_fast_shape_mxfp8", "quantize_mxfp4",
           "quantize_mxfp4_ref", "quantize_mxfp4_t", "quantize_mxfp4_dual", "linear_mxfp4",
           "is_mxfp4_linear_shape", "dequantize_mxfp4", "gemm_mxfp4_tn", "is_fast_shape_mxfp4",
           "sr_reseed", "sr_next", "swiglu_mlp_mx", "vector_add", "rmsnorm", "swiglu", "rope", "rope_tables", "kernels_available", "KERNEL_LIB_PATH"]
