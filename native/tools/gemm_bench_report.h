// mx-gemm-bench's verdict and RESULT line, in plain C++17 (no HIP): which
// 256x256 block is spot-checked, its tolerance, the pass rule and the line's
// text.  make test-gemm-bench-report pins every string here, quirks included
// (they are listed in gemm_bench_main.hip).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

namespace gemm_bench {

// JSON has no inf / NaN
inline std::string json_num(double v) {
  if (!std::isfinite(v)) return "null";
  char b[32];
  std::snprintf(b, sizeof(b), "%.4g", v);
  return b;
}

struct SpotBlock {
  int r0, c0;
};

// the pseudo-random 256x256 block of an n x n output (n a multiple of 256)
inline SpotBlock spot_block(int n, int dev) {
  const uint32_t h32 = (0x9E3779B1u * uint32_t(n)) ^ (0x85EBCA6Bu * uint32_t(dev + 1));
  const uint32_t blocks = uint32_t(n / 256);
  return {int(h32 % blocks) * 256, int((h32 >> 16) % blocks) * 256};
}

// 2^-7 max|ref|: bf16 output rounding is 2^-8
inline float spot_tolerance(float max_ref) { return 0.0078125f * max_ref; }

// nullptr when the block passes, else the error text
inline const char* spot_error(float max_abs_err, float max_ref) {
  if (max_ref > 0.f && max_abs_err <= spot_tolerance(max_ref)) return nullptr;
  return max_ref > 0.f ? "fp32 spot check failed" : "fp32 spot check: reference block is zero";
}

struct Result {
  const char* dtype = "bf16";
  bool mx = false;            // quantised operands: quantize_ms, no library reference
  bool ref = true;            // bf16 only: rel was measured against rocBLAS and is judged
  int gpu = 0, n = 0;
  double median_s = 0;        // median launch, seconds
  float min_ms = 0;
  double rel = -1;            // bf16 only; -1 when not measured
  SpotBlock block{0, 0};
  float max_abs_err = 0, max_ref = 0;
  float quantize_ms = 0;      // MX only
  std::string error;          // the first error met; empty when there was none
};

inline bool passes(const Result& r) {
  return r.error.empty() && (r.mx || !r.ref || (r.rel >= 0 && r.rel < 1e-2));
}

inline std::string result_line(const Result& r) {
  char b[512];
  std::snprintf(b, sizeof(b),
                "RESULT {\"test\":\"gemm\",\"gpu\":%d,\"M\":%d,\"N\":%d,\"K\":%d,\"dtype\":\"%s\","
                "\"median_ms\":%.4f,\"min_ms\":%.4f,\"tflops\":%.1f,\"rel_err_vs_rocblas\":%s,"
                "\"spot_block\":[%d,%d],\"max_abs_err\":%s,\"spot_tolerance\":%.4g,",
                r.gpu, r.n, r.n, r.n, r.dtype, r.median_s * 1e3, r.min_ms,
                2.0 * r.n * double(r.n) * r.n / r.median_s / 1e12,
                r.mx ? "null" : json_num(r.rel).c_str(), r.block.r0, r.block.c0,
                json_num(r.max_abs_err).c_str(), spot_tolerance(r.max_ref));
  std::string s = b;
  if (r.mx) {
    std::snprintf(b, sizeof(b), "\"quantize_ms\":%.4f,", r.quantize_ms);
    s += b;
  }
  s += passes(r) ? "\"pass\":true" : "\"pass\":false";
  if (!r.error.empty()) s += ",\"error\":\"" + r.error + "\"";
  return s + "}";
}

// the line of a size whose buffers could not be allocated
inline std::string alloc_failure_line(const Result& r) {
  const std::string dtype = r.mx ? std::string(",\"dtype\":\"") + r.dtype + "\"" : "";
  return "RESULT {\"test\":\"gemm\",\"gpu\":" + std::to_string(r.gpu) + ",\"M\":" + std::to_string(r.n) +
         dtype + ",\"pass\":false,\"error\":\"alloc\"}";
}

}  // namespace gemm_bench
