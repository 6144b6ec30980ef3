// gemm_bench_report.h against strings written down from the printf calls the
// header replaced, as a host program for the ASan + UBSan build
// (make test-gemm-bench-report).
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>

#include "gemm_bench_report.h"

namespace {
using gemm_bench::Result;
int n = 0, bad = 0;

void expect(const std::string& got, const std::string& want) {
  ++n;
  if (got == want) return;
  ++bad;
  std::printf("MISMATCH\n  got  %s\n  want %s\n", got.c_str(), want.c_str());
}

void expect(bool ok, const char* what) {
  ++n;
  if (ok) return;
  ++bad;
  std::printf("FAILED %s\n", what);
}

Result line(const char* dtype, int gpu, int size, double median_s, float min_ms, double rel, bool ref,
            gemm_bench::SpotBlock block, float max_abs_err, float max_ref, float quantize_ms,
            const char* error) {
  Result r;
  r.dtype = dtype;
  r.mx = std::string(dtype) != "bf16";
  r.ref = ref;
  r.gpu = gpu;
  r.n = size;
  r.median_s = median_s;
  r.min_ms = min_ms;
  r.rel = rel;
  r.block = block;
  r.max_abs_err = max_abs_err;
  r.max_ref = max_ref;
  r.quantize_ms = quantize_ms;
  r.error = error;
  return r;
}
}  // namespace

int main() {
  const float inf = std::numeric_limits<float>::infinity();
  const double nan = std::nan("");

  // ---- the five result lines ----
  expect(gemm_bench::result_line(line("bf16", 0, 8192, 0.0006871, 0.6794f, 0.0021537, true, {2304, 5120},
                                      0.28125f, 41.25f, 0.f, "")),
         "RESULT {\"test\":\"gemm\",\"gpu\":0,\"M\":8192,\"N\":8192,\"K\":8192,\"dtype\":\"bf16\","
         "\"median_ms\":0.6871,\"min_ms\":0.6794,\"tflops\":1600.2,\"rel_err_vs_rocblas\":0.002154,"
         "\"spot_block\":[2304,5120],\"max_abs_err\":0.2812,\"spot_tolerance\":0.3223,\"pass\":true}");
  expect(gemm_bench::result_line(line("bf16", 3, 1024, 0.0000212, 0.0207f, -1, false, {0, 768}, inf, 9.5f,
                                      0.f, "fp32 spot check failed")),
         "RESULT {\"test\":\"gemm\",\"gpu\":3,\"M\":1024,\"N\":1024,\"K\":1024,\"dtype\":\"bf16\","
         "\"median_ms\":0.0212,\"min_ms\":0.0207,\"tflops\":101.3,\"rel_err_vs_rocblas\":-1,"
         "\"spot_block\":[0,768],\"max_abs_err\":null,\"spot_tolerance\":0.07422,\"pass\":false,"
         "\"error\":\"fp32 spot check failed\"}");
  expect(gemm_bench::result_line(line("bf16", 1, 4096, 0.0001, 0.1f, nan, true, {256, 512}, 0.125f, 32.f,
                                      0.f, "NaN in the output")),
         "RESULT {\"test\":\"gemm\",\"gpu\":1,\"M\":4096,\"N\":4096,\"K\":4096,\"dtype\":\"bf16\","
         "\"median_ms\":0.1000,\"min_ms\":0.1000,\"tflops\":1374.4,\"rel_err_vs_rocblas\":null,"
         "\"spot_block\":[256,512],\"max_abs_err\":0.125,\"spot_tolerance\":0.25,\"pass\":false,"
         "\"error\":\"NaN in the output\"}");
  expect(gemm_bench::result_line(line("mxfp8", 0, 512, 0.0000123, 0.0119f, -1, true, {256, 0}, 0.0625f,
                                      12.75f, 0.0312f, "")),
         "RESULT {\"test\":\"gemm\",\"gpu\":0,\"M\":512,\"N\":512,\"K\":512,\"dtype\":\"mxfp8\","
         "\"median_ms\":0.0123,\"min_ms\":0.0119,\"tflops\":21.8,\"rel_err_vs_rocblas\":null,"
         "\"spot_block\":[256,0],\"max_abs_err\":0.0625,\"spot_tolerance\":0.09961,"
         "\"quantize_ms\":0.0312,\"pass\":true}");
  expect(gemm_bench::result_line(line("mxfp4", 7, 256, 0.0000101, 0.0098f, -1, true, {0, 0},
                                      float(nan), 0.f, 0.0105f, "kernel launch failed: invalid argument")),
         "RESULT {\"test\":\"gemm\",\"gpu\":7,\"M\":256,\"N\":256,\"K\":256,\"dtype\":\"mxfp4\","
         "\"median_ms\":0.0101,\"min_ms\":0.0098,\"tflops\":3.3,\"rel_err_vs_rocblas\":null,"
         "\"spot_block\":[0,0],\"max_abs_err\":null,\"spot_tolerance\":0,\"quantize_ms\":0.0105,"
         "\"pass\":false,\"error\":\"kernel launch failed: invalid argument\"}");

  // ---- the allocation-failure lines: no "dtype" key for bf16 ----
  expect(gemm_bench::alloc_failure_line(line("bf16", 2, 16384, 0, 0, -1, true, {0, 0}, 0, 0, 0, "")),
         "RESULT {\"test\":\"gemm\",\"gpu\":2,\"M\":16384,\"pass\":false,\"error\":\"alloc\"}");
  expect(gemm_bench::alloc_failure_line(line("mxfp8", 0, 8192, 0, 0, -1, true, {0, 0}, 0, 0, 0, "")),
         "RESULT {\"test\":\"gemm\",\"gpu\":0,\"M\":8192,\"dtype\":\"mxfp8\",\"pass\":false,\"error\":\"alloc\"}");
  expect(gemm_bench::alloc_failure_line(line("mxfp4", 5, 4096, 0, 0, -1, false, {0, 0}, 0, 0, 0, "")),
         "RESULT {\"test\":\"gemm\",\"gpu\":5,\"M\":4096,\"dtype\":\"mxfp4\",\"pass\":false,\"error\":\"alloc\"}");

  // ---- the pass rule: rel in {-1, 0.005, 0.02, NaN} x ref x error ----
  const double rels[4] = {-1, 0.005, 0.02, nan};
  const bool bf16_ref[4] = {false, true, false, false};   // judged against rocBLAS
  for (int i = 0; i < 4; ++i)
    for (int err = 0; err < 2; ++err) {
      const char* e = err ? "fp32 spot check failed" : "";
      expect(gemm_bench::passes(line("bf16", 0, 256, 1e-5, 0.01f, rels[i], true, {0, 0}, 0, 1, 0, e)) ==
                 (!err && bf16_ref[i]), "bf16 pass rule, compared with rocBLAS");
      expect(gemm_bench::passes(line("bf16", 0, 256, 1e-5, 0.01f, rels[i], false, {0, 0}, 0, 1, 0, e)) == !err,
             "bf16 pass rule under --no-ref");
      for (int ref = 0; ref < 2; ++ref)
        expect(gemm_bench::passes(line("mxfp8", 0, 256, 1e-5, 0.01f, rels[i], ref, {0, 0}, 0, 1, 0, e)) == !err,
               "MX pass rule");
    }

  // ---- the spot block of (n, dev), its tolerance and its two error texts ----
  const int blocks[7][4] = {{256, 0, 0, 0},        {512, 0, 256, 0},      {1024, 0, 768, 256},
                            {4096, 0, 2816, 0},    {8192, 0, 2816, 7424}, {8192, 7, 6144, 2048},
                            {16384, 3, 11264, 768}};
  for (const auto& b : blocks) {
    const gemm_bench::SpotBlock s = gemm_bench::spot_block(b[0], b[1]);
    expect(s.r0 == b[2] && s.c0 == b[3], "spot block");
  }
  expect(gemm_bench::spot_tolerance(41.25f) == 0.322265625f, "2^-7 max|ref|");
  expect(gemm_bench::spot_error(0.322265625f, 41.25f) == nullptr, "an error at the tolerance passes");
  expect(gemm_bench::spot_error(0.f, 1.f) == nullptr, "an exact block passes");
  expect(gemm_bench::spot_error(0.3224f, 41.25f) == std::string("fp32 spot check failed"), "above it");
  expect(gemm_bench::spot_error(inf, 9.5f) == std::string("fp32 spot check failed"), "inf (a NaN output)");
  expect(gemm_bench::spot_error(0.f, 0.f) == std::string("fp32 spot check: reference block is zero"),
         "zero reference");
  expect(gemm_bench::json_num(inf) == "null" && gemm_bench::json_num(nan) == "null" &&
             gemm_bench::json_num(-1) == "-1" && gemm_bench::json_num(0.0021537) == "0.002154",
         "json_num");

  std::printf("gemm_bench_report: %d checks, %d failed\n", n, bad);
  if (!bad) std::printf("every line equal to the recorded one\n");
  return bad ? 1 : 0;
}
