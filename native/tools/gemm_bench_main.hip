// mx-gemm-bench: standalone CDNA4 bf16 MFMA GEMM validator (BASELINE config 3).
//
// Runs the hand-written kernel (native/kernels/gemm_bf16.hip) on every GPU
// the pod was allocated (one host thread per GPU), on uniform random [-1, 1)
// bf16 operands, checks it against rocBLAS (bf16 in, fp32 compute) and prints
// per GPU and size:
//   RESULT {"test":"gemm","gpu":0,"M":8192,...,"tflops":...,"rel_err":...,"pass":true}
// Protocol: >= warmup_ms of back-to-back launches, then the median of `iters`
// hipEvent-timed launches (BASELINE.md "Measurement protocol").
//   mx-gemm-bench [--sizes 4096,8192,16384] [--iters 50] [--warmup-ms 2000]
//                 [--devices all|0,1] [--no-ref] [--dtype bf16|mxfp8|mxfp4]
// --dtype mxfp8 runs the block-scaled e4m3 path instead
// (native/kernels/gemm_mxfp8.hip): the same bf16 operands are quantised on the
// GPU (32-element blocks, E8M0 scales), the scaled-MFMA kernel is checked on
// the same 256x256 block against an fp32 fmaf chain over the DEQUANTISED
// operands (fp8's own error against the bf16 product is ~7 %, so that product
// is no reference), and timed by the same protocol.  rel_err_vs_rocblas is
// null there: the binary has no library reference for the format.
// --dtype mxfp4 does the same for block-scaled e2m1, two codes per byte
// (native/kernels/gemm_mxfp4.hip); its own error against the bf16 product is
// ~21 % on this data.
//
// The procedure is written once (run_size<D>) over one descriptor per dtype;
// the verdict and the line come from gemm_bench_report.h.  Consumers parse
// stdout, so these stay as they are (make test-gemm-bench-report pins the
// textual ones):
//  - key order and number formats of the RESULT line;
//  - "quantize_ms" sits before "pass", and only for the MX dtypes;
//  - "rel_err_vs_rocblas" is null for MX; for bf16 it is json_num(rel), which
//    prints -1 under --no-ref and null for NaN;
//  - the allocation-failure line has no "dtype" key for bf16; the MX lines
//    have it after "M";
//  - bf16 passes when there is no error and (--no-ref or 0 <= rel < 1e-2),
//    MX when there is no error;
//  - no rocBLAS handle is created for MX; a failing rocblas_gemm_ex prints to
//    stderr and fails the process without changing the line's "pass";
//  - the first error wins: quantiser launch, kernel launch, spot check, then
//    the rocBLAS-norm and NaN messages;
//  - roctx ranges gemm.warmup / gemm.timed, gemm_mxfp8.*, gemm_mxfp4.*;
//  - fill seeds 0x1234 + dev and 0x9876 + dev; the quantiser runs once
//    untimed, then once timed; one stream per device thread;
//  - a HIP call that fails outside those checks is reported on stderr only (CK).
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "gemm_bench_report.h"

extern "C" {
int mxk_gemm_bf16_tn(const void* A, const void* Bt, void* C, int M, int N, int K, int lda, int ldb,
                     int ldc, hipStream_t stream);
// the two MX formats' entry points have one signature each
using MxGemm = int(const void* Aq, const void* As, const void* Bq, const void* Bs, void* C, int M, int N,
                   int K, int lda, int ldsa, int ldb, int ldsb, int ldc, hipStream_t stream);
using MxQuantize = int(const void* x, void* q, void* s, long R, int K, long ldx, long ldq, long lds,
                       hipStream_t stream);
MxGemm mxk_gemm_mxfp8_tn, mxk_gemm_mxfp4_tn;
MxQuantize mxk_quantize_mxfp8, mxk_quantize_mxfp4;
}

namespace {

std::mutex g_print;

#define CK(x)                                                                       \
  do {                                                                              \
    hipError_t e_ = (x);                                                            \
    if (e_ != hipSuccess)                                                           \
      std::fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

__global__ void fill_uniform_bf16(uint16_t* p, size_t n, uint32_t seed) {
  for (size_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
    uint32_t x = static_cast<uint32_t>(i) * 0x9E3779B1u ^ seed;
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    const float u = (x >> 8) * (1.0f / 16777216.0f) * 2.f - 1.f;   // [-1, 1)
    p[i] = static_cast<uint16_t>(__float_as_uint(u) >> 16);
  }
}

__global__ void diff_norms(const uint16_t* c, const uint16_t* r, size_t n, double* out) {
  double d = 0, s = 0;
  for (size_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
    const float a = __uint_as_float(uint32_t(c[i]) << 16), b = __uint_as_float(uint32_t(r[i]) << 16);
    d += double(a - b) * (a - b);
    s += double(b) * b;
  }
  atomicAdd(&out[0], d);
  atomicAdd(&out[1], s);
}

// ---- the binary's own decoders, in plain arithmetic: an independent reference,
// deliberately not the headers the kernels use ----
// e4m3fn byte -> fp32 (finite codes; 0x7f / 0xff, the NaNs, do not occur in a
// quantiser's output) and E8M0 byte -> 2^(byte - 127)
__device__ float e4m3_to_f32(uint8_t b) {
  const int e = (b >> 3) & 15, m = b & 7;
  const float mag = e ? ldexpf(1.f + m * 0.125f, e - 7) : ldexpf(m * 0.125f, -6);
  return b & 0x80 ? -mag : mag;
}
__device__ float e8m0_to_f32(uint8_t b) { return ldexpf(1.f, int(b) - 127); }
// e2m1 nibble (magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6; bit 3 the sign) -> fp32
__device__ float e2m1_nibble_to_f32(uint8_t c) {
  const int e = (c >> 1) & 3, m = c & 1;
  const float mag = e ? ldexpf(1.f + 0.5f * m, e - 1) : 0.5f * m;
  return c & 8 ? -mag : mag;
}

// What the GEMM under test reads: rows of ldq bytes and, for the MX formats,
// rows of n / 32 E8M0 scales.  bf16 has no scales and reads A and B as filled.
struct Operands {
  const uint8_t *a, *as, *b, *bs;
  int ldq;
};

// One descriptor per dtype: name, roctx range prefix, bytes of a row of n
// elements, whether the operands are quantised first (and by what), whether a
// rocBLAS comparison exists, the GEMM launch, and decode(): the dequantised
// fp32 value of element k of a row, for the spot check.
struct Bf16 {
  static constexpr const char* name = "bf16";
  static constexpr const char* range = "gemm";
  static constexpr bool quantised = false, rocblas = true;
  static constexpr int row_bytes(int n) { return 2 * n; }
  static int gemm(const Operands& o, void* C, int n, hipStream_t st) {
    return mxk_gemm_bf16_tn(o.a, o.b, C, n, n, n, n, n, n, st);
  }
  static __device__ float decode(const uint8_t* row, const uint8_t*, int k) {
    return __uint_as_float(uint32_t(reinterpret_cast<const uint16_t*>(row)[k]) << 16);
  }
};

template <MxQuantize* Quantize, MxGemm* Gemm>
struct Mx {
  static constexpr bool quantised = true, rocblas = false;
  static int quantize(const void* x, void* q, void* s, int n, int ldq, hipStream_t st) {
    return Quantize(x, q, s, n, n, n, ldq, n / 32, st);
  }
  static int gemm(const Operands& o, void* C, int n, hipStream_t st) {
    return Gemm(o.a, o.as, o.b, o.bs, C, n, n, n, o.ldq, n / 32, o.ldq, n / 32, n, st);
  }
};

struct Mxfp8 : Mx<mxk_quantize_mxfp8, mxk_gemm_mxfp8_tn> {
  static constexpr const char* name = "mxfp8";
  static constexpr const char* range = "gemm_mxfp8";
  static constexpr int row_bytes(int n) { return n; }
  static __device__ float decode(const uint8_t* row, const uint8_t* s, int k) {
    return e4m3_to_f32(row[k]) * e8m0_to_f32(s[k >> 5]);
  }
};

struct Mxfp4 : Mx<mxk_quantize_mxfp4, mxk_gemm_mxfp4_tn> {
  static constexpr const char* name = "mxfp4";
  static constexpr const char* range = "gemm_mxfp4";
  static constexpr int row_bytes(int n) { return n / 2; }
  // element k in the low (even k) or high (odd k) nibble of byte k / 2
  static __device__ float decode(const uint8_t* row, const uint8_t* s, int k) {
    return e2m1_nibble_to_f32((row[k >> 1] >> (4 * (k & 1))) & 15) * e8m0_to_f32(s[k >> 5]);
  }
};

// fp32 reference of one 256x256 block of C = A * B^T (row-major, K-contiguous
// operands) at (r0, c0): one fmaf chain over the dequantised operands
// (element x block scale, both exact in fp32), k ascending, compared with the
// kernel's bf16 output: max |diff| and max |ref| (atomicMax on the float
// bits: both are non-negative).
template <class D>
__global__ void spot_check(Operands o, const uint16_t* C, int n, int r0, int c0, unsigned* max_err,
                           unsigned* max_ref) {
  const int r = r0 + blockIdx.x, c = c0 + threadIdx.x;
  const uint8_t* a = o.a + size_t(r) * o.ldq;
  const uint8_t* b = o.b + size_t(c) * o.ldq;
  const uint8_t* sa = D::quantised ? o.as + size_t(r) * (n / 32) : nullptr;
  const uint8_t* sb = D::quantised ? o.bs + size_t(c) * (n / 32) : nullptr;
  float acc = 0.f;
  for (int k = 0; k < n; ++k) acc = fmaf(D::decode(a, sa, k), D::decode(b, sb, k), acc);
  const float got = __uint_as_float(uint32_t(C[size_t(r) * n + c]) << 16);
  const float err = fabsf(got - acc);
  atomicMax(max_err, __float_as_uint(err == err ? err : INFINITY));   // NaN -> inf
  atomicMax(max_ref, __float_as_uint(fabsf(acc)));
}

// ---- RAII holders: every exit from a size's iteration frees what it allocated ----
template <class T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) CK(hipFree(p)); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
  operator T*() const { return p; }
};

struct Event {
  hipEvent_t e = nullptr;
  Event() { CK(hipEventCreate(&e)); }
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  ~Event() { CK(hipEventDestroy(e)); }
  operator hipEvent_t() const { return e; }
};

enum class Dtype { bf16, mxfp8, mxfp4 };

struct Opts {
  Dtype dtype = Dtype::bf16;
  std::vector<int> sizes{4096, 8192, 16384};
  int iters = 50;
  int warmup_ms = 2000;
  bool ref = true;
  std::vector<int> devices;
};

void emit(const std::string& line) {
  std::lock_guard<std::mutex> lk(g_print);
  std::printf("%s\n", line.c_str());
  std::fflush(stdout);
}

// Relative Frobenius error of C against rocBLAS (bf16 in, fp32 compute) into
// r.rel; false when rocblas_gemm_ex itself failed.
bool rocblas_compare(rocblas_handle rb, hipStream_t st, const uint16_t* A, const uint16_t* B,
                     const uint16_t* C, int n, double* nrm, gemm_bench::Result& r) {
  const size_t elems = size_t(n) * n;
  bool ok = true;
  DevBuf<uint16_t> R;
  CK(R.alloc(elems * 2));
  const float alpha = 1.f, beta = 0.f;
  // row-major C = A * B^T  ==  column-major C^T = B * A^T  (B^T stored = B row-major)
  const rocblas_status rs = rocblas_gemm_ex(
      rb, rocblas_operation_transpose, rocblas_operation_none, n, n, n, &alpha, B, rocblas_datatype_bf16_r,
      n, A, rocblas_datatype_bf16_r, n, &beta, R, rocblas_datatype_bf16_r, n, R, rocblas_datatype_bf16_r, n,
      rocblas_datatype_f32_r, rocblas_gemm_algo_standard, 0, 0);
  if (rs != rocblas_status_success) {
    std::lock_guard<std::mutex> lk(g_print);
    std::fprintf(stderr, "rocblas_gemm_ex failed: %s\n", rocblas_status_to_string(rs));
    ok = false;
  }
  CK(hipMemsetAsync(nrm, 0, 16, st));
  hipLaunchKernelGGL(diff_norms, dim3(1024), dim3(256), 0, st, C, R.p, elems, nrm);
  double h[2];
  CK(hipMemcpyAsync(h, nrm, 16, hipMemcpyDeviceToHost, st));
  CK(hipStreamSynchronize(st));
  if (!(h[1] > 0.0)) {
    if (r.error.empty()) r.error = "rocBLAS reference norm is 0 (reference did not run)";
    r.rel = -1;
  } else {
    r.rel = std::sqrt(h[0] / h[1]);
    if (!(r.rel == r.rel) && r.error.empty()) r.error = "NaN in the output";
  }
  return ok;
}

// >= warmup_ms of blocks of 10 back-to-back launches (clocks settle under load
// on random data), then `iters` single event-timed launches: median and minimum.
template <class D>
void time_gemm(const Operands& ops, void* C, int n, const Opts& o, hipStream_t st, hipEvent_t e0,
               hipEvent_t e1, gemm_bench::Result& r) {
  const auto timed = [&](int launches) {
    float ms = 0;
    CK(hipEventRecord(e0, st));
    for (int i = 0; i < launches; ++i) D::gemm(ops, C, n, st);
    CK(hipEventRecord(e1, st));
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&ms, e0, e1));
    return ms;
  };
  roctxRangePushA((std::string(D::range) + ".warmup").c_str());
  for (float spent = 0; spent < o.warmup_ms;) spent += timed(10);
  roctxRangePop();
  std::vector<float> t(o.iters);
  roctxRangePushA((std::string(D::range) + ".timed").c_str());
  for (float& ms : t) ms = timed(1);
  roctxRangePop();
  std::sort(t.begin(), t.end());
  r.median_s = t[t.size() / 2] * 1e-3;
  r.min_ms = t[0];
}

// One size on one device: allocate and fill, quantise (MX), poison C, the
// checked launch, the spot check, the rocBLAS comparison (bf16), timing, the
// RESULT line.  False when the size failed.
template <class D>
bool run_size(int dev, int n, const Opts& o, hipStream_t st, rocblas_handle rb) {
  const size_t elems = size_t(n) * n;
  const int ldq = D::row_bytes(n), nb = n / 32;
  gemm_bench::Result r{D::name, D::quantised, o.ref, dev, n};
  r.block = gemm_bench::spot_block(n, dev);
  DevBuf<uint16_t> A, B, C;
  DevBuf<uint8_t> Aq, Bq, As, Bs;
  DevBuf<double> nrm;
  if (A.alloc(elems * 2) || B.alloc(elems * 2) || C.alloc(elems * 2) ||
      (D::quantised && (Aq.alloc(size_t(n) * ldq) || Bq.alloc(size_t(n) * ldq) ||
                        As.alloc(size_t(n) * nb) || Bs.alloc(size_t(n) * nb))) ||
      (D::rocblas && nrm.alloc(16))) {
    emit(gemm_bench::alloc_failure_line(r));
    return false;
  }
  hipLaunchKernelGGL(fill_uniform_bf16, dim3(2048), dim3(256), 0, st, A.p, elems, 0x1234u + dev);
  hipLaunchKernelGGL(fill_uniform_bf16, dim3(2048), dim3(256), 0, st, B.p, elems, 0x9876u + dev);
  const auto fail = [&r](const char* what, hipError_t e) {   // the first error wins
    if (r.error.empty()) r.error = std::string(what) + hipGetErrorString(e);
  };
  Event e0, e1;
  Operands ops{reinterpret_cast<const uint8_t*>(A.p), nullptr, reinterpret_cast<const uint8_t*>(B.p),
               nullptr, ldq};
  if constexpr (D::quantised) {
    ops = Operands{Aq, As, Bq, Bs, ldq};
    // quantise both operands on the GPU (run once untimed, then timed)
    int qst = D::quantize(A, Aq, As, n, ldq, st);
    if (!qst) qst = D::quantize(B, Bq, Bs, n, ldq, st);
    CK(hipEventRecord(e0, st));
    if (!qst) qst = D::quantize(A, Aq, As, n, ldq, st);
    if (!qst) qst = D::quantize(B, Bq, Bs, n, ldq, st);
    CK(hipEventRecord(e1, st));
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&r.quantize_ms, e0, e1));
    if (qst != 0) fail("quantiser launch failed: ", static_cast<hipError_t>(qst));
  }
  // poison C first: a launch that silently did nothing cannot pass
  CK(hipMemsetAsync(C, 0xff, elems * 2, st));
  const char* skip = std::getenv("MXK_GEMM_BENCH_SKIP_KERNEL");   // fault-injection hook
  int launch_st = 0;
  if (!(skip && *skip == '1')) launch_st = D::gemm(ops, C, n, st);
  const hipError_t le = hipGetLastError();
  if (launch_st != 0 || le != hipSuccess)
    fail("kernel launch failed: ", launch_st ? static_cast<hipError_t>(launch_st) : le);
  {  // fp32 spot check of a pseudo-random 256x256 block
    DevBuf<unsigned> dmax;
    unsigned hmax[2] = {0, 0};
    CK(dmax.alloc(8));
    CK(hipMemsetAsync(dmax, 0, 8, st));
    hipLaunchKernelGGL(spot_check<D>, dim3(256), dim3(256), 0, st, ops, C.p, n, r.block.r0, r.block.c0,
                       dmax.p, dmax.p + 1);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(hmax, dmax, 8, hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    std::memcpy(&r.max_abs_err, &hmax[0], 4);
    std::memcpy(&r.max_ref, &hmax[1], 4);
  }
  const char* spot = gemm_bench::spot_error(r.max_abs_err, r.max_ref);
  if (spot && r.error.empty()) r.error = spot;
  bool ok = true;
  if (D::rocblas && o.ref) ok = rocblas_compare(rb, st, A, B, C, n, nrm, r);
  time_gemm<D>(ops, C, n, o, st, e0, e1, r);
  emit(gemm_bench::result_line(r));
  return ok && gemm_bench::passes(r);
}

// One host thread per GPU, one stream per thread; a rocBLAS handle only where
// the dtype has a library reference and --no-ref is not given.
template <class D>
bool run_device(int dev, const Opts& o) {
  bool all_ok = true;
  if (hipSetDevice(dev) != hipSuccess) return false;
  hipStream_t st;
  CK(hipStreamCreate(&st));
  rocblas_handle rb = nullptr;
  if (D::rocblas && o.ref) {
    rocblas_create_handle(&rb);
    rocblas_set_stream(rb, st);
  }
  for (int n : o.sizes) all_ok &= run_size<D>(dev, n, o, st, rb);
  if (rb) rocblas_destroy_handle(rb);
  CK(hipStreamDestroy(st));
  return all_ok;
}

std::vector<int> parse_list(const char* s) {
  std::vector<int> v;
  std::stringstream ss(s);
  std::string x;
  while (std::getline(ss, x, ',')) if (!x.empty()) v.push_back(std::atoi(x.c_str()));
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  Opts o;
  bool all = true;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--sizes") && i + 1 < argc) o.sizes = parse_list(argv[++i]);
    else if (!std::strcmp(argv[i], "--iters") && i + 1 < argc) o.iters = std::max(1, std::atoi(argv[++i]));
    else if (!std::strcmp(argv[i], "--warmup-ms") && i + 1 < argc) o.warmup_ms = std::atoi(argv[++i]);
    else if (!std::strcmp(argv[i], "--no-ref")) o.ref = false;
    else if (!std::strcmp(argv[i], "--dtype") && i + 1 < argc) {
      const char* v = argv[++i];
      if (!std::strcmp(v, "mxfp8")) o.dtype = Dtype::mxfp8;
      else if (!std::strcmp(v, "mxfp4")) o.dtype = Dtype::mxfp4;
      else if (std::strcmp(v, "bf16")) { std::fprintf(stderr, "--dtype must be bf16, mxfp8 or mxfp4\n"); return 2; }
    } else if (!std::strcmp(argv[i], "--devices") && i + 1 < argc) {
      const char* v = argv[++i];
      if (std::strcmp(v, "all")) { o.devices = parse_list(v); all = false; }
    } else { std::fprintf(stderr, "unknown argument %s\n", argv[i]); return 2; }
  }
  for (int n : o.sizes)
    if (n <= 0 || n % 256) { std::fprintf(stderr, "sizes must be positive multiples of 256\n"); return 2; }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
    std::printf("RESULT {\"test\":\"gemm\",\"pass\":false,\"error\":\"no GPU visible\"}\n");
    return 1;
  }
  if (all) for (int d = 0; d < count; ++d) o.devices.push_back(d);
  std::atomic<bool> ok{true};
  std::vector<std::thread> th;
  for (int d : o.devices)
    th.emplace_back([&, d] {
      const auto run = o.dtype == Dtype::bf16 ? run_device<Bf16>
                       : o.dtype == Dtype::mxfp8 ? run_device<Mxfp8> : run_device<Mxfp4>;
      if (!run(d, o)) ok = false;
    });
  for (auto& t : th) t.join();
  return ok ? 0 : 1;
}
