// Test helper library (tests/helpers/libsmilehip_testkernels.so, built by __graft_entry__.build(); NOT part of the product
// library): device entry points tests/test_gpu_fft.py uses to look at building blocks of the kernels in isolation -- the
// table logarithm log_d; further down the sweeps of tests/test_gpu_device_math.py. Links libsmilehip.so for the plan's host tables (make_f0_tables).
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../opensmile_amd/csrc/lld_blocks.hpp"
#include "../../opensmile_amd/csrc/lld_device.hpp"

namespace smilehip {
__global__ void log_check_kernel(const double *x, double *y, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = log_d(x[i]);
}
}  // namespace smilehip
// test entry: log_d (lld_device.hpp) on n host doubles
extern "C" int smilehip_debug_log_d(const double *in, double *out, int n) {
  using namespace smilehip;
  double *d_in = nullptr, *d_out = nullptr;
  int rc = -2;
  if (n > 0 && hipMalloc(&d_in, (size_t)n * 8) == hipSuccess && hipMalloc(&d_out, (size_t)n * 8) == hipSuccess &&
      hipMemcpy(d_in, in, (size_t)n * 8, hipMemcpyHostToDevice) == hipSuccess) {
    hipLaunchKernelGGL(log_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_in, d_out, n);
    if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, d_out, (size_t)n * 8, hipMemcpyDeviceToHost) == hipSuccess) rc = 0;
  }
  (void)hipFree(d_in); (void)hipFree(d_out);
  return rc;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// tests/test_gpu_device_math.py: the arithmetic sequences the bit-exact chains rest on -- glibc_float.hpp's functions, sqrt_rn_batch,
// div_markstein and its guards -- run on the device from the product's own headers, swept over their arguments. Nothing is restated
// here: the kernels below only feed arguments (device_math_args.h) to the product's functions and compare / store what comes back.
// A launch covers at most 2^26 arguments (short kernels); results travel through two page-locked staging slots so that the host's
// comparison of one chunk overlaps the next chunk's launch.
#include "device_math_args.h"
#include "../../opensmile_amd/csrc/tables.hpp"

namespace smilehip {
namespace dm {
constexpr uint32_t kChunk = 1u << 26;
struct Sweep {
  hipStream_t stream = nullptr;
  void *dev[2] = {nullptr, nullptr};
  void *host[2] = {nullptr, nullptr};
  unsigned long long *ctr = nullptr;     // device counters [8]
  size_t slot_bytes = 0;
};
static Sweep g_sw;

__global__ void __launch_bounds__(256) glibc_kernel(int which, uint32_t first, uint32_t n, float *out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float x = __uint_as_float(first + i);
  float r;
  switch (which) {
    case 0: r = glibc_logf(x); break;
    case 1: r = glibc_expf(x); break;
    case 2: r = glibc_log10f(x); break;
    case 3: r = glibc_atanf(x); break;
    default: r = glibc_acosf(x); break;
  }
  out[i] = r;
}
__global__ void __launch_bounds__(256) atan2f_kernel(const float *y, const float *x, float *out, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = glibc_atan2f(y[i], x[i]);
}

// n is a multiple of 4096 (a block: 256 lanes x 16 values); ctr[0] += waves on the lean branch, ctr[1] += waves on the library's
__global__ void __launch_bounds__(256) sqrt_kernel(int arrangement, unsigned long long first, float *out, unsigned long long *ctr) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  float v[16];
#pragma unroll
  for (int m = 0; m < 16; ++m) v[m] = __uint_as_float(dma_sqrt_arg(arrangement, first + 16ull * t + (unsigned)m));
  const bool lean = sqrt_rn_batch_is_lean(v);          // (the product's own wave-uniform test, the one sqrt_rn_batch branches on)
  sqrt_rn_batch(v);
  if ((threadIdx.x & 63) == 0) atomicAdd(&ctr[lean ? 0 : 1], 1ull);
  float4 *o = reinterpret_cast<float4 *>(out + 16ull * t);
#pragma unroll
  for (int m = 0; m < 4; ++m) o[m] = make_float4(v[4 * m], v[4 * m + 1], v[4 * m + 2], v[4 * m + 3]);
}

// The guarded quotient the way the kernels form it: a lane ORs the guard over its values, the wave takes div_markstein when no lane
// objects and the division otherwise. KIND 0: any sign (oo_quad_irfft_even_real, the delta regression), 1: never negative (f0_shs).
template <int KIND, int N>
__device__ __forceinline__ bool guarded_div(float (&v)[N], float b) {
  bool odd = false;
#pragma unroll
  for (int m = 0; m < N; ++m) odd |= (KIND == 0) ? div_needs_division(v[m]) : div_needs_division_nonneg(v[m]);
  const bool fast = (KIND == 0 ? div_divisor_is_safe(b) : true) && div_wave_is_safe(odd);
  if (fast) {
    const float y = 1.0f / b;
#pragma unroll
    for (int m = 0; m < N; ++m) v[m] = div_markstein(v[m], b, y);
  } else {
#pragma unroll
    for (int m = 0; m < N; ++m) v[m] = v[m] / b;
  }
  return fast;
}
__device__ __forceinline__ bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }
__device__ __forceinline__ bool same_bits(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b) || (a != a && b != b); }

// patterns first_bits + [0, n), n a multiple of 4096; ctr[0] += mismatches, ctr[1] += waves on the fast path, ctr[2] = min(bad pattern)
template <int KIND>
__global__ void __launch_bounds__(256) div_f32_sweep_kernel(uint32_t first_bits, float b, unsigned long long *ctr) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  float a[16], v[16];
#pragma unroll
  for (int m = 0; m < 16; ++m) { a[m] = __uint_as_float(first_bits + 16u * t + (unsigned)m); v[m] = a[m]; }
  const bool fast = guarded_div<KIND>(v, b);
  if ((threadIdx.x & 63) == 0 && fast) atomicAdd(&ctr[1], 1ull);
#pragma unroll
  for (int m = 0; m < 16; ++m)
    if (!same_bits(v[m], a[m] / b)) { atomicAdd(&ctr[0], 1ull); atomicMin(&ctr[2], (unsigned long long)__float_as_uint(a[m])); }
}
// n a multiple of 64: one value per lane
template <int KIND>
__global__ void __launch_bounds__(64) div_f32_kernel(const float *a, float b, float *out_helper, float *out_div) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  float v[1] = {a[i]};
  guarded_div<KIND>(v, b);
  out_helper[i] = v[0];
  out_div[i] = a[i] / b;
}
__global__ void __launch_bounds__(256) div_f32_sample_kernel(const float *divs, int ndiv, uint32_t n, float *a, float *b, float *q) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float x = __uint_as_float(dma_f32_sample_bits(i)), d = divs[i % (uint32_t)ndiv];
  a[i] = x; b[i] = d; q[i] = x / d;
}
// numerators dma_f64_numerator_bits(seed, mode, first + [0, n)); y = RN(1 / b) from the caller (a host table), or NaN: formed here
// by the division, as the ComParE frame kernel forms its 1.0 / dn. ctr[0] += mismatches, ctr[2] = min(index of a bad numerator)
__global__ void __launch_bounds__(256) div_f64_sweep_kernel(unsigned long long seed, int mode, unsigned long long first, uint32_t n, double b,
                                                            double y, unsigned long long *ctr) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (y != y) y = 1.0 / b;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const uint32_t i = 4u * t + (unsigned)m;
    if (i >= n) break;
    const double a = __longlong_as_double((long long)dma_f64_numerator_bits(seed, mode, first + i));
    if (!same_bits(div_markstein(a, b, y), a / b)) { atomicAdd(&ctr[0], 1ull); atomicMin(&ctr[2], first + i); }
  }
}
__global__ void __launch_bounds__(256) div_f64_sample_kernel(unsigned long long seed, int mode, const double *divs, int ndiv, uint32_t n,
                                                             double *a, double *b, double *q, double *qm) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const double x = __longlong_as_double((long long)dma_f64_numerator_bits(seed, mode, i)), d = divs[i % (uint32_t)ndiv];
  a[i] = x; b[i] = d; q[i] = x / d; qm[i] = div_markstein(x, d, 1.0 / d);
}

static bool ctr_reset() { return hipMemsetAsync(g_sw.ctr, 0, 2 * 8, g_sw.stream) == hipSuccess &&
                                 hipMemsetAsync(g_sw.ctr + 2, 0xff, 8, g_sw.stream) == hipSuccess; }
static bool ctr_read(unsigned long long out[3]) {
  return hipMemcpyAsync(out, g_sw.ctr, 3 * 8, hipMemcpyDeviceToHost, g_sw.stream) == hipSuccess && hipStreamSynchronize(g_sw.stream) == hipSuccess;
}
}  // namespace dm
}  // namespace smilehip

extern "C" void smilehip_debug_sweep_close() {
  using namespace smilehip::dm;
  for (int s = 0; s < 2; ++s) { if (g_sw.dev[s]) (void)hipFree(g_sw.dev[s]); if (g_sw.host[s]) (void)hipHostFree(g_sw.host[s]); }
  if (g_sw.ctr) (void)hipFree(g_sw.ctr);
  if (g_sw.stream) (void)hipStreamDestroy(g_sw.stream);
  g_sw = Sweep();
}
// two device buffers + two page-locked host slots of slot_bytes each, one stream, the counters
extern "C" int smilehip_debug_sweep_open(size_t slot_bytes) {
  using namespace smilehip::dm;
  smilehip_debug_sweep_close();
  bool ok = slot_bytes > 0 && hipStreamCreate(&g_sw.stream) == hipSuccess && hipMalloc(&g_sw.ctr, 8 * 8) == hipSuccess;
  for (int s = 0; ok && s < 2; ++s)
    ok = hipMalloc(&g_sw.dev[s], slot_bytes) == hipSuccess && hipHostMalloc(&g_sw.host[s], slot_bytes, hipHostMallocDefault) == hipSuccess;
  if (!ok) { smilehip_debug_sweep_close(); return -2; }
  g_sw.slot_bytes = slot_bytes;
  return ctr_reset() && hipStreamSynchronize(g_sw.stream) == hipSuccess ? 0 : -2;
}
extern "C" void *smilehip_debug_sweep_host(int slot) { return (slot == 0 || slot == 1) ? smilehip::dm::g_sw.host[slot] : nullptr; }
extern "C" int smilehip_debug_sweep_wait() { return hipStreamSynchronize(smilehip::dm::g_sw.stream) == hipSuccess ? 0 : -2; }

// which: 0 logf, 1 expf, 2 log10f, 3 atanf, 4 acosf of glibc_float.hpp; f(first), f(first + 1), ... -> slot (asynchronous)
extern "C" int smilehip_debug_glibc_launch(int which, uint32_t first, uint32_t n, int slot) {
  using namespace smilehip::dm;
  if (which < 0 || which > 4 || (slot != 0 && slot != 1) || n < 1 || n > kChunk || (size_t)n * 4 > g_sw.slot_bytes) return -1;
  hipLaunchKernelGGL(glibc_kernel, dim3((n + 255u) / 256u), dim3(256), 0, g_sw.stream, which, first, n, (float *)g_sw.dev[slot]);
  if (hipGetLastError() != hipSuccess) return -2;
  return hipMemcpyAsync(g_sw.host[slot], g_sw.dev[slot], (size_t)n * 4, hipMemcpyDeviceToHost, g_sw.stream) == hipSuccess ? 0 : -2;
}
extern "C" int smilehip_debug_glibc_atan2f(const float *y, const float *x, float *out, int n) {
  using namespace smilehip::dm;
  if (n < 1 || (uint32_t)n > kChunk) return -1;
  float *d[3] = {nullptr, nullptr, nullptr};
  int rc = -2;
  const size_t nb = (size_t)n * 4;
  if (hipMalloc(&d[0], nb) == hipSuccess && hipMalloc(&d[1], nb) == hipSuccess && hipMalloc(&d[2], nb) == hipSuccess &&
      hipMemcpy(d[0], y, nb, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d[1], x, nb, hipMemcpyHostToDevice) == hipSuccess) {
    hipLaunchKernelGGL(atan2f_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d[0], d[1], d[2], n);
    if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(out, d[2], nb, hipMemcpyDeviceToHost) == hipSuccess) rc = 0;
  }
  for (float *p : d) (void)hipFree(p);
  return rc;
}
// sqrt_rn_batch<16> of dma_sqrt_arg(arrangement, first + [0, n)) -> slot (asynchronous); n a multiple of 4096
extern "C" int smilehip_debug_sqrt_launch(int arrangement, unsigned long long first, uint32_t n, int slot) {
  using namespace smilehip::dm;
  const unsigned long long total = arrangement == 2 ? DMA_SQRT_REST_COUNT : DMA_SQRT_LEAN_COUNT;
  if (arrangement < 0 || arrangement > 2 || (slot != 0 && slot != 1) || n < 4096 || n > kChunk || n % 4096u || first % 1024ull ||
      first + n > total || (size_t)n * 4 > g_sw.slot_bytes) return -1;
  hipLaunchKernelGGL(sqrt_kernel, dim3(n / 4096u), dim3(256), 0, g_sw.stream, arrangement, first, (float *)g_sw.dev[slot], g_sw.ctr);
  if (hipGetLastError() != hipSuccess) return -2;
  return hipMemcpyAsync(g_sw.host[slot], g_sw.dev[slot], (size_t)n * 4, hipMemcpyDeviceToHost, g_sw.stream) == hipSuccess ? 0 : -2;
}
// the counters since the last call (waits for the stream): out[0], out[1] = the two sums, out[2] = the minimum (all ones: none)
extern "C" int smilehip_debug_sweep_counters(unsigned long long *out) {
  using namespace smilehip::dm;
  if (!ctr_read(out)) return -2;
  return ctr_reset() && hipStreamSynchronize(g_sw.stream) == hipSuccess ? 0 : -2;
}
// every float of one sign with a normal exponent (0x00800000 .. 0x7f7fffff: 254 x 2^23) divided by b through the guarded helper and
// compared with a / b on the device. res: arguments checked, mismatches, waves that took div_markstein, waves in all, first bad bits
extern "C" int smilehip_debug_div_f32_sweep(int kind, float b, int negative, unsigned long long *res) {
  using namespace smilehip::dm;
  if ((kind != 0 && kind != 1) || !g_sw.ctr) return -1;
  const uint32_t lo = 0x00800000u, hi = 0x7f800000u, sign = negative ? 0x80000000u : 0u;
  unsigned long long checked = 0;
  for (uint32_t f = lo; f < hi;) {
    const uint32_t n = (hi - f < kChunk) ? hi - f : kChunk;             // (multiples of 2^23)
    if (kind == 0) hipLaunchKernelGGL(div_f32_sweep_kernel<0>, dim3(n / 4096u), dim3(256), 0, g_sw.stream, sign | f, b, g_sw.ctr);
    else hipLaunchKernelGGL(div_f32_sweep_kernel<1>, dim3(n / 4096u), dim3(256), 0, g_sw.stream, sign | f, b, g_sw.ctr);
    if (hipGetLastError() != hipSuccess) return -2;
    checked += n;
    f += n;
  }
  unsigned long long c[3];
  if (smilehip_debug_sweep_counters(c) != 0) return -2;
  res[0] = checked; res[1] = c[0]; res[2] = c[1]; res[3] = checked / 1024ull; res[4] = c[2];
  return 0;
}
// n values (a multiple of 64; a wave is 64 consecutive ones, one value per lane): the guarded helper's result and the division's
extern "C" int smilehip_debug_div_f32(int kind, const float *a, int n, float b, float *out_helper, float *out_div) {
  using namespace smilehip::dm;
  if ((kind != 0 && kind != 1) || n < 64 || n % 64 || (uint32_t)n > kChunk) return -1;
  float *d[3] = {nullptr, nullptr, nullptr};
  int rc = -2;
  const size_t nb = (size_t)n * 4;
  if (hipMalloc(&d[0], nb) == hipSuccess && hipMalloc(&d[1], nb) == hipSuccess && hipMalloc(&d[2], nb) == hipSuccess &&
      hipMemcpy(d[0], a, nb, hipMemcpyHostToDevice) == hipSuccess) {
    if (kind == 0) hipLaunchKernelGGL(div_f32_kernel<0>, dim3((unsigned)(n / 64)), dim3(64), 0, 0, d[0], b, d[1], d[2]);
    else hipLaunchKernelGGL(div_f32_kernel<1>, dim3((unsigned)(n / 64)), dim3(64), 0, 0, d[0], b, d[1], d[2]);
    if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(out_helper, d[1], nb, hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(out_div, d[2], nb, hipMemcpyDeviceToHost) == hipSuccess) rc = 0;
  }
  for (float *p : d) (void)hipFree(p);
  return rc;
}
// n <= 2^26 triples (a, b, a / b) of the device's own division: a = dma_f32_sample_bits(i), b = divs[i % ndiv]
extern "C" int smilehip_debug_div_f32_sample(const float *divs, int ndiv, uint32_t n, float *a, float *b, float *q) {
  using namespace smilehip::dm;
  if (ndiv < 1 || n < 1 || n > kChunk) return -1;
  float *d[4] = {nullptr, nullptr, nullptr, nullptr};
  int rc = -2;
  const size_t nb = (size_t)n * 4;
  if (hipMalloc(&d[0], (size_t)ndiv * 4) == hipSuccess && hipMalloc(&d[1], nb) == hipSuccess && hipMalloc(&d[2], nb) == hipSuccess &&
      hipMalloc(&d[3], nb) == hipSuccess && hipMemcpy(d[0], divs, (size_t)ndiv * 4, hipMemcpyHostToDevice) == hipSuccess) {
    hipLaunchKernelGGL(div_f32_sample_kernel, dim3((n + 255u) / 256u), dim3(256), 0, 0, d[0], ndiv, n, d[1], d[2], d[3]);
    if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(a, d[1], nb, hipMemcpyDeviceToHost) == hipSuccess &&
        hipMemcpy(b, d[2], nb, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(q, d[3], nb, hipMemcpyDeviceToHost) == hipSuccess) rc = 0;
  }
  for (float *p : d) (void)hipFree(p);
  return rc;
}
// n_total seeded numerators (launches of 2^26) through div_markstein(a, b, y) against a / b on the device; y NaN: 1.0 / b on the device.
// res: checked, mismatches, index of the first bad numerator
extern "C" int smilehip_debug_div_f64_sweep(unsigned long long seed, int mode, double b, double y, unsigned long long n_total,
                                            unsigned long long *res) {
  using namespace smilehip::dm;
  if ((mode != 0 && mode != 1) || !g_sw.ctr) return -1;
  for (unsigned long long f = 0; f < n_total;) {
    const uint32_t n = (n_total - f < kChunk) ? (uint32_t)(n_total - f) : kChunk;
    hipLaunchKernelGGL(div_f64_sweep_kernel, dim3((n + 1023u) / 1024u), dim3(256), 0, g_sw.stream, seed, mode, f, n, b, y, g_sw.ctr);
    if (hipGetLastError() != hipSuccess) return -2;
    f += n;
  }
  unsigned long long c[3];
  if (smilehip_debug_sweep_counters(c) != 0) return -2;
  res[0] = n_total; res[1] = c[0]; res[2] = c[2];
  return 0;
}
// n <= 2^26 quadruples (a, b, a / b, div_markstein(a, b, 1 / b)) for the host's check of the device's double division
extern "C" int smilehip_debug_div_f64_sample(unsigned long long seed, int mode, const double *divs, int ndiv, uint32_t n, double *a, double *b,
                                             double *q, double *qm) {
  using namespace smilehip::dm;
  if ((mode != 0 && mode != 1) || ndiv < 1 || n < 1 || n > kChunk) return -1;
  double *d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int rc = -2;
  const size_t nb = (size_t)n * 8;
  bool ok = hipMalloc(&d[0], (size_t)ndiv * 8) == hipSuccess && hipMemcpy(d[0], divs, (size_t)ndiv * 8, hipMemcpyHostToDevice) == hipSuccess;
  for (int k = 1; ok && k < 5; ++k) ok = hipMalloc(&d[k], nb) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(div_f64_sample_kernel, dim3((n + 255u) / 256u), dim3(256), 0, 0, seed, mode, d[0], ndiv, n, d[1], d[2], d[3], d[4]);
    double *dst[4] = {a, b, q, qm};
    ok = hipDeviceSynchronize() == hipSuccess;
    for (int k = 0; ok && k < 4; ++k) ok = hipMemcpy(dst[k], d[k + 1], nb, hipMemcpyDeviceToHost) == hipSuccess;
    if (ok) rc = 0;
  }
  for (double *p : d) (void)hipFree(p);
  return rc;
}
// the F0 sweep's per-bin records as the plan builds them (tables.cpp: make_f0_tables): out[K x 8], d1 / RN(1 / d1) / d2 / RN(1 / d2) in 3 .. 6
extern "C" int smilehip_debug_f0_sw_rec(long long K, double fft_frame_size_sec, int n_harmonics, float compression, double min_f, double *out) {
  smilehip::F0Host h;
  const int rc = smilehip::make_f0_tables(K, fft_frame_size_sec, n_harmonics, compression, min_f, h);
  if (rc != 0 || h.sw_rec.size() != (size_t)K * 8) return rc ? rc : -2;
  for (size_t i = 0; i < h.sw_rec.size(); ++i) out[i] = h.sw_rec[i];
  return 0;
}
