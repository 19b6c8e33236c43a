// Test helper (tests/test_gpu_device_math.py): compares what the DEVICE build of the product's headers returned for a chunk of
// arguments (tests/helpers/testkernels.hip) with the real libm / the IEEE square root of the machine running the test, on up to 16
// threads. NaNs compare equal as a class (the two architectures' default NaNs differ). For the first mismatch of a chunk it also
// gives the bits of the HOST build of the header, which tells a device code-generation difference from a libm that is not the one
// the tables were read from.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../opensmile_amd/csrc/glibc_float.hpp"
#include "device_math_args.h"

static inline float u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline uint32_t f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline bool same(uint32_t a, uint32_t b) { return a == b || (u2f(a) != u2f(a) && u2f(b) != u2f(b)); }

static int n_threads() {
  const char *e = getenv("OMP_NUM_THREADS");
  int n = e ? atoi(e) : 0;
  if (n < 1) n = (int)std::thread::hardware_concurrency();
  if (n < 1) n = 1;
  return n > 16 ? 16 : n;
}
extern "C" int device_math_threads() { return n_threads(); }

static float libm_fn(int which, float x) {
  switch (which) {
    case 0: return logf(x);
    case 1: return expf(x);
    case 2: return log10f(x);
    case 3: return atanf(x);
    default: return acosf(x);
  }
}
static float header_fn(int which, float x) {
  switch (which) {
    case 0: return smilehip::glibc_logf(x);
    case 1: return smilehip::glibc_expf(x);
    case 2: return smilehip::glibc_log10f(x);
    case 3: return smilehip::glibc_atanf(x);
    default: return smilehip::glibc_acosf(x);
  }
}

// F(i) -> (argument bits, expected bits); dev[i] = the device's bits. Returns the mismatches; first[0..2] = index, device bits,
// expected bits of the one with the lowest index.
template <class F>
static long long compare(uint64_t n, const uint32_t *dev, uint64_t *first, F expect) {
  const int T = n_threads();
  std::vector<long long> bad(T, 0);
  std::vector<uint64_t> fi(T, ~0ull);
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t)
    th.emplace_back([&, t]() {
      const uint64_t lo = n * t / T, hi = n * (t + 1) / T;
      for (uint64_t i = lo; i < hi; ++i)
        if (!same(dev[i], expect(i))) { if (!bad[t]) fi[t] = i; ++bad[t]; }
    });
  for (auto &x : th) x.join();
  long long total = 0;
  uint64_t f = ~0ull;
  for (int t = 0; t < T; ++t) { total += bad[t]; if (fi[t] < f) f = fi[t]; }
  if (total && first) { first[0] = f; first[1] = dev[f]; first[2] = expect(f); }
  return total;
}

// which: 0 logf, 1 expf, 2 log10f, 3 atanf, 4 acosf; dev[i] = device f(bits first + i). first_bad: argument bits, device bits, libm
// bits, host-header bits.
extern "C" long long device_math_check_libm(int which, uint32_t first, uint64_t n, const uint32_t *dev, uint32_t *first_bad) {
  uint64_t f[3] = {0, 0, 0};
  const long long bad = compare(n, dev, f, [=](uint64_t i) { return f2u(libm_fn(which, u2f(first + (uint32_t)i))); });
  if (bad && first_bad) {
    first_bad[0] = first + (uint32_t)f[0]; first_bad[1] = (uint32_t)f[1]; first_bad[2] = (uint32_t)f[2];
    first_bad[3] = f2u(header_fn(which, u2f(first_bad[0])));
  }
  return bad;
}
// the same comparison against the HOST build of the header (for a machine whose libm is not the one the tables were read from)
extern "C" long long device_math_check_header(int which, uint32_t first, uint64_t n, const uint32_t *dev, uint32_t *first_bad) {
  uint64_t f[3] = {0, 0, 0};
  const long long bad = compare(n, dev, f, [=](uint64_t i) { return f2u(header_fn(which, u2f(first + (uint32_t)i))); });
  if (bad && first_bad) { first_bad[0] = first + (uint32_t)f[0]; first_bad[1] = (uint32_t)f[1]; first_bad[2] = (uint32_t)f[2]; first_bad[3] = (uint32_t)f[2]; }
  return bad;
}
// dev[i] = device sqrt_rn_batch of dma_sqrt_arg(arrangement, first + i), against the host's correctly rounded sqrtf (IEEE 754)
extern "C" long long device_math_check_sqrt(int arrangement, uint64_t first, uint64_t n, const uint32_t *dev, uint32_t *first_bad) {
  uint64_t f[3] = {0, 0, 0};
  const long long bad = compare(n, dev, f, [=](uint64_t i) { return f2u(__builtin_sqrtf(u2f(dma_sqrt_arg(arrangement, first + i)))); });
  if (bad && first_bad) { first_bad[0] = dma_sqrt_arg(arrangement, first + f[0]); first_bad[1] = (uint32_t)f[1]; first_bad[2] = (uint32_t)f[2]; }
  return bad;
}
// how many of the n arguments of an arrangement lie outside [2^-96, inf) (what the test expects the library branch to be caused by)
extern "C" long long device_math_sqrt_odd_waves(int arrangement, uint64_t first, uint64_t n) {
  long long waves = 0;
  for (uint64_t w = 0; w < n / 1024; ++w) {
    bool odd = false;
    for (uint64_t i = 0; i < 1024 && !odd; ++i) { const uint32_t u = dma_sqrt_arg(arrangement, first + 1024 * w + i); odd = !(u >= 0x0f800000u && u < 0x7f800000u); }
    waves += odd;
  }
  return waves;
}

// The pair generator of glibc_float_check.cpp's glibc_atan2f_pairs (same recurrence, same special values, same seed handling),
// resumable: state[0] = generator state (0: seed it), state[1] = pairs produced so far. Fills n pairs; NaN pairs are kept (the
// results then compare as NaNs).
extern "C" void device_math_atan2f_pairs(uint64_t *state, uint64_t seed, uint64_t n, float *ys, float *xs) {
  unsigned long long rs = state[0] ? state[0] : (seed ? seed : 88172645463325252ull);
  auto rnd = [&]() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t)(rs >> 16); };
  const uint32_t sp[] = {0, 0x80000000u, 0x3f800000u, 0xbf800000u, 0x7f800000u, 0xff800000u, 0x00000001u, 0x80000001u, 0x7f7fffffu, 0x00800000u, 0x34000000u};
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t it = state[1] + k;
    uint32_t by = rnd(), bx = rnd();
    if (it % 97 == 0) by = sp[rnd() % 11];
    if (it % 89 == 0) bx = sp[rnd() % 11];
    if (it % 3 == 0) { const uint32_t e = (((by >> 23) & 0xff) + (rnd() % 13) - 6) & 0xff; bx = (bx & 0x807fffffu) | (e << 23); }
    ys[k] = u2f(by); xs[k] = u2f(bx);
  }
  state[0] = rs;
  state[1] += n;
}
// dev[i] = device glibc_atan2f(ys[i], xs[i]) against the real atan2f. first_bad: y bits, x bits, device, libm, host header
extern "C" long long device_math_check_atan2f(uint64_t n, const float *ys, const float *xs, const uint32_t *dev, uint32_t *first_bad) {
  uint64_t f[3] = {0, 0, 0};
  const long long bad = compare(n, dev, f, [=](uint64_t i) { return f2u(atan2f(ys[i], xs[i])); });
  if (bad && first_bad) {
    first_bad[0] = f2u(ys[f[0]]); first_bad[1] = f2u(xs[f[0]]); first_bad[2] = (uint32_t)f[1]; first_bad[3] = (uint32_t)f[2];
    first_bad[4] = f2u(smilehip::glibc_atan2f(ys[f[0]], xs[f[0]]));
  }
  return bad;
}
