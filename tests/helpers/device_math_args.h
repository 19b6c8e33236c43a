// Test infrastructure (tests/test_gpu_device_math.py): the ARGUMENTS of the device sweeps as functions of a running index, shared by the
// device kernels (tests/helpers/testkernels.hip) and the host comparison (tests/helpers/device_math_check.cpp), so that a sweep only
// has to bring results back. No arithmetic under test lives here.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DMA_HD __host__ __device__ inline
#else
#define DMA_HD inline
#endif

// sqrt_rn_batch<16> sweep. A wave is 64 lanes x 16 values = 1024 consecutive indices.
//  arrangement 0: every pattern of [2^-96, inf) = 0x0f800000 .. 0x7f7fffff (0x70000000 of them): every wave must take the lean branch
//  arrangement 1: the same, with ONE value of each wave replaced by a value the lean form is not valid for (the class and the place
//                 move with the wave number): every wave must take the library branch
//  arrangement 2: all the other patterns, 0 .. 0x0f7fffff and 0x7f800000 .. 0xffffffff (0x90000000 of them): library branch
#define DMA_SQRT_LEAN_COUNT 0x70000000ull
#define DMA_SQRT_REST_COUNT 0x90000000ull
#define DMA_SQRT_CLASSES 7
DMA_HD uint32_t dma_sqrt_class_bits(uint32_t c, uint32_t salt) {
  switch (c) {
    case 0: return 0x00000000u;                            // +0
    case 1: return 0x80000000u;                            // -0
    case 2: return 1u + (salt * 2654435761u) % 0x007fffffu;   // a subnormal, 0x00000001 .. 0x007fffff
    case 3: return 0x0f000000u;                            // 2^-97
    case 4: return 0x7f800000u;                            // +inf
    case 5: return 0x7fc00000u | (salt & 0xffu);           // NaN
    default: return 0x80800000u + (salt * 2246822519u) % 0x7f000000u;   // a negative normal number
  }
}
DMA_HD uint32_t dma_sqrt_arg(int arrangement, uint64_t i) {
  if (arrangement == 2) return (uint32_t)(i < 0x0f800000ull ? i : i + 0x70000000ull);
  uint32_t bits = 0x0f800000u + (uint32_t)i;
  if (arrangement == 1) {
    const uint64_t wave = i >> 10;
    const uint32_t place = (uint32_t)((wave / DMA_SQRT_CLASSES) & 1023u);       // lane (place >> 4), value (place & 15) of the wave
    if ((uint32_t)(i & 1023u) == place) bits = dma_sqrt_class_bits((uint32_t)(wave % DMA_SQRT_CLASSES), (uint32_t)wave);
  }
  return bits;
}

// counter-based 64-bit mix (splitmix64's finaliser) for the seeded numerators
DMA_HD uint64_t dma_mix64(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
// double numerators: random sign and significand; mode 0: exponent -17 .. 0 (magnitudes 7.6e-6 .. 2, what the kernels divide),
// mode 1: exponent -900 .. 900 (the whole domain div_markstein's comment claims)
DMA_HD uint64_t dma_f64_numerator_bits(uint64_t seed, int mode, uint64_t i) {
  const uint64_t r = dma_mix64(seed ^ (i * 0xd1342543de82ef95ull)), r2 = dma_mix64(r);
  const int64_t e = mode == 0 ? -17 + (int64_t)(r2 % 18u) : -900 + (int64_t)(r2 % 1801u);
  return (r & 0x800fffffffffffffull) | ((uint64_t)(1023 + e) << 52);
}
// float sample of the plain division: every 32-bit pattern class turns up (an odd multiplier walks all of them)
DMA_HD uint32_t dma_f32_sample_bits(uint64_t i) { return (uint32_t)i * 0x9e3779b1u + 0x01234567u; }
