// Development instrumentation of the kernels' phases (-DSMILEHIP_PHASE_TIMING in a private build: tools/ubench/variant*.sh;
// read by tools/ubench/phase_timing*.py): s_memtime at the phase boundaries, summed over all waves by one lane per wave.
// It measures wave RESIDENCE, not issue slots: a phase that waits for memory shows large here and may cost little.
// Without the switch everything here is empty and nothing of it reaches the product.
// The switch has levels: -DSMILEHIP_PHASE_TIMING (= 1) the phase stamps below; -DSMILEHIP_PHASE_TIMING=2 NO phase stamp (they cost
// ~10 % and force waits) and the per-wave lifetime records of wave_lifetimes.hpp instead.
//   SMILEHIP_PHASE_COUNTERS(g_x, 16, smilehip_debug_phase_x)   the counters and their read / reset entry point
//   PhaseTimer<8> PH;  ..  PH(3);  ..  PH.flush(g_x);           per thread: stamp the end of phase 3; add the sums to g_x[0 .. 7]
//   PH.flush(g_x, 8);                                           .. to g_x[8 .. 15], where two kernels share the counters
#pragma once
#include <hip/hip_runtime.h>

namespace smilehip {

#if defined(SMILEHIP_PHASE_TIMING) && SMILEHIP_PHASE_TIMING != 2
#define SMILEHIP_PHASE_COUNTERS(array, len, entry)                                                                   \
  __device__ unsigned long long array[len];                                                                         \
  extern "C" int entry(unsigned long long *out, int reset) {                                                        \
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(array), sizeof(unsigned long long) * (len)) != hipSuccess) return -1; \
    if (reset) {                                                                                                    \
      unsigned long long z[len] = {0};                                                                              \
      if (hipMemcpyToSymbol(HIP_SYMBOL(array), z, sizeof(z)) != hipSuccess) return -1;                              \
    }                                                                                                               \
    return 0;                                                                                                       \
  }
template <int N>
struct PhaseTimer {
  unsigned long long acc[N] = {};
  unsigned long long last = __builtin_amdgcn_s_memtime();
  __device__ __forceinline__ void operator()(int i) {               // the time since the last stamp belongs to phase i
    const unsigned long long t = __builtin_amdgcn_s_memtime();
    acc[i] += t - last;
    last = t;
  }
  __device__ __forceinline__ void count(int i) { acc[i] += 1; }     // slot i as an event counter
  __device__ __forceinline__ void flush(unsigned long long *counters, int first = 0) {
    if ((threadIdx.x & 63) == 0)
      for (int i = 0; i < N; ++i) atomicAdd(&counters[first + i], acc[i]);
  }
};
// a phase boundary that has to wait for the outstanding loads to mean anything
__device__ __forceinline__ void phase_wait_vm() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
#else
#define SMILEHIP_PHASE_COUNTERS(array, len, entry) constexpr unsigned long long *array = nullptr;
template <int N>
struct PhaseTimer {
  __device__ __forceinline__ void operator()(int) {}
  __device__ __forceinline__ void count(int) {}
  __device__ __forceinline__ void flush(unsigned long long *, int = 0) {}
};
__device__ __forceinline__ void phase_wait_vm() {}
#endif

}  // namespace smilehip
