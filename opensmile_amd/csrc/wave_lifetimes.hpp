// Development record of every wave's lifetime in a persistent kernel (-DSMILEHIP_PHASE_TIMING=2 in a private build --
// level 2 of the instrumentation switch of phase_timing.hpp, which at this level takes no phase stamp:
// tools/ubench/variant.sh; read by tools/ubench/wave_lifetimes.py): s_memtime when a wave enters its pass loop and when it leaves,
// where it ran (the raw HW_ID and XCC_ID registers), which wave of which block it is and how many passes it ran. One record per
// wave, written once by one lane with ordinary vector stores after the loop: nothing is added inside the loop but the scalar
// pass count, no wait is forced (the phase stamps of phase_timing.hpp cost ~10 % and wait for the loads; this does neither).
// s_memtime counters of different CUs need not share a zero: compare lifetimes (end - begin) across the chip and absolute times
// only within a CU. Without the switch everything here is empty and nothing of it reaches the product.
//   SMILEHIP_WAVE_LIFE_RECORDS(g_x, smilehip_debug_wave_life_x)   the records of the last launch and their read / reset entry point
//   WaveLife WL;  WL.begin();  for (..) { .. }  WL.end(g_x, block, wave, passes);
#pragma once
#include <hip/hip_runtime.h>

namespace smilehip {

// a record is six 64-bit words: begin | end | HW_ID + (XCC_ID << 32) | block + (wave << 32) | passes | 1 (written)
constexpr int kWaveLifeWords = 6;
constexpr int kWaveLifeSlots = 8192;     // waves of the resident grid (256 CUs x 2 blocks x 8 waves = 4096) with room to spare

#if defined(SMILEHIP_PHASE_TIMING) && SMILEHIP_PHASE_TIMING == 2
#define SMILEHIP_WAVE_LIFE_RECORDS(array, entry)                                                                      \
  __device__ unsigned long long array[kWaveLifeSlots * kWaveLifeWords];                                              \
  extern "C" int entry(unsigned long long *out, int n_slots, int reset) {                                            \
    if (n_slots < 0 || n_slots > kWaveLifeSlots) return -1;                                                          \
    const size_t bytes = sizeof(unsigned long long) * kWaveLifeWords * (size_t)n_slots;                              \
    if (out && bytes && hipMemcpyFromSymbol(out, HIP_SYMBOL(array), bytes) != hipSuccess) return -1;                 \
    if (reset) {                                                                                                     \
      void *p = nullptr;                                                                                             \
      if (hipGetSymbolAddress(&p, HIP_SYMBOL(array)) != hipSuccess) return -1;                                       \
      if (hipMemset(p, 0, sizeof(unsigned long long) * kWaveLifeWords * kWaveLifeSlots) != hipSuccess) return -1;    \
    }                                                                                                                \
    return kWaveLifeSlots;                                                                                           \
  }
struct WaveLife {
  unsigned long long t0 = 0;
  __device__ __forceinline__ void begin() { t0 = __builtin_amdgcn_s_memtime(); }
  __device__ __forceinline__ void end(unsigned long long *records, unsigned block, unsigned wave, unsigned passes) {
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    const unsigned hw_id = __builtin_amdgcn_s_getreg((31 << 11) | 4);      // HW_REG_HW_ID, all 32 bits
    const unsigned xcc_id = __builtin_amdgcn_s_getreg((31 << 11) | 20);    // HW_REG_XCC_ID
    const unsigned slot = block * (blockDim.x >> 6) + wave;
    if ((threadIdx.x & 63) == 0 && slot < (unsigned)kWaveLifeSlots) {
      unsigned long long *r = records + (size_t)slot * kWaveLifeWords;
      r[0] = t0;
      r[1] = t1;
      r[2] = (unsigned long long)hw_id | ((unsigned long long)xcc_id << 32);
      r[3] = (unsigned long long)block | ((unsigned long long)wave << 32);
      r[4] = passes;
      r[5] = 1ull;
    }
  }
};
#else
#define SMILEHIP_WAVE_LIFE_RECORDS(array, entry) constexpr unsigned long long *array = nullptr;
struct WaveLife {
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void end(unsigned long long *, unsigned, unsigned, unsigned) {}
};
#endif

}  // namespace smilehip
