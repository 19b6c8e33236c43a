// config/spectrum/spectrogram.conf (SMILEHIP_CHAIN_SPECTROGRAM): window, transform and cFFTmagphase per frame, the whole chain in one
// launch. It replaces, per frame, cWindower::processVector (windower.cpp:204-218), cTransformFFT::processVector
// (transformFft.cpp:143-195) and cFFTmagphase::processVector (fftmagphase.cpp:215-255).
//
// lld_spectrogram_frame does, per frame: Hamming (or any) window -> forward reference-order transform -> spectrogram::bin_value per
// bin in the plan's form -> the row of K = Nfft / 2 + 1 floats, straight into the caller's matrix. The row is wider than the frame
// (257 floats from 400 int16 samples at 16 kHz): this is the one chain whose stores outweigh its loads. Lane l takes bins l, l + 64, ..,
// so consecutive lanes write consecutive dwords (256 contiguous bytes per store instruction); bin M is the one-lane tail. Rows start
// on 4-byte boundaries whenever K is odd and ld_out = K, so a 16-byte store would need the row staged in LDS first; measured, the launch
// is bound by instruction issue and runs at 22 % of the memory rate, so there is one form of the store.
//
// Two forms, those of lld_audspec_frame (lld_audspec.hip):
//  * wave per frame (Nfft = 512 / 1024: 25 ms frames at 11.025 / 16 kHz and at 22.05 / 32 kHz): the transform is lld_ooura_wave.hpp's
//    register-resident network with M known at compile time, fed from global memory (consecutive lanes take consecutive sample pairs).
//    A frame's LDS is z[M] pairs: 4 KB at M = 512. Four waves per workgroup, persistent: the window and the transform tables are staged
//    once per workgroup, one barrier, none afterwards.
//  * workgroup per frame (any other length: 64 .. 256 points, 2048 .. 8192): ooura_forward on BlockG, the tables in global memory.
// Every global load carries an index clamped into the frame; what lies outside is selected away afterwards. Cell indices are 64-bit:
// 12 500 x 10 s at 16 kHz are 3.2e9 cells. The form is a wave-uniform switch outside the bin loop; the plain-magnitude loop holds no log10f.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "kernel_timing.hpp"
#include "lld_blocks.hpp"
#include "lld_device.hpp"
#include "lld_launch.hpp"
#include "lld_params.hpp"
#include "lld_spectrogram_ops.hpp"

namespace smilehip {

namespace {
constexpr int kSpgWaves = 4;                               // waves (= frames in flight) per workgroup of the wave form
__host__ __device__ constexpr int spg_wave_floats(int M) { return 2 * M; }   // z

// the windowed sample pair i of the frame (pad_left zeros in front with zeroPadSymmetric, zeros behind the frame)
template <class PCM>
__device__ __forceinline__ float2 spg_load_pair(const LldParams &P, const PCM &x, const float *win, int i) {
  const int n0 = 2 * i - P.pad_left, n1 = n0 + 1, last = P.N - 1;
  const int c0 = n0 < 0 ? 0 : (n0 > last ? last : n0), c1 = n1 < 0 ? 0 : (n1 > last ? last : n1);
  const float y0 = x[c0] * win[c0] + P.win_offset, y1 = x[c1] * win[c1] + P.win_offset;
  return make_float2((n0 >= 0 && n0 <= last) ? y0 : 0.0f, (n1 >= 0 && n1 <= last) ? y1 : 0.0f);
}

// the row's cells lane, lane + 64, .. of the wave form, in one form
template <int MC, int FORM>
__device__ __forceinline__ void spg_store_wave(const float2 *z, const OouraTab &oo, const spectrogram::FormConsts &F, float *o, int lane) {
  constexpr int M = MC;
  for (int k = lane; k < M; k += 64) {
    const float2 X = oo_wave_bin<MC>(z, oo, k);
    o[k] = spectrogram::bin_value_form<FORM>(X.x, X.y, k == 0, F);
  }
  if (lane == 0) {                                         // bin M: the one-lane tail
    const float2 X = oo_wave_bin<MC>(z, oo, M);
    o[M] = spectrogram::bin_value_form<FORM>(X.x, X.y, true, F);
  }
}

template <class PCM, int MC>
__device__ __forceinline__ void spg_frame_wave(const LldParams &P, const spectrogram::FormConsts &F, const PCM &pcm, const float *win,
                                               const OouraTab &oo, int64_t row, float *wm) {
  float2 *z = reinterpret_cast<float2 *>(wm);
  const int lane = threadIdx.x & 63;
  const int u = P.frame_utt[row];                          // (wave-uniform)
  const int64_t t = row - P.frame_off[u];
  const PCM x = pcm + (P.samp_off[u] + t * (int64_t)P.H);
  oo_wave_forward<MC>(z, oo, lane, [&](int i) { return spg_load_pair(P, x, win, i); });
  float *o = P.out + row * P.ld_out;                       // (64-bit cell index)
  switch (F.form) {                                        // (wave-uniform)
    case spectrogram::kSpecDens: spg_store_wave<MC, spectrogram::kSpecDens>(z, oo, F, o, lane); break;
    case spectrogram::kPowSpec: spg_store_wave<MC, spectrogram::kPowSpec>(z, oo, F, o, lane); break;
    case spectrogram::kPowSpecDens: spg_store_wave<MC, spectrogram::kPowSpecDens>(z, oo, F, o, lane); break;
    case spectrogram::kDbPsd: spg_store_wave<MC, spectrogram::kDbPsd>(z, oo, F, o, lane); break;
    default: spg_store_wave<MC, spectrogram::kMagnitude>(z, oo, F, o, lane); break;
  }
  WaveG::sync();                                           // (the wave's next frame writes z)
}

template <int FORM>
__device__ __forceinline__ void spg_store_block(const float2 *z, const OouraTab &oo, int M, const spectrogram::FormConsts &F, float *o) {
  for (int k = threadIdx.x; k <= M; k += 256) {
    const float2 X = ooura_bin(z, oo, k);
    o[k] = spectrogram::bin_value_form<FORM>(X.x, X.y, k == 0 || k == M, F);
  }
}
}  // namespace

// one WAVE per frame, persistent workgroups of kSpgWaves waves; LDS: window | transform tables | frame buffers
template <class PCM, int MC>
__global__ void __launch_bounds__(kSpgWaves * 64) lld_spectrogram_frame_wave(LldParams P, spectrogram::FormConsts F, PCM pcm) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Npad = (P.N + 3) & ~3;
  float *s_win = smem;
  for (int i = threadIdx.x; i < P.N; i += kSpgWaves * 64) s_win[i] = P.window[i];
  float *s_oo = smem + Npad;
  const OouraTab oo = oo_stage_tables(P.oo, s_oo, threadIdx.x, kSpgWaves * 64);
  __syncthreads();                                         // the only workgroup barrier
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float *wm = s_oo + oo_table_floats(P.oo) + wave * spg_wave_floats(MC);
  const int64_t stride = (int64_t)gridDim.x * kSpgWaves;
  for (int64_t row = (int64_t)blockIdx.x * kSpgWaves + wave; row < P.total_frames; row += stride)
    spg_frame_wave<PCM, MC>(P, F, pcm, s_win, oo, row, wm);
}

// one WORKGROUP per frame (any transform length the LDS holds); LDS: z[M] pairs; the tables stay in global memory
template <class PCM>
__global__ void __launch_bounds__(256) lld_spectrogram_frame_block(LldParams P, spectrogram::FormConsts F, PCM pcm) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int M = P.Nfft >> 1;
  float2 *z = reinterpret_cast<float2 *>(smem);
  const int64_t row = (int64_t)blockIdx.x;
  const int u = P.frame_utt[row];
  const int64_t t = row - P.frame_off[u];
  const PCM x = pcm + (P.samp_off[u] + t * (int64_t)P.H);
  ooura_forward<BlockG>(z, P.oo, [&](int i) { return spg_load_pair(P, x, P.window, i); });
  float *o = P.out + row * P.ld_out;
  switch (F.form) {
    case spectrogram::kSpecDens: spg_store_block<spectrogram::kSpecDens>(z, P.oo, M, F, o); break;
    case spectrogram::kPowSpec: spg_store_block<spectrogram::kPowSpec>(z, P.oo, M, F, o); break;
    case spectrogram::kPowSpecDens: spg_store_block<spectrogram::kPowSpecDens>(z, P.oo, M, F, o); break;
    case spectrogram::kDbPsd: spg_store_block<spectrogram::kDbPsd>(z, P.oo, M, F, o); break;
    default: spg_store_block<spectrogram::kMagnitude>(z, P.oo, M, F, o); break;
  }
}

namespace {
size_t spg_wave_lds_bytes(const LldParams &P, int M) {
  return sizeof(float) * ((size_t)((P.N + 3) & ~3) + (size_t)oo_table_floats(P.oo) + (size_t)kSpgWaves * spg_wave_floats(M));
}
template <class PCM, int MC>
hipError_t launch_wave(const LldParams &P, const spectrogram::FormConsts &F, const PCM &pcm, hipStream_t s) {
  const size_t bytes = spg_wave_lds_bytes(P, MC);
  if (bytes > 160 * 1024) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&lld_spectrogram_frame_wave<PCM, MC>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)bytes);
  if (e != hipSuccess) return e;
  int64_t grid = (P.total_frames + kSpgWaves - 1) / kSpgWaves;
  const int64_t cap = audspec_wave_grid_cap(current_device_cus(), (int64_t)bytes);
  if (grid > cap) grid = cap;
  SMILEHIP_KLAUNCH((lld_spectrogram_frame_wave<PCM, MC>), dim3((unsigned)grid), dim3(kSpgWaves * 64), bytes, s, P, F, pcm);
  return hipGetLastError();
}
template <class PCM>
hipError_t launch_block(const LldParams &P, const spectrogram::FormConsts &F, const PCM &pcm, hipStream_t s) {
  const size_t bytes = sizeof(float) * (size_t)P.Nfft;     // 2 M floats
  if (bytes > 160 * 1024) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&lld_spectrogram_frame_block<PCM>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)bytes);
  if (e != hipSuccess) return e;
  SMILEHIP_KLAUNCH((lld_spectrogram_frame_block<PCM>), dim3((unsigned)P.total_frames), dim3(256), bytes, s, P, F, pcm);
  return hipGetLastError();
}
template <class PCM>
hipError_t launch_frames(const LldParams &P, const spectrogram::FormConsts &F, const PCM &pcm, hipStream_t s) {
  // SMILEHIP_SPECTROGRAM=block (A/B switch, tools/spectrogram_timing.py): the workgroup form where the wave form would run
  const char *form = getenv("SMILEHIP_SPECTROGRAM");
  const bool block = form && !strcmp(form, "block");
  if (P.Nfft == 1024 && !block) return launch_wave<PCM, 512>(P, F, pcm, s);
  if (P.Nfft == 512 && !block) return launch_wave<PCM, 256>(P, F, pcm, s);
  return launch_block<PCM>(P, F, pcm, s);
}
}  // namespace

hipError_t launch_spectrogram(const LldParams &P, const spectrogram::FormConsts &F, hipStream_t s) {
  if (P.total_frames <= 0) return hipSuccess;
  if (!P.oo.tw || !P.frame_utt || !P.window || !P.out || !(P.pcm || P.pcm_f32)) return hipErrorInvalidValue;
  if (P.Nfft < 64 || P.Nfft > 8192 || P.N < 1 || P.N > P.Nfft || P.K != P.Nfft / 2 + 1 || P.oo.M != P.Nfft / 2 || P.pad_left < 0 ||
      P.pad_left + P.N > P.Nfft || P.total_frames > 0x7fffffffLL)
    return hipErrorInvalidValue;
  if (F.form < spectrogram::kMagnitude || F.form > spectrogram::kDbPsd || P.ld_out < P.K) return hipErrorInvalidValue;
  if (P.pcm_f32) { PcmF32In p; p.f = P.pcm_f32; return launch_frames(P, F, p, s); }
  Pcm16In p; p.s = P.pcm;
  return launch_frames(P, F, p, s);
}

}  // namespace smilehip
