// config/audspec/audspec.conf (SMILEHIP_CHAIN_AUDSPEC): pre-emphasis, window, transform, power spectrum, cMelspec and cPlp as auditory
// spectrum per frame; the two cDeltaRegression stages follow as the window chain (lld_kernels.hip).
//
// lld_audspec_frame does, per frame: audspec::frame_sample per sample (R2 / R3) -> forward reference-order transform -> magnitudes,
// squared with use_power, into an LDS row -> one mel band per lane / thread in the reference's bin order -> audspec::aud_band with the
// HTK equal-loudness weights -> the band row (P.out: the batch's compact static scratch when deltas follow, the output otherwise).
//
// Two forms, those of lld_chroma_frame (lld_chroma.hip):
//  * wave per frame (Nfft = 512 / 1024: 25 ms frames at 11.025 / 16 kHz and at 22.05 / 32 kHz): the transform is lld_ooura_wave.hpp's
//    register-resident network with M known at compile time, fed from global memory (consecutive lanes take consecutive sample pairs).
//    A frame's LDS is z[M + 4] pairs | pw[M + 4]: 6.2 KB at M = 512; behind the transform z holds the mel terms (mel_terms_fill,
//    lld_device.hpp: a[K] | r[K]). Four waves per workgroup, persistent: window, transform tables, mel coefficients, band ranges and
//    equal-loudness weights are staged once per workgroup, one barrier, none afterwards.
//  * workgroup per frame (any other length: 256 points at 8 kHz, 2048 at 44.1 / 48 kHz, edited frame sizes): ooura_forward on BlockG,
//    one thread per band (audspec::mel_band), the tables in global memory.
// Every global load carries an index clamped into the frame; what lies outside is selected away afterwards.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "kernel_timing.hpp"
#include "lld_audspec_ops.hpp"
#include "lld_blocks.hpp"
#include "lld_device.hpp"
#include "lld_launch.hpp"
#include "lld_params.hpp"

namespace smilehip {

namespace {
constexpr int kAudWaves = 4;                               // waves (= frames in flight) per workgroup of the wave form
__host__ __device__ constexpr int aud_wave_floats(int M) { return 2 * (M + 4) + (M + 4); }   // z (then a | r) | pw
__host__ __device__ inline int aud_table_floats(int K) { return ((K + 3) & ~3) + 4 * audspec::kMaxBands + audspec::kMaxBands; }   // coef | ranges | eql

// the pre-emphasised, windowed sample pair i of the frame (R2 / R3; pad_left zeros in front with zeroPadSymmetric, zeros behind the frame)
template <class PCM>
__device__ __forceinline__ float2 aud_load_pair(const LldParams &P, const PCM &x, const float *win, int i) {
  const int n0 = 2 * i - P.pad_left, n1 = n0 + 1, nm = n0 - 1, last = P.N - 1;
  const int cm = nm < 0 ? 0 : (nm > last ? last : nm), c0 = n0 < 0 ? 0 : (n0 > last ? last : n0), c1 = n1 < 0 ? 0 : (n1 > last ? last : n1);
  const float sm = x[cm], s0 = x[c0], s1 = x[c1];
  const float y0 = audspec::frame_sample(s0, sm, n0 == 0, P.preemph, P.de, P.k, P.one_minus_k, win[c0], P.win_offset);
  const float y1 = audspec::frame_sample(s1, s0, n1 == 0, P.preemph, P.de, P.k, P.one_minus_k, win[c1], P.win_offset);
  return make_float2((n0 >= 0 && n0 <= last) ? y0 : 0.0f, (n1 >= 0 && n1 <= last) ? y1 : 0.0f);
}

template <class PCM, int MC>
__device__ __forceinline__ void aud_frame_wave(const LldParams &P, const PCM &pcm, const float *win, const OouraTab &oo, const float *coef,
                                               const int32_t *rng, const float *eql, int64_t row, float *wm) {
  constexpr int M = MC, K = MC + 1;
  float2 *z = reinterpret_cast<float2 *>(wm);
  float *pw = wm + 2 * (M + 4);
  const int lane = threadIdx.x & 63;
  const int u = P.frame_utt[row];                          // (wave-uniform)
  const int64_t t = row - P.frame_off[u];
  const PCM x = pcm + (P.samp_off[u] + t * (int64_t)P.H);
  oo_wave_forward<MC>(z, oo, lane, [&](int i) { return aud_load_pair(P, x, win, i); });
  for (int k = lane; k <= M; k += 64) {
    const float mag = bin_magnitude(oo_wave_bin<MC>(z, oo, k), k == 0 || k == M);   // R5
    pw[k] = P.use_power ? mag * mag : mag;                 // melspec.cpp:520-527
  }
  WaveG::sync();                                           // (every bin is read: the terms replace z)
  float *mt_a = wm, *mt_r = wm + (M + 4);
  mel_terms_fill<WaveG>(pw, coef, K, mt_a, mt_r);
  WaveG::sync();
  if (lane < P.n_bands) {
    const float mel = mel_band_from_terms(mt_a, mt_r, rng, lane, P.mel_scale);      // R6, the reference's bin order
    P.out[row * P.ld_out + lane] = audspec::aud_band(mel, P.melfloor, eql[lane], P.plp_compression);
  }
  WaveG::sync();                                           // (the wave's next frame writes these buffers)
}
}  // namespace

// one WAVE per frame, persistent workgroups of kAudWaves waves; LDS: window | transform tables | mel coefficients | ranges | eql | frame buffers
template <class PCM, int MC>
__global__ void __launch_bounds__(kAudWaves * 64) lld_audspec_frame_wave(LldParams P, PCM pcm) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Npad = (P.N + 3) & ~3, Kpad = (P.K + 3) & ~3;
  float *s_win = smem;
  for (int i = threadIdx.x; i < P.N; i += kAudWaves * 64) s_win[i] = P.window[i];
  float *s_oo = smem + Npad;
  const OouraTab oo = oo_stage_tables(P.oo, s_oo, threadIdx.x, kAudWaves * 64);
  float *s_coef = s_oo + oo_table_floats(P.oo);
  int32_t *s_rng = reinterpret_cast<int32_t *>(s_coef + Kpad);
  float *s_eql = s_coef + Kpad + 4 * audspec::kMaxBands;
  for (int i = threadIdx.x; i < P.K; i += kAudWaves * 64) s_coef[i] = P.mel_coef[i];
  for (int i = threadIdx.x; i < 4 * P.n_bands; i += kAudWaves * 64) s_rng[i] = P.mel_rng[i];
  for (int i = threadIdx.x; i < P.n_bands; i += kAudWaves * 64) s_eql[i] = P.plp_eql[i];
  __syncthreads();                                         // the only workgroup barrier
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float *wm = s_coef + aud_table_floats(P.K) + wave * aud_wave_floats(MC);
  const int64_t stride = (int64_t)gridDim.x * kAudWaves;
  for (int64_t row = (int64_t)blockIdx.x * kAudWaves + wave; row < P.total_frames; row += stride)
    aud_frame_wave<PCM, MC>(P, pcm, s_win, oo, s_coef, s_rng, s_eql, row, wm);
}

// one WORKGROUP per frame (any transform length the LDS holds); LDS: z[M] pairs | pw[Kpad]; the tables stay in global memory
template <class PCM>
__global__ void __launch_bounds__(256) lld_audspec_frame_block(LldParams P, PCM pcm) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int M = P.Nfft >> 1;
  float2 *z = reinterpret_cast<float2 *>(smem);
  float *pw = smem + 2 * M;
  const int64_t row = (int64_t)blockIdx.x;
  const int u = P.frame_utt[row];
  const int64_t t = row - P.frame_off[u];
  const PCM x = pcm + (P.samp_off[u] + t * (int64_t)P.H);
  ooura_forward<BlockG>(z, P.oo, [&](int i) { return aud_load_pair(P, x, P.window, i); });
  for (int k = threadIdx.x; k <= M; k += 256) {
    const float mag = bin_magnitude(ooura_bin(z, P.oo, k), k == 0 || k == M);       // R5
    pw[k] = P.use_power ? mag * mag : mag;
  }
  __syncthreads();
  const int b = threadIdx.x;
  if (b < P.n_bands) {
    const float mel = audspec::mel_band(pw, P.mel_coef, P.mel_rng, b, P.mel_scale);  // R6
    P.out[row * P.ld_out + b] = audspec::aud_band(mel, P.melfloor, P.plp_eql[b], P.plp_compression);
  }
}

namespace {
size_t aud_wave_lds_bytes(const LldParams &P, int M) {
  return sizeof(float) * ((size_t)((P.N + 3) & ~3) + (size_t)oo_table_floats(P.oo) + (size_t)aud_table_floats(P.K) + (size_t)kAudWaves * aud_wave_floats(M));
}
template <class PCM, int MC>
hipError_t launch_wave(const LldParams &P, const PCM &pcm, hipStream_t s) {
  const size_t bytes = aud_wave_lds_bytes(P, MC);
  if (bytes > 160 * 1024) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&lld_audspec_frame_wave<PCM, MC>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)bytes);
  if (e != hipSuccess) return e;
  int64_t grid = (P.total_frames + kAudWaves - 1) / kAudWaves;
  const int64_t cap = audspec_wave_grid_cap(current_device_cus(), (int64_t)bytes);
  if (grid > cap) grid = cap;
  SMILEHIP_KLAUNCH((lld_audspec_frame_wave<PCM, MC>), dim3((unsigned)grid), dim3(kAudWaves * 64), bytes, s, P, pcm);
  return hipGetLastError();
}
template <class PCM>
hipError_t launch_block(const LldParams &P, const PCM &pcm, hipStream_t s) {
  const int M = P.Nfft / 2, Kpad = (P.K + 3) & ~3;
  const size_t bytes = sizeof(float) * (size_t)(2 * M + Kpad);
  if (bytes > 160 * 1024) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&lld_audspec_frame_block<PCM>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)bytes);
  if (e != hipSuccess) return e;
  SMILEHIP_KLAUNCH((lld_audspec_frame_block<PCM>), dim3((unsigned)P.total_frames), dim3(256), bytes, s, P, pcm);
  return hipGetLastError();
}
template <class PCM>
hipError_t launch_frames(const LldParams &P, const PCM &pcm, hipStream_t s) {
  // SMILEHIP_AUDSPEC=block (A/B switch, tools/audspec_timing.py): the workgroup form where the wave form would run
  const char *form = getenv("SMILEHIP_AUDSPEC");
  const bool block = form && !strcmp(form, "block");
  if (P.Nfft == 1024 && !block) return launch_wave<PCM, 512>(P, pcm, s);
  if (P.Nfft == 512 && !block) return launch_wave<PCM, 256>(P, pcm, s);
  return launch_block<PCM>(P, pcm, s);
}
}  // namespace

// persistent workgroups: as many as the LDS admits per CU, four waves per SIMD at most
int64_t audspec_wave_grid_cap(int n_cu, int64_t lds_bytes) {
  int64_t per_cu = lds_bytes > 0 ? (int64_t)(160 * 1024) / lds_bytes : 1;
  if (per_cu > 16 / kAudWaves) per_cu = 16 / kAudWaves;
  if (per_cu < 1) per_cu = 1;
  return (int64_t)(n_cu > 0 ? n_cu : 256) * per_cu;
}
int audspec_wave_frames() { return kAudWaves; }

hipError_t launch_audspec(const LldParams &P, hipStream_t s) {
  if (P.total_frames <= 0) return hipSuccess;
  if (!P.oo.tw || !P.frame_utt || !P.window || !P.out || !P.mel_coef || !P.mel_rng || !P.plp_eql || !(P.pcm || P.pcm_f32)) return hipErrorInvalidValue;
  if (P.Nfft < 64 || P.Nfft > 8192 || P.N < 1 || P.N > P.Nfft || P.K != P.Nfft / 2 + 1 || P.oo.M != P.Nfft / 2 || P.pad_left < 0 ||
      P.pad_left + P.N > P.Nfft || P.total_frames > 0x7fffffffLL)
    return hipErrorInvalidValue;
  if (P.n_bands < 1 || P.n_bands > audspec::kMaxBands || P.ld_out < P.n_bands) return hipErrorInvalidValue;
  if (P.pcm_f32) { PcmF32In p; p.f = P.pcm_f32; return launch_frames(P, p, s); }
  Pcm16In p; p.s = P.pcm;
  return launch_frames(P, p, s);
}

}  // namespace smilehip
