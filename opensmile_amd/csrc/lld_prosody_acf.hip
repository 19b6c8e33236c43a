// config/prosody/prosodyAcf.conf (SMILEHIP_CHAIN_PROSODY_ACF): the ACF / cepstrum pitch chain and cIntensity per frame,
// cPitchACF's causal contour per utterance. cContourSmoother follows as one SMA stage of the window-chain kernel (lld_kernels.hip).
//
// lld_acf_pitch_frame does, per frame: gauss window -> forward reference-order transform -> magnitudes -> power -> inverse
// transform -> |.| / K = ACF; log(mag + 1) (or log(mag^2 + 1): ProsodyAcfParams::cep_use_power) -> inverse transform -> / K =
// cepstrum; group_pitchacf_frame (lld_blocks.hpp); the frame's loudness. Three floats per frame go into the batch's scratch:
// voicing probability | cut-off pitch candidate | loudness. It is is09_frame_body (lld_is09.hip) without the raw frame in LDS,
// ZCR, RMS, mel, log and DCT, and with the cepstrum's usePower as a parameter.
//
// Two forms:
//  * wave per frame (Nfft = 512 / 1024: 8, 11.025, 16 kHz): the three transforms are lld_ooura_wave.hpp's register-resident
//    networks with M known at compile time. The windowed samples go from global memory straight into the forward network's
//    registers (consecutive lanes take consecutive sample pairs), so a frame's LDS is z[M] pairs | mg[M + 4] | sp[M + 4] |
//    acf[M]: 10.0 KB at M = 512; the cepstrum's lags replace their own input. Four waves per workgroup, persistent: window and
//    transform tables (about 9 KB at 16 kHz) are staged once per workgroup, one barrier, none afterwards; about 49 KB per
//    workgroup = three workgroups per CU, which is also what the 144 VGPRs of the M = 512 instance allow (three waves per SIMD).
//  * workgroup per frame (any other length, 2048 / 4096 at 22.05 .. 48 kHz): ooura_forward / oo_irfft_even on BlockG.
// Every global load carries an index clamped into the frame; what lies outside is selected away afterwards. The utterance of a
// frame is one load (frame_utt).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "kernel_timing.hpp"
#include "lld_blocks.hpp"
#include "lld_device.hpp"
#include "lld_launch.hpp"
#include "lld_params.hpp"
#include "lld_prosody_acf_ops.hpp"

namespace smilehip {

namespace {
constexpr int kAcfWaves = 4;                               // waves (= frames in flight) per workgroup of the wave form
__host__ __device__ constexpr int acf_wave_floats(int M) { return 2 * M + 2 * (M + 4) + M; }   // z | mg | sp | acf

// the windowed sample pair i of the frame (R2 / R3; pad_left zeros in front with zeroPadSymmetric, N .. Nfft - 1 zeros behind)
template <class PCM>
__device__ __forceinline__ float2 acf_load_pair(const LldParams &P, const PCM &x, const float *win, int i) {
  const int n0 = 2 * i - P.pad_left, n1 = n0 + 1, last = P.N - 1;
  const int c0 = n0 < 0 ? 0 : (n0 > last ? last : n0), c1 = n1 < 0 ? 0 : (n1 > last ? last : n1);
  const float y0 = x[c0] * win[c0] + P.win_offset, y1 = x[c1] * win[c1] + P.win_offset;
  return make_float2((n0 >= 0 && n0 <= last) ? y0 : 0.0f, (n1 >= 0 && n1 <= last) ? y1 : 0.0f);
}

// R9's cepstrum input of one bin (acf.cpp:252-305)
__device__ __forceinline__ float acf_cep_input(float mag, int use_power) {
  const float s = use_power ? mag * mag : mag;
  return (s > 0.0f) ? (float)log_d((double)s + 1.0) : 0.0f;
}

// R10, per-frame part (pitchACF.cpp:137-192) and the three cells of the frame
__device__ __forceinline__ void acf_store(const ProsodyAcfParams &Q, int64_t row, double voicing, int max_idx, double Tsamp, float loud) {
  float *o = Q.raw3 + row * 3;
  o[0] = (float)voicing;
  o[1] = prosody_acf::cut_pitch(voicing, prosody_acf::raw_pitch(max_idx, Tsamp), Q.voicingCutoff);   // smoothed in place by lld_acf_pitch_contour
  o[2] = loud;
}

template <class PCM, int MC>
__device__ __forceinline__ void acf_frame_wave(const LldParams &P, const ProsodyAcfParams &Q, const PCM &pcm, const float *win,
                                               const OouraTab &oo, int64_t row, float *wm) {
  constexpr int M = MC, Kpad = MC + 4;
  float2 *z = reinterpret_cast<float2 *>(wm);
  float *mg = wm + 2 * M;
  float *sp = mg + Kpad;
  float *acf = sp + Kpad;
  float *cep = sp;                                         // the cepstrum's lags replace its own input (read by then)
  const int lane = threadIdx.x & 63;
  const int u = P.frame_utt[row];                          // (wave-uniform)
  const int64_t t = row - P.frame_off[u];
  const PCM utt = pcm + P.samp_off[u];
  const PCM x = utt + t * (int64_t)P.H;
  const float loud = prosody_acf::loudness_frame(utt, P.H, Q.win0, Q.win_sum, (int)t);
  oo_wave_forward<MC>(z, oo, lane, [&](int i) { return acf_load_pair(P, x, win, i); });
  for (int k = lane; k <= M; k += 64) {
    const float m = bin_magnitude(oo_wave_bin<MC>(z, oo, k), k == 0 || k == M);   // R5
    mg[k] = m;
    sp[k] = m * m;                                         // [acf:cAcf] usePower = 1 (acf.cpp:252-259)
  }
  WaveG::sync();
  oo_wave_irfft_even<MC>(sp, z, oo, acf, (float)(M + 1), true, lane);
  for (int k = lane; k <= M; k += 64) sp[k] = acf_cep_input(mg[k], Q.cep_use_power);
  WaveG::sync();
  oo_wave_irfft_even<MC>(sp, z, oo, cep, (float)(M + 1), false, lane);
  double voicing, Tsamp;
  int max_idx;
  group_pitchacf_frame<WaveG>(acf, cep, M, Q.fsSec, Q.maxPitch, nullptr, nullptr, voicing, max_idx, Tsamp);
  if (lane == 0) acf_store(Q, row, voicing, max_idx, Tsamp, loud);
  WaveG::sync();                                           // (the wave's next frame writes these buffers)
}
}  // namespace

// one WAVE per frame, persistent workgroups of kAcfWaves waves; LDS: window | transform tables | kAcfWaves frame buffers
template <class PCM, int MC>
__global__ void __launch_bounds__(kAcfWaves * 64) lld_acf_pitch_frame_wave(LldParams P, ProsodyAcfParams Q, PCM pcm) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Npad = (P.N + 3) & ~3;
  float *s_win = smem;
  for (int i = threadIdx.x; i < P.N; i += kAcfWaves * 64) s_win[i] = P.window[i];
  const OouraTab s_oo = oo_stage_tables(P.oo, smem + Npad, threadIdx.x, kAcfWaves * 64);
  __syncthreads();                                         // the only workgroup barrier
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float *wm = smem + Npad + oo_table_floats(P.oo) + wave * acf_wave_floats(MC);
  const int64_t stride = (int64_t)gridDim.x * kAcfWaves;
  for (int64_t row = (int64_t)blockIdx.x * kAcfWaves + wave; row < P.total_frames; row += stride)
    acf_frame_wave<PCM, MC>(P, Q, pcm, s_win, s_oo, row, wm);
}

// one WORKGROUP per frame (any transform length the LDS holds); LDS: z[M] pairs | mg[Kpad] | sp[Kpad] | acf[M] | cep[M] | scr
template <class PCM>
__global__ void __launch_bounds__(256) lld_acf_pitch_frame_block(LldParams P, ProsodyAcfParams Q, PCM pcm) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int M = P.Nfft >> 1, Kpad = (P.K + 3) & ~3;
  float2 *z = reinterpret_cast<float2 *>(smem);
  float *mg = smem + 2 * M;
  float *sp = mg + Kpad;
  float *acf = sp + Kpad;
  float *cep = acf + M;
  double *scr = reinterpret_cast<double *>(cep + M);
  int *iscr = reinterpret_cast<int *>(scr + 4);
  const int64_t row = (int64_t)blockIdx.x;
  const int u = P.frame_utt[row];
  const int64_t t = row - P.frame_off[u];
  const PCM utt = pcm + P.samp_off[u];
  const PCM x = utt + t * (int64_t)P.H;
  const float loud = prosody_acf::loudness_frame(utt, P.H, Q.win0, Q.win_sum, (int)t);
  ooura_forward<BlockG>(z, P.oo, [&](int i) { return acf_load_pair(P, x, P.window, i); });
  for (int k = threadIdx.x; k <= M; k += 256) {
    const float m = bin_magnitude(ooura_bin(z, P.oo, k), k == 0 || k == M);   // R5
    mg[k] = m;
    sp[k] = m * m;
  }
  __syncthreads();
  oo_irfft_even<BlockG>(sp, z, P.oo, acf, (float)P.K, true);
  for (int k = threadIdx.x; k <= M; k += 256) sp[k] = acf_cep_input(mg[k], Q.cep_use_power);
  __syncthreads();
  oo_irfft_even<BlockG>(sp, z, P.oo, cep, (float)P.K, false);
  double voicing, Tsamp;
  int max_idx;
  group_pitchacf_frame<BlockG>(acf, cep, M, Q.fsSec, Q.maxPitch, scr, iscr, voicing, max_idx, Tsamp);
  if (threadIdx.x == 0) acf_store(Q, row, voicing, max_idx, Tsamp, loud);
}

// R10, sequential part: cPitchACF's causal contour (lld_pitch_contour.hpp) in place on the scratch's pitch column, state per
// utterance. One thread per utterance (lld_pitch_smooth of lld_is09.hip with this scratch's stride).
__global__ void __launch_bounds__(64) lld_acf_pitch_contour(const int64_t *frame_off, int n_utt, float *raw3) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_utt) return;
  const int64_t f0 = frame_off[u];
  prosody_acf::contour_utterance(raw3 + f0 * 3 + 1, 3, frame_off[u + 1] - f0);
}

namespace {
template <class PCM, int MC>
hipError_t launch_wave(const LldParams &P, const ProsodyAcfParams &Q, const PCM &pcm, hipStream_t s) {
  const size_t bytes = sizeof(float) * ((size_t)((P.N + 3) & ~3) + (size_t)oo_table_floats(P.oo) + (size_t)kAcfWaves * acf_wave_floats(MC));
  if (bytes > 160 * 1024) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&lld_acf_pitch_frame_wave<PCM, MC>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return e;
  const int n_cu = current_device_cus();
  int64_t per_cu = (int64_t)(160 * 1024 / bytes);
  if (per_cu > 16 / kAcfWaves) per_cu = 16 / kAcfWaves;    // (four waves per SIMD at most: 128 VGPRs)
  int64_t grid = (P.total_frames + kAcfWaves - 1) / kAcfWaves;
  const int64_t cap = (int64_t)(n_cu > 0 ? n_cu : 256) * per_cu;
  if (grid > cap) grid = cap;
  SMILEHIP_KLAUNCH((lld_acf_pitch_frame_wave<PCM, MC>), dim3((unsigned)grid), dim3(kAcfWaves * 64), bytes, s, P, Q, pcm);
  return hipGetLastError();
}
template <class PCM>
hipError_t launch_block(const LldParams &P, const ProsodyAcfParams &Q, const PCM &pcm, hipStream_t s) {
  const int M = P.Nfft / 2, Kpad = (P.K + 3) & ~3;
  const size_t bytes = sizeof(float) * (size_t)(2 * M + 2 * Kpad + 2 * M) + 4 * sizeof(double) + 8 * sizeof(int);
  if (bytes > 160 * 1024) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&lld_acf_pitch_frame_block<PCM>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return e;
  SMILEHIP_KLAUNCH((lld_acf_pitch_frame_block<PCM>), dim3((unsigned)P.total_frames), dim3(256), bytes, s, P, Q, pcm);
  return hipGetLastError();
}
template <class PCM>
hipError_t launch_frames(const LldParams &P, const ProsodyAcfParams &Q, const PCM &pcm, hipStream_t s) {
  // SMILEHIP_PROSODY_ACF=block (A/B switch, tools/prosody_acf_timing.py): the workgroup form where the wave form would run
  const char *form = getenv("SMILEHIP_PROSODY_ACF");
  const bool block = form && !strcmp(form, "block");
  if (P.Nfft == 1024 && !block) return launch_wave<PCM, 512>(P, Q, pcm, s);
  if (P.Nfft == 512 && !block) return launch_wave<PCM, 256>(P, Q, pcm, s);
  return launch_block<PCM>(P, Q, pcm, s);
}
}  // namespace

int prosody_acf_wave_frames() { return kAcfWaves; }

hipError_t launch_prosody_acf(const LldParams &P, const ProsodyAcfParams &Q, hipStream_t s) {
  if (P.total_frames <= 0) return hipSuccess;
  if (!P.oo.tw || !P.frame_utt || !P.window || !Q.raw3 || !(P.pcm || P.pcm_f32)) return hipErrorInvalidValue;
  if (P.Nfft < 64 || P.Nfft > 8192 || P.N < 1 || P.N > P.Nfft || P.K != P.Nfft / 2 + 1 || P.oo.M != P.Nfft / 2 ||
      P.pad_left < 0 || P.pad_left + P.N > P.Nfft || P.total_frames > 0x7fffffffLL)
    return hipErrorInvalidValue;
  hipError_t e;
  if (P.pcm_f32) { PcmF32In p; p.f = P.pcm_f32; e = launch_frames(P, Q, p, s); }
  else { Pcm16In p; p.s = P.pcm; e = launch_frames(P, Q, p, s); }
  if (e != hipSuccess) return e;
  SMILEHIP_KLAUNCH(lld_acf_pitch_contour, dim3((unsigned)((P.n_utt + 63) / 64)), dim3(64), 0, s, P.frame_off, P.n_utt, Q.raw3);
  return hipGetLastError();
}

}  // namespace smilehip
