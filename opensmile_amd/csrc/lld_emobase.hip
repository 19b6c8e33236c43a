// config/emobase/emobase.conf, levels lld and lld_de (SMILEHIP_CHAIN_EMOBASE): two framers with one step, one pass over the samples.
//
// lld_emobase_frame handles step t of an utterance -- the 40 ms frame and the 25 ms frame that start at sample t H; the last one or
// two steps of an utterance have only the 25 ms frame (T40 <= T25):
//   40 ms: Hamming window -> forward reference-order transform -> magnitudes -> power -> inverse transform -> |.| = ACF (no / K:
//          acfCepsNormOutput = 0); the old-style cepstrum input (DC and Nyquist as they are, log(mag^2) where positive on the inner
//          bins, acf.cpp:275-286) -> inverse transform -> |.| = cepstrum; group_pitchacf_frame (lld_blocks.hpp): voicing
//          probability and the cut-off pitch candidate into raw3
//   25 ms: cIntensity and cMZcr on the raw frame; pre-emphasis and Hamming window on the way into the forward transform ->
//          magnitudes -> mel bands -> log -> DCT: intensity | loudness | mfcc 1 .. 12 | . | zcr into raw25
// It is is09_frame_body (lld_is09.hip) and acf_frame_wave (lld_prosody_acf.hip) in one pass, with this file's window, normalisation
// and cepstrum input. Two forms:
//  * wave per step (25 / 40 ms transforms of 256 | 128 / 256 / 512 points: 8, 11.025, 16 kHz), persistent workgroups of kEmoWaves
//    waves: the 256- and 512-point transforms are lld_ooura_wave.hpp's register-resident networks, the 40 ms frame goes from global
//    memory straight into the forward network's registers. The two parts of a step share one buffer: z[M40] pairs | mg[M40 + 4] |
//    sp[M40 + 4] | acf[M40] (the cepstrum's lags replace their own input), 10.0 KB at 16 kHz; the 25 ms part (raw frame | z | mg | sp |
//    log mel, 7.3 KB) runs in it afterwards. Both windows, the mel bank, the DCT rows and both transforms' tables are staged once per
//    workgroup (one barrier, none afterwards).
//  * workgroup per step (any other length, 64 .. 8192 points; SMILEHIP_EMOBASE=block forces it): the same body on BlockG.
// cLpc and cLsp are not in it: the autocorrelation in the reference's summation order, Durbin's recursion and the LSP root search
// are one dependent float chain per frame, which one lane of a wave would walk while 63 wait. lld_emobase_lsp runs them a lane
// per 25 ms frame straight from the samples (emobase::lsp_from_frame, order known at compile time: no private array is indexed
// dynamically, no scratch memory). lld_emobase_contour is cPitchACF's causal contour with F0env, a lane per utterance.
// lld_emobase_tail writes the output: a lane per cell of lld | lld_de by the measured row rules (lld_emobase_ops.hpp).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "kernel_timing.hpp"
#include "lld_blocks.hpp"
#include "lld_device.hpp"
#include "lld_emobase_ops.hpp"
#include "lld_launch.hpp"
#include "lld_params.hpp"

namespace smilehip {

namespace {
constexpr int kEmoWaves = 6;                               // waves (= steps in flight) per workgroup of the wave form

// floats of a step's buffer: the 40 ms part (the block form keeps the cepstrum's lags apart) and the 25 ms part, whichever is larger
__host__ __device__ inline int emo_floats40(int M40, bool wave) { return 2 * M40 + 2 * (M40 + 4) + (wave ? M40 : 2 * M40); }
__host__ __device__ inline int emo_floats25(int N25, int M25) { return ((N25 + 3) & ~3) + 2 * M25 + 2 * (M25 + 4) + 32; }
__host__ __device__ inline int emo_step_floats(int N25, int M25, int M40, bool wave) {
  const int a = emo_floats40(M40, wave), b = emo_floats25(N25, M25);
  return ((a > b ? a : b) + 3) & ~3;
}
// floats of the tables the wave form stages: window40 | window25 | mel_coef | mel_rng | dct_rows (the transforms' tables follow)
__host__ __device__ inline int emo_table_floats(int N40, int N25, int K25) { return ((N40 + 3) & ~3) + ((N25 + 3) & ~3) + ((K25 + 3) & ~3) + 128 + 16 * 32; }

struct EmoTbl {
  const float *win40, *win25, *mel_coef;
  const int32_t *mel_rng;
  const float *dct_rows;
  OouraTab oo40, oo25;
};

// the old-style cepstrum's input of one bin (acf.cpp:275-286, usePower = 1)
__device__ __forceinline__ float emo_cep_input(float mag, bool edge) {
  const float p = mag * mag;
  if (edge) return p;
  return (p > 0.0f) ? (float)log((double)p) : 0.0f;
}

// M40C / M25C: the half lengths where they are known at compile time (256 / 512: the register networks); -1 = run-time length,
// the in-place LDS transform (on one wave or on the workgroup)
template <class G, class PCM, int M40C, int M25C>
__device__ __forceinline__ void emo_step(const LldParams &P, const EmobaseParams &E, const EmoTbl &T, const PCM &pcm, int64_t row,
                                         float *wm, double *scr, int *iscr) {
  constexpr bool kWave = std::is_same<G, WaveG>::value;
  const int u = P.frame_utt[row];                          // (uniform over the group)
  const int64_t t = row - P.frame_off[u];
  const int64_t s0 = P.samp_off[u], len = P.samp_off[u + 1] - s0;
  const PCM x = pcm + (s0 + t * (int64_t)P.H);
  const bool has40 = t < emobase::frames_of(len, E.N40, P.H);
  // The lane index is made opaque per part: what depends on the lane alone (addresses, the networks' masks) is invariant over the
  // wave's steps, and the compiler would carry all of it across the persistent loop (lld_is09.hip: is09_quad_body)
  int tid = G::tid();
  asm volatile("" : "+v"(tid));
  // ---------------------------------------------------------------------------------------------------------------- 40 ms
  if (has40) {
    const int M = M40C > 0 ? M40C : (E.Nfft40 >> 1), Kpad = M + 4, last = E.N40 - 1;
    float2 *z = reinterpret_cast<float2 *>(wm);
    float *mg = wm + 2 * M;
    float *sp = mg + Kpad;
    float *acf = sp + Kpad;
    float *cep = kWave ? sp : acf + M;                     // wave form: the cepstrum's lags replace their own input (read by then)
    // the windowed sample pair i (R2 / R3; zeroPadSymmetric = 0: zeros behind the frame): clamped index, the zero selected afterwards
    const auto load_pair = [&](int i) {
      const int n0 = 2 * i, n1 = n0 + 1;
      const int c0 = n0 > last ? last : n0, c1 = n1 > last ? last : n1;
      const float y0 = x[c0] * T.win40[c0] + P.win_offset, y1 = x[c1] * T.win40[c1] + P.win_offset;
      return make_float2(n0 <= last ? y0 : 0.0f, n1 <= last ? y1 : 0.0f);
    };
    if constexpr (kWave) {
      oo_wave_forward<M40C>(z, T.oo40, tid, load_pair);
      for (int k = tid; k <= M; k += 64) {
        const float m = bin_magnitude(oo_wave_bin<M40C>(z, T.oo40, k), k == 0 || k == M);   // R5
        mg[k] = m;
        sp[k] = m * m;                                     // [acf40] usePower = 1 (acf.cpp:252-259)
      }
    } else {
      ooura_forward<G>(z, T.oo40, load_pair);
      for (int k = tid; k <= M; k += G::size()) {
        const float m = bin_magnitude(ooura_bin(z, T.oo40, k), k == 0 || k == M);
        mg[k] = m;
        sp[k] = m * m;
      }
    }
    G::sync();
    // (acfCepsNormOutput = 0: no division; a division by one leaves the bits as they are)
    if constexpr (kWave) oo_wave_irfft_even<M40C>(sp, z, T.oo40, acf, 1.0f, true, tid);
    else oo_irfft_even<G>(sp, z, T.oo40, acf, 1.0f, true);
    for (int k = tid; k <= M; k += G::size()) sp[k] = emo_cep_input(mg[k], k == 0 || k == M);
    G::sync();
    if constexpr (kWave) oo_wave_irfft_even<M40C>(sp, z, T.oo40, cep, 1.0f, true, tid);   // absCepstrum = 1
    else oo_irfft_even<G>(sp, z, T.oo40, cep, 1.0f, true);
    double voicing, Tsamp;
    int max_idx;
    group_pitchacf_frame<G>(acf, cep, M, E.fsSec40, E.maxPitch, scr, iscr, voicing, max_idx, Tsamp);
    if (tid == 0) {
      float *o = E.raw3 + row * 3;
      o[0] = (float)voicing;
      o[1] = prosody_acf::cut_pitch(voicing, prosody_acf::raw_pitch(max_idx, Tsamp), E.voicingCutoff);   // lld_emobase_contour: F0
      o[2] = 0.0f;                                                                                    // ... and F0env
    }
    G::sync();                                             // (the 25 ms part writes these buffers)
  }
  // ---------------------------------------------------------------------------------------------------------------- 25 ms
  {
    asm volatile("" : "+v"(tid));
    const int N = P.N, M = M25C > 0 ? M25C : (P.Nfft >> 1), Npad = (N + 3) & ~3, Kpad = M + 4, last = N - 1;
    float *xr = wm;
    float2 *z = reinterpret_cast<float2 *>(xr + Npad);
    float *mg = reinterpret_cast<float *>(z + M);
    float *sp = mg + Kpad;
    float *lmel = sp + Kpad;
    float *out = E.raw25 + row * E.n25;
    for (int n = tid; n < N; n += G::size()) xr[n] = x[n];   // R0 (or already done: float input)
    G::sync();
    {                                                      // cMZcr zcr (mzcr.cpp:117-124) and cIntensity (intensity.cpp:125-145) on the RAW frame
      int cnt = 0;
      for (int i = 1 + tid; i < N - 1; i += G::size())
        if (((xr[i - 1] * xr[i + 1] <= 0.0f) && (xr[i] == 0.0f)) || (xr[i - 1] * xr[i] < 0.0f)) ++cnt;
      const int total = G::sum_i(cnt, iscr);
      if (tid == 0) {
        out[E.n25 - 1] = (float)total / (float)N;
        emobase::intensity_frame(xr[0], xr[1], E.w0, E.w1, E.win_sum, out);
      }
    }
    // cVectorPreemphasis and cWindower on the way into the transform (R2 / R3), zeros behind the frame
    const auto load_pair = [&](int i) {
      const int n0 = 2 * i, n1 = n0 + 1;
      const int c0 = n0 > last ? last : n0, c1 = n1 > last ? last : n1;
      const float a = xr[c0], b = xr[c1], before = xr[c0 > 0 ? c0 - 1 : 0];
      const float y0 = emobase::preemph_sample(a, before, c0, P.k, P.one_minus_k) * T.win25[c0] + P.win_offset;
      const float y1 = emobase::preemph_sample(b, a, c1, P.k, P.one_minus_k) * T.win25[c1] + P.win_offset;
      return make_float2(n0 <= last ? y0 : 0.0f, n1 <= last ? y1 : 0.0f);
    };
    if constexpr (kWave) {
      oo_wave_forward<M25C>(z, T.oo25, tid, load_pair);
      for (int k = tid; k <= M; k += 64) mg[k] = bin_magnitude(oo_wave_bin<M25C>(z, T.oo25, k), k == 0 || k == M);   // R5
    } else {
      ooura_forward<G>(z, T.oo25, load_pair);
      for (int k = tid; k <= M; k += G::size()) mg[k] = bin_magnitude(ooura_bin(z, T.oo25, k), k == 0 || k == M);
    }
    G::sync();
    // R6 / R7: mel (usePower per config) -> log -> DCT
    for (int k = tid; k <= M; k += G::size()) sp[k] = P.use_power ? mg[k] * mg[k] : mg[k];
    G::sync();
    for (int b = tid; b < P.n_bands; b += G::size())
      lmel[b] = log_mel(mel_band_exact(sp, T.mel_coef, T.mel_rng, b, P.mel_scale), P.melfloor, P.log_floor);
    G::sync();
    for (int r = tid; r < P.n_mfcc; r += G::size()) out[2 + r] = dct_coeff(lmel, T.dct_rows + r * P.n_bands, P.n_bands, P.dct_gain[r]);
    G::sync();                                             // (the group's next step writes these buffers)
  }
}
}  // namespace

// one WAVE per step, persistent workgroups of kEmoWaves waves; LDS: tables | transform tables (40 ms, 25 ms) | kEmoWaves step buffers
template <class PCM, int M40C, int M25C>
__global__ void __launch_bounds__(kEmoWaves * 64) lld_emobase_frame_wave(LldParams P, EmobaseParams E, PCM pcm, int step_floats) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int kT = kEmoWaves * 64;
  const int N40pad = (E.N40 + 3) & ~3, N25pad = (P.N + 3) & ~3, K25pad = (P.K + 3) & ~3;
  float *s_win40 = smem;
  float *s_win25 = s_win40 + N40pad;
  float *s_coef = s_win25 + N25pad;
  int32_t *s_rng = reinterpret_cast<int32_t *>(s_coef + K25pad);
  float *s_dct = reinterpret_cast<float *>(s_rng + 128);
  for (int i = threadIdx.x; i < E.N40; i += kT) s_win40[i] = E.window40[i];
  for (int i = threadIdx.x; i < P.N; i += kT) s_win25[i] = P.window[i];
  for (int i = threadIdx.x; i < P.K; i += kT) s_coef[i] = P.mel_coef[i];
  for (int i = threadIdx.x; i < 4 * P.n_bands; i += kT) s_rng[i] = P.mel_rng[i];
  for (int i = threadIdx.x; i < P.n_mfcc * P.n_bands; i += kT) s_dct[i] = P.dct_rows[i];
  float *tb = smem + emo_table_floats(E.N40, P.N, P.K);
  const OouraTab s_oo40 = oo_stage_tables(E.oo40, tb, threadIdx.x, kT);
  // (11.025 kHz: both transforms have 512 points and one set of tables serves them)
  const bool same = E.oo40.M == P.oo.M;
  const OouraTab s_oo25 = same ? s_oo40 : oo_stage_tables(P.oo, tb + oo_table_floats(E.oo40), threadIdx.x, kT);
  __syncthreads();                                         // the only workgroup barrier
  const EmoTbl T = {s_win40, s_win25, s_coef, s_rng, s_dct, s_oo40, s_oo25};
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float *wm = tb + oo_table_floats(E.oo40) + (same ? 0 : oo_table_floats(P.oo)) + wave * step_floats;
  const int64_t stride = (int64_t)gridDim.x * kEmoWaves;
  for (int64_t row = (int64_t)blockIdx.x * kEmoWaves + wave; row < P.total_frames; row += stride)
    emo_step<WaveG, PCM, M40C, M25C>(P, E, T, pcm, row, wm, nullptr, nullptr);
}

// one WORKGROUP per step (any transform length the LDS holds); LDS: the step buffer | 4 doubles | 8 ints of reduction scratch
template <class PCM>
__global__ void __launch_bounds__(256) lld_emobase_frame_block(LldParams P, EmobaseParams E, PCM pcm, int step_floats) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  double *scr = reinterpret_cast<double *>(smem + step_floats);
  int *iscr = reinterpret_cast<int *>(scr + 4);
  const EmoTbl T = {E.window40, P.window, P.mel_coef, P.mel_rng, P.dct_rows, E.oo40, P.oo};
  emo_step<BlockG, PCM, -1, -1>(P, E, T, pcm, (int64_t)blockIdx.x, smem, scr, iscr);
}

// cVectorPreemphasis -> cLpc (autocorrelation, Durbin) -> cLsp, a lane per 25 ms frame, straight from the samples
template <class PCM, int ORDER>
__global__ void __launch_bounds__(64) lld_emobase_lsp(LldParams P, EmobaseParams E, PCM pcm) {
  const int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= P.total_frames) return;
  const int u = P.frame_utt[row];
  const int64_t t = row - P.frame_off[u];
  const PCM x = pcm + (P.samp_off[u] + t * (int64_t)P.H);
  emobase::lsp_from_frame<ORDER>(x, P.N, P.k, P.one_minus_k, E.raw25 + row * E.n25 + 14, nullptr);
}

// R10, sequential part: cPitchACF's causal contour and F0env in place on the 40 ms scratch, state per utterance; a lane per utterance
__global__ void __launch_bounds__(64) lld_emobase_contour(const int64_t *samp_off, const int64_t *frame_off, int n_utt, int N40, int H, float *raw3) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_utt) return;
  const int64_t T40 = emobase::frames_of(samp_off[u + 1] - samp_off[u], N40, H);
  emobase::contour_env_utterance(raw3 + frame_off[u] * 3, T40);
}

// [lld:cContourSmoother] and [delta1:cDeltaRegression]: a lane per (output row, column); the row's lld cell and its lld_de cell
__global__ void __launch_bounds__(256) lld_emobase_tail(LldParams P, EmobaseParams E) {
  const int D = E.n25 + 3;
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= E.total_rows * D) return;
  const int64_t orow = g / D;
  const int c = (int)(g - orow * D);
  int lo = 0, hi = P.n_utt;                                // the utterance of the row: row_off[lo] <= orow < row_off[lo + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (E.row_off[mid] <= orow) lo = mid; else hi = mid;
  }
  const int64_t f0 = P.frame_off[lo];
  emobase::Levels L;
  L.a25 = E.raw25 + f0 * E.n25;
  L.p3 = E.raw3 + f0 * 3;
  L.T25 = (int32_t)(P.frame_off[lo + 1] - f0);
  L.T40 = (int32_t)emobase::frames_of(P.samp_off[lo + 1] - P.samp_off[lo], E.N40, P.H);
  L.n25 = E.n25;
  L.W = E.W;
  const int n = (int)(orow - E.row_off[lo]);
  float *o = P.out + orow * P.ld_out;
  o[c] = emobase::lld_cell(L, n, c);
  o[D + c] = emobase::lld_de_cell(L, n, c);
}

namespace {
// bytes of LDS a workgroup of the wave form takes
size_t wave_bytes(const LldParams &P, const EmobaseParams &E) {
  const size_t tbl = (size_t)emo_table_floats(E.N40, P.N, P.K) + (size_t)oo_table_floats(E.oo40) + (E.oo40.M == P.oo.M ? 0 : (size_t)oo_table_floats(P.oo));
  return sizeof(float) * (tbl + (size_t)kEmoWaves * (size_t)emo_step_floats(P.N, P.Nfft / 2, E.Nfft40 / 2, true));
}
template <class PCM, int M40C, int M25C>
hipError_t launch_wave(const LldParams &P, const EmobaseParams &E, const PCM &pcm, hipStream_t s) {
  const int step_floats = emo_step_floats(P.N, P.Nfft / 2, E.Nfft40 / 2, true);
  const size_t bytes = wave_bytes(P, E);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&lld_emobase_frame_wave<PCM, M40C, M25C>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return e;
  const int n_cu = current_device_cus();
  int64_t per_cu = (int64_t)(160 * 1024 / bytes);
  if (per_cu > 16 / kEmoWaves) per_cu = 16 / kEmoWaves;    // (four waves per SIMD at most: 128 VGPRs)
  if (per_cu < 1) per_cu = 1;
  int64_t grid = (P.total_frames + kEmoWaves - 1) / kEmoWaves;
  const int64_t cap = (int64_t)(n_cu > 0 ? n_cu : 256) * per_cu;
  if (grid > cap) grid = cap;
  SMILEHIP_KLAUNCH((lld_emobase_frame_wave<PCM, M40C, M25C>), dim3((unsigned)grid), dim3(kEmoWaves * 64), bytes, s, P, E, pcm, step_floats);
  return hipGetLastError();
}
template <class PCM>
hipError_t launch_block(const LldParams &P, const EmobaseParams &E, const PCM &pcm, hipStream_t s) {
  const int step_floats = emo_step_floats(P.N, P.Nfft / 2, E.Nfft40 / 2, false);
  const size_t bytes = sizeof(float) * (size_t)step_floats + 4 * sizeof(double) + 8 * sizeof(int);
  if (bytes > 160 * 1024) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&lld_emobase_frame_block<PCM>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return e;
  SMILEHIP_KLAUNCH((lld_emobase_frame_block<PCM>), dim3((unsigned)P.total_frames), dim3(256), bytes, s, P, E, pcm, step_floats);
  return hipGetLastError();
}
template <class PCM, int ORDER>
hipError_t launch_lsp(const LldParams &P, const EmobaseParams &E, const PCM &pcm, hipStream_t s) {
  SMILEHIP_KLAUNCH((lld_emobase_lsp<PCM, ORDER>), dim3((unsigned)((P.total_frames + 63) / 64)), dim3(64), 0, s, P, E, pcm);
  return hipGetLastError();
}
template <class PCM>
hipError_t launch_all(const LldParams &P, const EmobaseParams &E, const PCM &pcm, hipStream_t s) {
  // SMILEHIP_EMOBASE=block (A/B switch, tools/emobase_timing.py): the workgroup form where the wave form would run
  const char *form = getenv("SMILEHIP_EMOBASE");
  const bool block = (form && !strcmp(form, "block")) || wave_bytes(P, E) > 160 * 1024;
  hipError_t e;
  if (!block && E.Nfft40 == 1024 && P.Nfft == 512) e = launch_wave<PCM, 512, 256>(P, E, pcm, s);        // 16 kHz
  else if (!block && E.Nfft40 == 512 && P.Nfft == 512) e = launch_wave<PCM, 256, 256>(P, E, pcm, s);    // 11.025 kHz
  else if (!block && E.Nfft40 == 512 && P.Nfft == 256) e = launch_wave<PCM, 256, -1>(P, E, pcm, s);     // 8 kHz
  else e = launch_block<PCM>(P, E, pcm, s);
  if (e != hipSuccess) return e;
  switch (E.p) {
    case 2: return launch_lsp<PCM, 2>(P, E, pcm, s);
    case 4: return launch_lsp<PCM, 4>(P, E, pcm, s);
    case 6: return launch_lsp<PCM, 6>(P, E, pcm, s);
    case 8: return launch_lsp<PCM, 8>(P, E, pcm, s);
    case 10: return launch_lsp<PCM, 10>(P, E, pcm, s);
    case 12: return launch_lsp<PCM, 12>(P, E, pcm, s);
    case 14: return launch_lsp<PCM, 14>(P, E, pcm, s);
    case 16: return launch_lsp<PCM, 16>(P, E, pcm, s);
  }
  return hipErrorInvalidValue;
}
}  // namespace

int emobase_wave_steps() { return kEmoWaves; }

hipError_t launch_emobase(const LldParams &P, const EmobaseParams &E, hipStream_t s) {
  if (P.total_frames <= 0) return hipSuccess;
  if (!P.oo.tw || !E.oo40.tw || !P.frame_utt || !P.window || !E.window40 || !E.raw25 || !E.raw3 || !E.row_off || !(P.pcm || P.pcm_f32) ||
      !P.mel_coef || !P.mel_rng || !P.dct_rows || !P.dct_gain)
    return hipErrorInvalidValue;
  if (P.Nfft < 64 || P.Nfft > 8192 || P.N < 2 || P.N > P.Nfft || P.K != P.Nfft / 2 + 1 || P.oo.M != P.Nfft / 2 || P.pad_left != 0 ||
      E.Nfft40 < 64 || E.Nfft40 > 8192 || E.N40 < P.N || E.N40 > E.Nfft40 || E.oo40.M != E.Nfft40 / 2 || P.total_frames > 0x7fffffffLL ||
      P.n_bands < 1 || P.n_bands > 32 || P.n_mfcc != 12 || !P.preemph || P.de || E.n25 != emobase::n25_cols(E.p) || E.W < 1 || E.W > 4 ||
      E.total_rows * (int64_t)(E.n25 + 3) > 0x7fffffffLL * 256 || (E.total_rows > 0 && (!P.out || P.ld_out < 2 * (E.n25 + 3))))
    return hipErrorInvalidValue;
  hipError_t e;
  if (P.pcm_f32) { PcmF32In p; p.f = P.pcm_f32; e = launch_all(P, E, p, s); }
  else { Pcm16In p; p.s = P.pcm; e = launch_all(P, E, p, s); }
  if (e != hipSuccess) return e;
  SMILEHIP_KLAUNCH(lld_emobase_contour, dim3((unsigned)((P.n_utt + 63) / 64)), dim3(64), 0, s, P.samp_off, P.frame_off, P.n_utt, E.N40, P.H, E.raw3);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (E.total_rows <= 0) return hipSuccess;
  const int64_t cells = E.total_rows * (int64_t)(E.n25 + 3);
  SMILEHIP_KLAUNCH(lld_emobase_tail, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, P, E);
  return hipGetLastError();
}

}  // namespace smilehip
