// config/audspec/audspec.conf (SMILEHIP_CHAIN_AUDSPEC) as row functions: the frame's samples behind cVectorPreemphasis and cWindower,
// cMelspec's bands from a power spectrum, cPlp as auditory spectrum. __host__ __device__ like lld_chroma_ops.hpp:
// tests/test_audspec_host.py compiles this header with g++ (tests/helpers/audspec_check.cpp) and holds it to the real binary's levels
// bit for bit without a GPU; lld_audspec.hip calls the very same functions from both forms of the frame kernel.
//
// What the components do per frame, as read in their source and measured against the binary (tests/golden/make_golden_audspec.py):
//  * [audspec_pe:cVectorPreemphasis] (vectorPreemphasis.cpp:88-106): y[0] = (1 - k) x[0] with 1 - k formed in float, y[n] = x[n] - k x[n-1]
//    (de: + k x[n-1]), product and difference each rounded to float.
//  * [audspec_win:cWindower] (windower.cpp:204-218): y[n] * win[n] + offset.
//  * [audspec_melspec:cMelspec] (melspec.cpp:520-570) with usePower: the magnitudes are squared, then per band the bins in ascending
//    order, first the rising slope's p - p w, then the falling slope's p w, into a float accumulator; the sum times the HTK scale.
//  * [audspec_plp:cPlp] with htkcompatible = 1 and doAud alone (plp.cpp:489-510): melfloor forced to 1.0 (:153-163), the band floored
//    there, times the HTK equal-loudness weight at the band's centre, (FLOAT_DMEM)pow((double)v, (double)compression). With doIDFT =
//    doLP = doLpToCeps = 0 the component copies these values out (:584-588) under the name audSpec (:259-266); lpOrder, firstCC,
//    cepLifter and nCeps are read and never used on this path.
//  * [audspec_frame:cFramer] with noPostEOIprocessing = 1 writes (n - N) / H + 1 frames for n >= N samples, none below; the two
//    cDeltaRegression levels and the concatenation hold as many rows: rows_of.
// No operation here may be contracted into a fused multiply-add (the library is built with -ffp-contract=off; the helper too).
#pragma once
#include <cmath>
#include <cstdint>

#include "glibc_float.hpp"

namespace smilehip {
namespace audspec {

constexpr int kMaxBands = 64;        // one lane per band in the wave form; the window chain's widest level

// rows of every level behind the framer for an utterance of n_samples samples (frame N, step H)
GLF_HD int64_t rows_of(int64_t n_samples, int64_t N, int64_t H) { return n_samples >= N ? (n_samples - N) / H + 1 : 0; }

// sample n of the frame behind pre-emphasis and window: s = x[n], sp = x[n - 1] (any value at n = 0), w = win[n]
GLF_HD float frame_sample(float s, float sp, bool first, int preemph, int de, float k, float one_minus_k, float w, float offset) {
  const float a = one_minus_k * s;
  const float kp = k * sp;
  const float b = de ? s + kp : s - kp;
  const float y = preemph ? (first ? a : b) : s;
  return y * w + offset;
}

// one band of cMelspec from the frame's power (or magnitude) spectrum p: rng = rise_lo, rise_hi, fall_lo, fall_hi per band
GLF_HD float mel_band(const float *p, const float *coef, const int32_t *rng, int b, float scale) {
  const int rl = rng[4 * b + 0], rh = rng[4 * b + 1], fl = rng[4 * b + 2], fh = rng[4 * b + 3];
  float acc = 0.0f;
  for (int n = rl; n < rh; ++n) {
    const float a = p[n] * coef[n];
    acc += p[n] - a;
  }
  for (int n = fl; n < fh; ++n) {
    const float a = p[n] * coef[n];
    acc += a;
  }
  return acc * scale;
}

// cPlp::initTables with htkcompatible (plp.cpp:335-357): smileDsp_equalLoudnessWeight_htk at the band centre cMelspec publishes on
// the mel axis (melspec.cpp:408-412) -- the expression the PLP chain's table is built with (smilehip_plan.cpp). Host side only.
inline float eql_htk(float centre_mel) {
  const double hz = 700.0 * (std::exp(double(centre_mel) / 1127.0) - 1.0);
  const double f2 = hz * hz, fs = f2 / (f2 + 1.6e5);
  return (float)(fs * fs * ((f2 + 1.44e6) / (f2 + 9.61e6)));
}

// one band of cPlp's auditory spectrum (plp_aud_band of lld_blocks_compare.hpp, restated for both sides)
GLF_HD float aud_band(float mel, float melfloor, float eql, float compression) {
  float v = mel < melfloor ? melfloor : mel;
  v *= eql;
  return (float)pow((double)v, (double)compression);
}

// a frame of the melspec level from K magnitudes, and a frame of the plp level from that
GLF_HD void mel_row(const float *mag, int K, int use_power, const float *coef, const int32_t *rng, int n_bands, float scale, float *pw, float *dst) {
  for (int k = 0; k < K; ++k) pw[k] = use_power ? mag[k] * mag[k] : mag[k];
  for (int b = 0; b < n_bands; ++b) dst[b] = mel_band(pw, coef, rng, b, scale);
}
GLF_HD void aud_row(const float *mel, const float *eql, int n_bands, float melfloor, float compression, float *dst) {
  for (int b = 0; b < n_bands; ++b) dst[b] = aud_band(mel[b], melfloor, eql[b], compression);
}

}  // namespace audspec
}  // namespace smilehip
