// config/prosody/prosodyAcf.conf behind cAcf: what one utterance's frames become on their way to the lld level -- cPitchACF's
// voicing cut-off and causal contour, cIntensity's loudness, cContourSmoother's rows. __host__ __device__ like
// lld_prosody_ops.hpp: tests/test_prosody_acf_host.py compiles this header with g++ (tests/helpers/prosody_acf_check.cpp) and
// holds it against the real binary's levels bit for bit without a GPU; lld_prosody_acf.hip calls the frame functions, and the
// window-chain kernel (lld_kernels.hip: lld_chain_tiled / lld_chain_short, one SMA stage, D = 3) is what sma_row restates.
//
// What the file does, as measured against the binary (tests/golden/make_golden_prosody_acf.py) and read in its source:
//  * [pitch:cPitchACF] writes one frame per input frame: voiceProb = (float)voicing, and F0 = the causal contour
//    (pitchACF.cpp:197-237, lld_pitch_contour.hpp) of the candidate 1 / (maxIdx * Tsamp), set to zero where voicing (a double) is
//    below voicingCutoff (:186-192). Tsamp = fsSec / Nfft with fsSec the level's frameSizeSec as a float (:113-116, :151-153).
//  * [int:cIntensity] sums MIN(N, number of outputs) = 1 term of its Hamming-weighted sum (intensity.cpp:134), on the
//    UNWINDOWED frame: prosody::loudness_frame of lld_prosody_ops.hpp as it stands.
//  * [smo:cContourSmoother] reads `pitch;intens`, both of T frames, and writes rows_of(T, W) = T + W rows (W = smaWin / 2) for
//    T >= 1 frames, none for T = 0: IS09's rule. Row n averages positions n - W .. n + W of each level, summed centre, -1, +1,
//    -2, +2, ... (contourSmoother.cpp:104-111), positions clamped to the level's own frames [0, T - 1] (getMatrix replicates the
//    first and the last frame, dataMemoryLevel.cpp:1687-1712) -- except in its left-padding branch (n - W < 0, :1687-1698), which
//    reads the level's slots as they are: a position beyond the last frame is a slot never written, zero. (That shows for
//    T <= 2 W only.) Row n carries the time stamp of frame min(n, T - 1); the second row of a one-frame utterance carries that
//    of frame 1 (row_time_frame).
#pragma once
#include <cstdint>

#include "lld_pitch_contour.hpp"
#include "lld_prosody_ops.hpp"

namespace smilehip {
namespace prosody_acf {

GLF_HD int64_t rows_of(int64_t T, int W) { return T >= 1 ? T + W : 0; }
// the frame whose time stamp row n of an utterance of T frames carries
GLF_HD int64_t row_time_frame(int64_t T, int64_t n) { return T <= 1 ? n : (n < T - 1 ? n : T - 1); }

// cPitchACF's F0 candidate of a frame as the contour sees it (pitchACF.cpp:186-192): raw = 1 / ((float)maxIdx * (float)Tsamp)
GLF_HD float raw_pitch(int max_idx, double Tsamp) {
  float pitch = 0.0f;
  if (max_idx > 0) pitch = 1.0f / ((float)max_idx * (float)Tsamp);
  return pitch;
}
GLF_HD float cut_pitch(double voicing, float raw, double voicing_cutoff) { return voicing < voicing_cutoff ? 0.0f : raw; }

// the level `pitch`, column F0: the contour over an utterance's T cut-off candidates, in place (state per utterance)
GLF_HD void contour_utterance(float *p, int64_t stride, int64_t T) {
  PitchContour S = {};
  for (int64_t t = 0; t < T; ++t) p[t * stride] = pitch_contour_step(S, p[t * stride]);
}

// pcm_loudness of frame t: cIntensity on the unwindowed frame (lld_prosody_ops.hpp), PCM = the utterance's samples
template <class PCM>
GLF_HD float loudness_frame(const PCM &pcm, int32_t H, double win0, double win_sum, int t) {
  prosody::RowConsts R;
  R.voicing_cutoff = 0.0f; R.W = 0; R.H = H; R.reserved = 0; R.win0 = win0; R.win_sum = win_sum;
  return prosody::loudness_frame(pcm, R, t);
}

// Row n (0 <= n < rows_of(T, W)) of one column of the lld level: lv = the column's T values in the level before the smoother
// (stride floats apart). Every load carries an index inside the utterance, an unwritten slot's zero is selected afterwards.
GLF_HD float sma_row(const float *lv, int64_t stride, int T, int W, int n) {
  const bool left_pad = n - W < 0;
  auto value = [&](int i) {
    const int j = i < 0 ? 0 : (i > T - 1 ? T - 1 : i);
    const float v = lv[(int64_t)j * stride];
    return (left_pad && i > T - 1) ? 0.0f : v;
  };
  float acc = value(n);
  for (int k = 1; k <= W; ++k) {
    acc += value(n - k);
    acc += value(n + k);
  }
  return acc / (float)(2 * W + 1);
}

}  // namespace prosody_acf
}  // namespace smilehip
