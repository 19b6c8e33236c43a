// One output row of config/prosody/prosodyShs.conf's lld level from the cPitchShs rows and the samples of its utterance:
// cPitchSmoother, cIntensity and cContourSmoother as the binary runs them in that file. __host__ __device__ like lld_is10_ops.hpp,
// whose per-frame bodies it calls: tests/test_prosody_shs_host.py compiles this header with g++ and holds it against the real
// binary's level bit for bit without a GPU; lld_prosody.hip calls the same function, one lane per row.
//
// What the file does, as measured against the binary (tests/golden/make_golden_prosody_shs.py) and read in its source:
//  * [smooth:cPitchSmoother] sets postSmoothing = 0 AND postSmoothingMethod = simple; the method string wins
//    (pitchSmoother.cpp:91-99: "simp" sets postSmoothing = 1). So the component runs its one-frame-delay smoother: no output for
//    the first frame (:331), then per call t >= 1 the F0 of frame t - 1 with single-frame spikes and octave jumps removed, and the
//    voicing of frame t - 1 -- except that the first call returns before it stores its voicing (:331-332), so the level's first
//    frame has voicing 0 and F0 0. The level `pitch` holds Tp = T - 1 frames for T frames of input, and frame j carries the time
//    stamp of input frame j + 1.
//  * The smoother's state is short-lived: what call t writes is a function of the (cut-off) pitch of frames t - 2, t - 1, t and
//    the voicing of frame t - 1. ons_flag is set anew by every call unless (last > 0, pitch == 0, flag != 0), and such a call is
//    followed by one with last == 0, which sets it anew; ons_flag_o follows from the call's own (last, pitch) pair, because
//    halving needs last > 0 and pitch > 0, which puts ons_flag to 0. So a replay that starts two calls early from a cleared state
//    gives call t's output exactly (pitch_level_frame below; the host test runs it against the sequential pass over random
//    contours). That is what makes the rows independent of one another.
//  * [smo:cContourSmoother] reads `pitch;intens` and writes Tp + W rows (W = smaWin / 2) if Tp >= 1, none otherwise: the
//    first level decides. Row n averages positions n - W .. n + W of each level, summed centre, -1, +1, -2, +2, ...
//    (contourSmoother.cpp:104-111), positions clamped to the level's own frames [0, len - 1] (getMatrix replicates the first and
//    the last frame, dataMemoryLevel.cpp:1687-1712) -- except in its left-padding branch (n - W < 0, :1687-1698), which reads the
//    level's slots as they are: a position beyond the last frame is a slot never written, zero.
//  * [int:cIntensity] sums MIN(N, number of outputs) = 1 term of its Hamming-weighted sum (intensity.cpp:134).
#pragma once
#include <cstdint>

#include "lld_is10_ops.hpp"

namespace smilehip {
namespace prosody {

struct RowConsts {
  float voicing_cutoff;            // cPitchShs' voicingCutoff as cPitchSmoother reads it from the level's meta data (pitchSmoother.cpp:177)
  int32_t W;                       // cContourSmoother smaWin / 2
  int32_t H;                       // frame step in samples (frame t starts at sample t * H: frameCenterSpecial = left)
  int32_t reserved;
  double win0, win_sum;            // cIntensity: the Hamming window's first value and its sum in index order (intensity.cpp:99-104)
};

GLF_HD int64_t rows_of(int64_t T, int W) { return T >= 2 ? T - 1 + W : 0; }

// Frame j (0 <= j <= T - 2) of the level `pitch`: [F0final, voicingFinalUnclipped], what call j + 1 of cPitchSmoother writes.
// shs: the utterance's cPitchShs rows, 21 values each: nCandidates | F0Cand[6] | candVoicing[6] | ... (six slots per field whatever
// nCandidates is; without octave correction the smoother looks at slot 0 only). Every load carries an index inside the utterance.
GLF_HD void pitch_level_frame(const float *shs, int T, float voicing_cutoff, int j, float (&v)[2]) {
  is10::PitchSmootherOpts o;
  o.n_cand = 1; o.octave_correction = 0; o.post_simple = 1; o.flags = 1 | 8;
  o.voicing_cutoff = voicing_cutoff;
  const int c = j + 1;                                   // the call that writes frame j
  const int s0 = c > 2 ? c - 2 : 0;                      // replay from here: call 0 is the stream's real first call
  is10::PitchSmootherState st;
  is10::pitch_smoother_reset(st);
  if (s0 > 0) st.first_frame = 0;
  v[0] = 0.0f; v[1] = 0.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int call = s0 + i;
    const int t = call < T - 1 ? call : T - 1;
    const float *row = shs + (int64_t)t * 21;
    const float cand[3] = {row[1], row[7], 0.0f};        // F0Cand[0] | candVoicing[0] | candScore[0] (not read)
    float o2[2] = {0.0f, 0.0f};
    is10::pitch_smoother_frame(o, st, cand, 1, o2);
    if (call == c) { v[0] = o2[0]; v[1] = o2[1]; }
  }
}

// pcm_loudness of frame t: cIntensity on the unwindowed frame. PCM: samples of the utterance as floats (operator[])
template <class PCM>
GLF_HD float loudness_frame(const PCM &pcm, const RowConsts &R, int t) {
  const float x0 = pcm[(int64_t)t * R.H];
  const double win[1] = {R.win0};
  float lo[1];
  is10::intensity_frame(&x0, 1, win, R.win_sum, 2, lo);
  return lo[0];
}

// Row n (0 <= n < rows_of(T, W)) of an utterance of T >= 2 frames: F0final_sma | voicingFinalUnclipped_sma | pcm_loudness_sma
template <class PCM>
GLF_HD void row(const RowConsts &R, const float *shs, const PCM &pcm, int T, int n, float (&out)[3]) {
  const int Tp = T - 1, W = R.W;
  const bool left_pad = n - W < 0;
  // position i of both levels as the smoother's block holds it: loads with clamped indices, an unwritten slot's zero selected afterwards
  auto value = [&](int i, float (&v)[3]) {
    const int jp = i < 0 ? 0 : (i > Tp - 1 ? Tp - 1 : i), jl = i < 0 ? 0 : (i > T - 1 ? T - 1 : i);
    float p[2];
    pitch_level_frame(shs, T, R.voicing_cutoff, jp, p);
    const float l = loudness_frame(pcm, R, jl);
    const bool zp = left_pad && i > Tp - 1, zl = left_pad && i > T - 1;
    v[0] = zp ? 0.0f : p[0];
    v[1] = zp ? 0.0f : p[1];
    v[2] = zl ? 0.0f : l;
  };
  float acc[3];
  value(n, acc);
  for (int k = 1; k <= W; ++k) {
    float a[3], b[3];
    value(n - k, a);
    value(n + k, b);
    for (int c = 0; c < 3; ++c) {
      acc[c] += a[c];
      acc[c] += b[c];
    }
  }
  const float div = (float)(2 * W + 1);
  for (int c = 0; c < 3; ++c) out[c] = acc[c] / div;
}

}  // namespace prosody
}  // namespace smilehip
