// Host build of opensmile_amd/csrc/lld_prosody_acf_ops.hpp (tests/test_prosody_acf_host.py): what the prosodyAcf chain does behind
// cAcf, over one utterance -- the voicing cut-off and cPitchACF's contour (the frame kernel's last step and lld_acf_pitch_contour),
// cIntensity's loudness (the frame kernel), and cContourSmoother's rows (what the window-chain kernel computes, restated by sma_row).
#include <cstdint>

#include "../../opensmile_amd/csrc/lld_prosody_acf_ops.hpp"

using namespace smilehip;

namespace {
struct Pcm16Host {                                        // smilePcm_convertSamples, 16-bit (smileUtil.c:2527-2535)
  const int16_t *s;
  float operator[](int64_t n) const { return (float)s[n] / 32767.0f; }
};
struct PcmF32Host {
  const float *f;
  float operator[](int64_t n) const { return f[n]; }
};
}  // namespace

extern "C" int64_t prosody_acf_rows_of(int64_t T, int W) { return prosody_acf::rows_of(T, W); }
extern "C" int64_t prosody_acf_row_time_frame(int64_t T, int64_t n) { return prosody_acf::row_time_frame(T, n); }

// voice_prob, f0raw: T values each (the binary's voiceProb column and the F0raw column of a second cPitchACF instance); exactly one
// of pcm16 / pcm_f32; level: T x 3 = voiceProb | F0 | pcm_loudness (the levels pitch and intens)
extern "C" void prosody_acf_levels(const float *voice_prob, const float *f0raw, int64_t T, const int16_t *pcm16, const float *pcm_f32,
                                   double voicing_cutoff, int H, double win0, double win_sum, float *level) {
  if (voicing_cutoff > 1.0) voicing_cutoff = 1.0;         // pitchACF.cpp:96-98
  if (voicing_cutoff < 0.0) voicing_cutoff = 0.0;
  for (int64_t t = 0; t < T; ++t) {
    level[t * 3] = voice_prob[t];
    level[t * 3 + 1] = prosody_acf::cut_pitch((double)voice_prob[t], f0raw[t], voicing_cutoff);
    if (pcm16) { Pcm16Host p{pcm16}; level[t * 3 + 2] = prosody_acf::loudness_frame(p, H, win0, win_sum, (int)t); }
    else { PcmF32Host p{pcm_f32}; level[t * 3 + 2] = prosody_acf::loudness_frame(p, H, win0, win_sum, (int)t); }
  }
  prosody_acf::contour_utterance(level + 1, 3, T);
}

// level: T x 3; out: rows_of(T, W) x 3. Returns the number of rows.
extern "C" int64_t prosody_acf_smooth(const float *level, int64_t T, int W, float *out) {
  const int64_t rows = prosody_acf::rows_of(T, W);
  for (int64_t n = 0; n < rows; ++n)
    for (int c = 0; c < 3; ++c) out[n * 3 + c] = prosody_acf::sma_row(level + c, 3, (int)T, W, (int)n);
  return rows;
}
