// Host build of opensmile_amd/csrc/lld_prosody_ops.hpp (tests/test_prosody_shs_host.py): the row function the tail kernel of
// lld_prosody.hip runs one lane per row, here over all rows of one utterance; and cPitchSmoother's level both ways -- the
// windowed replay the row function uses and the plain sequential pass of is10::pitch_smoother_frame over the whole contour.
#include <cstdint>

#include "../../opensmile_amd/csrc/lld_prosody_ops.hpp"

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

// shs: T rows of 21 values; exactly one of pcm16 / pcm_f32; out: rows_of(T, W) x 3. Returns the number of rows.
extern "C" int64_t prosody_rows(const float *shs, int64_t T, const int16_t *pcm16, const float *pcm_f32, float voicing_cutoff, int W, int H,
                                double win0, double win_sum, float *out) {
  prosody::RowConsts c;
  c.voicing_cutoff = voicing_cutoff; c.W = W; c.H = H; c.reserved = 0; c.win0 = win0; c.win_sum = win_sum;
  const int64_t rows = prosody::rows_of(T, W);
  for (int64_t n = 0; n < rows; ++n) {
    float o[3];
    if (pcm16) { Pcm16Host p{pcm16}; prosody::row(c, shs, p, (int)T, (int)n, o); }
    else { PcmF32Host p{pcm_f32}; prosody::row(c, shs, p, (int)T, (int)n, o); }
    for (int q = 0; q < 3; ++q) out[n * 3 + q] = o[q];
  }
  return rows;
}

// the level `pitch` (T - 1 frames x 2) by the windowed replay
extern "C" void prosody_pitch_level_windowed(const float *shs, int64_t T, float voicing_cutoff, float *out) {
  for (int64_t j = 0; j + 1 < T; ++j) {
    float v[2];
    prosody::pitch_level_frame(shs, (int)T, voicing_cutoff, (int)j, v);
    out[j * 2] = v[0];
    out[j * 2 + 1] = v[1];
  }
}

// ... and by one sequential pass of the component's own frame function over the whole contour
extern "C" void prosody_pitch_level_sequential(const float *shs, int64_t T, float voicing_cutoff, float *out) {
  is10::PitchSmootherOpts o;
  o.n_cand = 1; o.octave_correction = 0; o.post_simple = 1; o.flags = 1 | 8;
  o.voicing_cutoff = voicing_cutoff;
  is10::PitchSmootherState st;
  is10::pitch_smoother_reset(st);
  int64_t w = 0;
  for (int64_t t = 0; t < T; ++t) {
    const float cand[3] = {shs[t * 21 + 1], shs[t * 21 + 7], 0.0f};
    float v[2];
    if (is10::pitch_smoother_frame(o, st, cand, 1, v) > 0) { out[w * 2] = v[0]; out[w * 2 + 1] = v[1]; ++w; }
  }
}
