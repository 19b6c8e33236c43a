// Host build of opensmile_amd/csrc/lld_emobase_ops.hpp (tests/test_emobase_host.py): what the emobase chain does outside its
// transforms -- cIntensity, cMZcr, cVectorPreemphasis + cLpc + cLsp per 25 ms frame, cPitchACF's cut-off and contour with F0env per
// utterance, and the rows of cContourSmoother and cDeltaRegression (what lld_emobase_lsp, lld_emobase_contour and lld_emobase_tail run).
#include <cstdint>

#include "../../opensmile_amd/csrc/lld_emobase_ops.hpp"

using namespace smilehip;

namespace {
struct Lsp {                                               // what a lane of lld_emobase_lsp does for its frame
  const float *x; int N; float k, omk; float *lsp, *lpc;
  template <int ORDER> void operator()() { emobase::lsp_from_frame<ORDER>(x, N, k, omk, lsp, lpc); }
};
}  // namespace

extern "C" int64_t emobase_rows_of(int64_t T25, int64_t T40, int W) { return emobase::rows_of(T25, T40, W); }
extern "C" int64_t emobase_row_time_frame(int64_t T25, int64_t T40, int W, int64_t n) { return emobase::row_time_frame(T25, T40, W, n); }

// x: the utterance's samples as floats (R0 done); out25: T25 x (3 + 2 p) = intensity | loudness | zcr | lpc (p) | lsp (p)
extern "C" void emobase_frames25(const float *x, int64_t T25, int N, int H, float k, double w0, double w1, double win_sum, int p, float *out25) {
  for (int64_t t = 0; t < T25; ++t) {
    const float *f = x + t * H;
    float *o = out25 + t * (3 + 2 * p);
    emobase::intensity_frame(f[0], f[1], w0, w1, win_sum, o);
    o[2] = emobase::zcr_frame(f, N);
    Lsp job{f, N, k, 1 - k, o + 3 + p, o + 3};
    emobase::with_order(p, job);
  }
}

// p3: T40 x 3, in: voiceProb | F0raw | anything; out: the level pitch = voiceProb | F0 | F0env
extern "C" void emobase_pitch_level(float *p3, int64_t T40, double voicing_cutoff) {
  if (voicing_cutoff > 1.0) voicing_cutoff = 1.0;         // pitchACF.cpp:96-98
  if (voicing_cutoff < 0.0) voicing_cutoff = 0.0;
  for (int64_t t = 0; t < T40; ++t) p3[t * 3 + 1] = prosody_acf::cut_pitch((double)p3[t * 3], p3[t * 3 + 1], voicing_cutoff);
  emobase::contour_env_utterance(p3, T40);
}

// out: rows x 2 (n25 + 3) = lld | lld_de. Returns the number of rows.
extern "C" int64_t emobase_rows(const float *a25, int64_t T25, const float *p3, int64_t T40, int n25, int W, float *out) {
  const emobase::Levels L = {a25, p3, (int32_t)T25, (int32_t)T40, n25, W};
  const int64_t rows = emobase::rows_of(T25, T40, W);
  const int D = n25 + 3;
  for (int64_t n = 0; n < rows; ++n)
    for (int c = 0; c < D; ++c) {
      out[n * 2 * D + c] = emobase::lld_cell(L, (int)n, c);
      out[n * 2 * D + D + c] = emobase::lld_de_cell(L, (int)n, c);
    }
  return rows;
}
