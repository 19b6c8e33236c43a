// config/emobase/emobase.conf, levels lld and lld_de (SMILEHIP_CHAIN_EMOBASE): the sequential recipes of a frame and the row rules of
// [lld:cContourSmoother] and [delta1:cDeltaRegression]. __host__ __device__ like lld_prosody_acf_ops.hpp:
// tests/test_emobase_host.py compiles this header with g++ (tests/helpers/emobase_check.cpp) and holds it against the real binary's
// levels bit for bit without a GPU; lld_emobase.hip calls the same functions.
//
// What the file does, as measured against the binary (tests/golden/make_golden_emobase.py) and read in its source:
//  * Two framers read `wave` with the same step: fr25 (25 ms, T25 frames) and fr40 (40 ms, T40 <= T25 frames). The levels intens (2
//    columns), mfcc1 (12), lsp (p), mzcr (1) hold T25 frames, the level pitch (voiceProb | F0 | F0env) holds T40.
//  * [lld:cContourSmoother] reads the five levels side by side. It writes rows_of(T40, W) = T40 + W rows (W = smaWin / 2) for
//    T40 >= 1 and none for T40 = 0, however many 25 ms frames there are: the shortest level decides. Row n of a column averages
//    positions n - W .. n + W of the column's OWN level, summed centre, -1, +1, -2, +2, ... (contourSmoother.cpp:104-111), positions
//    clamped to that level's frames [0, Tl - 1] (getMatrix replicates the first and the last frame, dataMemoryLevel.cpp:1687-1712):
//    the pitch columns replicate frame T40 - 1 where the other columns still read frames T40 .. T25 - 1 -- no zero is read there.
//    The exception is getMatrix's left-padding branch (n - W < 0, :1687-1698), which reads the level's slots as they are: a position
//    beyond the level's last frame is a slot never written, zero (prosody_acf::sma_row, which this is per column).
//  * Row n carries the time stamp of frame n for n < W, of frame min(n, T25 - 1) otherwise (the first level's time stamps).
//  * [delta1:cDeltaRegression] (deltawin V = 2) runs in the same ticks. Row n of lld_de is the regression over rows n - V .. n + V of
//    lld as they stand WHEN THE ROW IS COMPUTED: before the end of input lld has A = max(T40 - W, 0) rows and lld_de B = max(A - V, 0);
//    afterwards both components write one row per tick, the smoother first, so that row n >= B of lld_de sees
//    de_avail = min(A + (n - B) + 1, T40 + W) rows of lld. Positions are clamped to [0, de_avail - 1], except in the left-padding
//    branch (n - V < 0), where a position >= de_avail reads zero. For T40 > W + V this is the plain clamp to lld's rows.
//    lld_de has as many rows as lld (the sinks read both levels side by side).
// Inputs this was measured on (16 kHz): 0, 100, 399, 400, 560, 639, 640, 720, 800, 880, 2080, 16000, 48000 samples -- (T25, T40) =
// (0,0) (0,0) (0,0) (1,0) (2,0) (2,0) (2,1) (3,1) (3,2) (4,2) (11,10) (98,97) (298,297) -- with smaWin 3, and 400 .. 2080 samples with
// smaWin 5, 7, 9; one input of about 0.3 s at 8, 11.025, 22.05 (T25 = 28, T40 = 26), 32, 44.1 and 48 kHz.
#pragma once
#include <cstdint>

#include "lld_is10_ops.hpp"
#include "lld_pitch_contour.hpp"
#include "lld_prosody_acf_ops.hpp"

namespace smilehip {
namespace emobase {

constexpr int kMaxLpcOrder = 16;                           // cLpc p: even, 2 .. 16
constexpr int kDeltaWin = 2;                               // [delta1:cDeltaRegression] deltawin

GLF_HD int n25_cols(int p) { return 15 + p; }              // intens (2) | mfcc1 (12) | lsp (p) | mzcr (1)
GLF_HD int n_lld(int p) { return 18 + p; }                 // ... | pitch (3)

GLF_HD int64_t frames_of(int64_t len, int64_t N, int64_t H) { return len < N ? 0 : (len - N) / H + 1; }
GLF_HD int64_t rows_of(int64_t T25, int64_t T40, int W) { (void)T25; return T40 >= 1 ? T40 + W : 0; }
// the frame whose time stamp row n carries
GLF_HD int64_t row_time_frame(int64_t T25, int64_t T40, int W, int64_t n) { (void)T40; return n < W ? n : (n < T25 - 1 ? n : T25 - 1); }

// ---- per 25 ms frame ------------------------------------------------------------------------------------------------------
// cMZcr zcr (mzcr.cpp:117-124) on the raw frame x[0 .. N - 1]
template <class X>
GLF_HD float zcr_frame(const X &x, int N) {
  int cnt = 0;
  for (int i = 1; i < N - 1; ++i)
    if (((x[i - 1] * x[i + 1] <= 0.0f) && (x[i] == 0.0f)) || (x[i - 1] * x[i] < 0.0f)) ++cnt;
  return (float)cnt / (float)N;
}

// cIntensity (intensity.cpp:125-145) with both outputs: MIN(N, outputs) = 2 terms of the Hamming-weighted sum; dst = intensity | loudness
GLF_HD void intensity_frame(float x0, float x1, double w0, double w1, double win_sum, float *dst) {
  const float x[2] = {x0, x1};
  const double win[2] = {w0, w1};
  is10::intensity_frame(x, 2, win, win_sum, 3, dst);
}

// cVectorPreemphasis (vectorPreemphasis.cpp:88-100): sample n of the pre-emphasised frame from the raw one
GLF_HD float preemph_sample(float x_n, float x_prev, int n, float k, float one_minus_k) { return n == 0 ? one_minus_k * x_n : x_n - k * x_prev; }

// The three sequential recipes behind cVectorPreemphasis -- cLpc (method = acf, saveLPCoeff only) and cLsp -- with the order known
// at compile time and every loop over coefficients unrolled: the arrays live in registers (a dynamically indexed private array
// would be scratch memory on the device). lld_is10_ops.hpp holds the same recipes for a run-time order.

// smileDsp_autoCorr (smileUtil.c:1560-1570) of the pre-emphasised frame: r[lag] = sum over i = lag .. N - 1 of pe[i] pe[i - lag], a
// float accumulation in sample order per lag; the frame's last ORDER + 1 values are kept in h
template <int ORDER, class X>
GLF_HD void autocorr_preemph(const X &x, int N, float k, float one_minus_k, float (&r)[ORDER + 1]) {
  float h[ORDER + 1];
#pragma unroll
  for (int l = 0; l <= ORDER; ++l) { h[l] = 0.0f; r[l] = 0.0f; }
  float prev = 0.0f;
  for (int i = 0; i < N; ++i) {
    const float xi = x[i];
    const float pe = preemph_sample(xi, prev, i, k, one_minus_k);
    prev = xi;
#pragma unroll
    for (int l = ORDER; l > 0; --l) h[l] = h[l - 1];
    h[0] = pe;
#pragma unroll
    for (int l = 0; l <= ORDER; ++l)
      if (i >= l) r[l] += pe * h[l];
  }
}

// smileDsp_calcLpcAcf (Durbin, smileUtil.c:1572-1630) as cLpc::processVector calls it (lpc.cpp:171-213): all zero for r[0] == 0;
// the recursion stops where the error reaches zero (the coefficients behind stay zero)
template <int ORDER>
GLF_HD void durbin(const float (&r)[ORDER + 1], float (&lpc)[ORDER]) {
#pragma unroll
  for (int i = 0; i < ORDER; ++i) lpc[i] = 0.0f;
  bool live = !(r[0] == 0.0f);
  float e = r[0];
#pragma unroll
  for (int m = 1; m <= ORDER; ++m) {
    if (live) {
      float sum = 1.0f * r[m];
#pragma unroll
      for (int i = 1; i < m; ++i) sum += lpc[i - 1] * r[m - i];
      const float k_m = (-1.0f / e) * sum;
      lpc[m - 1] = k_m;
#pragma unroll
      for (int i = 1; i <= m / 2; ++i) {
        const float xx = lpc[i - 1];
        lpc[i - 1] += k_m * lpc[m - i - 1];
        if ((i < (m / 2)) || ((m & 1) == 1)) lpc[m - i - 1] += k_m * xx;
      }
      e *= (1.0f - k_m * k_m);
      if (e == 0.0f) live = false;
    }
  }
}

// cLsp (src/lld/lsp.cpp:112-312, the Speex-derived lpc_to_lsp): is10::cheb_poly_eva / lpc_to_lsp / lsp_frame for M = ORDER / 2
template <int M>
GLF_HD float cheb_eva(const float (&coef)[M + 1], float x) {
  float b0 = 0.0f, b1 = 0.0f;
  x *= 2.0f;
#pragma unroll
  for (int k = M; k > 0; --k) {
    const float tmp = b0;
    b0 = x * b0 - b1 + coef[M - k];
    b1 = tmp;
  }
  return (-b1 + 0.5f * x * b0 + coef[M]);
}
struct LspSearch { float xr, xl, xm; int roots; };
// one root of the polynomial pt: the grid walk from S.xl downwards, then nb + 1 bisections; *freq receives the root's angle
template <int M>
GLF_HD void lsp_root(const float (&pt)[M + 1], LspSearch &S, int nb, float delta, float *freq) {
  float psuml = cheb_eva<M>(pt, S.xl);
  bool searching = true;
  while (searching && (S.xr >= -1.0f)) {
    float dd = delta * (1.0f - 0.9f * S.xl * S.xl);
    if ((double)__builtin_fabsf(psuml) < .2) dd *= 0.5f;
    S.xr = S.xl - dd;
    float psumr = cheb_eva<M>(pt, S.xr);
    const float temp_psumr = psumr, temp_xr = S.xr;
    if ((psumr * psuml) < 0.0f) {
      S.roots++;
      for (int k = 0; k <= nb; ++k) {
        S.xm = 0.5f * (S.xl + S.xr);
        const float psumm = cheb_eva<M>(pt, S.xm);
        if (!((psumm * psuml) < 0.0f)) { psuml = psumm; S.xl = S.xm; }
        else { psumr = psumm; S.xr = S.xm; }
      }
      if (S.xm > 1.0f) S.xm = 1.0f;
      else if (S.xm < -1.0f) S.xm = -1.0f;
      *freq = glibc_acosf(S.xm);
      S.xl = S.xm;
      searching = false;
    } else {
      psuml = temp_psumr;
      S.xl = temp_xr;
    }
  }
}
// freq: ORDER floats, `stride` apart (the caller's row; positions without a root keep what they hold)
template <int ORDER>
GLF_HD int lpc_to_lsp(const float (&a)[ORDER], float *freq, int64_t stride, int nb, float delta) {
  constexpr int M = ORDER / 2;
  float P[M + 1], Q[M + 1];
  P[0] = 1.0f;
  Q[0] = 1.0f;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    P[i + 1] = (a[i] + a[ORDER - 1 - i]) - P[i];
    Q[i + 1] = (a[i] - a[ORDER - 1 - i]) + Q[i];
  }
#pragma unroll
  for (int i = 0; i < M; ++i) { P[i] = 2.0f * P[i]; Q[i] = 2.0f * Q[i]; }
  LspSearch S = {0.0f, 1.0f, 0.0f, 0};
  for (int jj = 0; jj < M; ++jj) {                         // (roots alternate between the two polynomials: j even P, j odd Q)
    lsp_root<M>(P, S, nb, delta, freq + (int64_t)(2 * jj) * stride);
    lsp_root<M>(Q, S, nb, delta, freq + (int64_t)(2 * jj + 1) * stride);
  }
  return S.roots;
}
template <int ORDER>
GLF_HD void lsp_frame(const float (&lpc)[ORDER], float *dst, int64_t stride) {   // processVector, lsp.cpp:289-312
  for (int i = 0; i < ORDER; ++i) dst[i * stride] = 0.0f;
  int roots = lpc_to_lsp<ORDER>(lpc, dst, stride, 10, 0.2f);
  if (roots != ORDER) {
    roots = lpc_to_lsp<ORDER>(lpc, dst, stride, 10, 0.05f);
    if (roots != ORDER)
      for (int i = roots; i < ORDER; ++i) dst[i * stride] = 0.0f;
  }
}

// cVectorPreemphasis + cLpc + cLsp of the raw 25 ms frame x[0 .. N - 1]: lsp[0 .. ORDER - 1]; lpc_out (optional): the LP coefficients
template <int ORDER, class X>
GLF_HD void lsp_from_frame(const X &x, int N, float k, float one_minus_k, float *lsp, float *lpc_out) {
  float r[ORDER + 1], lpc[ORDER];
  autocorr_preemph<ORDER>(x, N, k, one_minus_k, r);
  durbin<ORDER>(r, lpc);
  if (lpc_out) {
#pragma unroll
    for (int i = 0; i < ORDER; ++i) lpc_out[i] = lpc[i];
  }
  lsp_frame<ORDER>(lpc, lsp, 1);
}
// the orders the chain takes (cLpc p: even, 2 .. 16): f.template operator()<ORDER>() for ORDER == p; false for any other p
template <class F>
GLF_HD bool with_order(int p, F &&f) {
  switch (p) {
    case 2: f.template operator()<2>(); return true;
    case 4: f.template operator()<4>(); return true;
    case 6: f.template operator()<6>(); return true;
    case 8: f.template operator()<8>(); return true;
    case 10: f.template operator()<10>(); return true;
    case 12: f.template operator()<12>(); return true;
    case 14: f.template operator()<14>(); return true;
    case 16: f.template operator()<16>(); return true;
  }
  return false;
}

// ---- per 40 ms frame / utterance --------------------------------------------------------------------------------------------
// the level `pitch`, columns F0 | F0env: cPitchACF's contour over an utterance's T40 cut-off candidates (in p3[1], stride 3), in
// place; F0env (pitchACF.cpp:236-240) follows the emitted value
GLF_HD void contour_env_utterance(float *p3, int64_t T40) {
  PitchContour S = {};
  for (int64_t t = 0; t < T40; ++t) {
    p3[t * 3 + 1] = pitch_contour_step(S, p3[t * 3 + 1]);
    p3[t * 3 + 2] = S.env;
  }
}

// ---- the rows ----------------------------------------------------------------------------------------------------------------
// Levels of one utterance in front of the smoother: a25 = [T25 x n25] (intens | mfcc1 | lsp | mzcr), p3 = [T40 x 3] (pitch)
struct Levels {
  const float *a25;
  const float *p3;
  int32_t T25, T40, n25, W;
};

// cell (row n, column c) of the level lld, 0 <= n < rows_of, 0 <= c < n25 + 3
GLF_HD float lld_cell(const Levels &L, int n, int c) {
  return c < L.n25 ? prosody_acf::sma_row(L.a25 + c, L.n25, L.T25, L.W, n) : prosody_acf::sma_row(L.p3 + (c - L.n25), 3, L.T40, L.W, n);
}

// rows of lld that exist when row n of lld_de is computed
GLF_HD int de_avail(int T40, int W, int n) {
  const int R = T40 + W, A = T40 - W > 0 ? T40 - W : 0, B = A - kDeltaWin > 0 ? A - kDeltaWin : 0;
  if (n < B) return R;                                     // (every row it reads exists: n + V < A)
  const int a = A + (n - B) + 1;
  return a < R ? a : R;
}

// cell (row n, column c) of the level lld_de (deltaRegression.cpp:144-152, norm :77-79)
GLF_HD float lld_de_cell(const Levels &L, int n, int c) {
  constexpr int V = kDeltaWin;
  const int avail = de_avail(L.T40, L.W, n);
  const bool left_pad = n - V < 0;
  auto value = [&](int i) {
    const int j = i < 0 ? 0 : (i > avail - 1 ? avail - 1 : i);
    const float v = lld_cell(L, j, c);
    return (left_pad && i > avail - 1) ? 0.0f : v;
  };
  float norm = 0.0f;
  for (int i = 1; i <= V; ++i) norm += (float)i * (float)i;
  norm *= 2.0;
  float num = 0.0f;
  for (int k = 1; k <= V; ++k) {
    const float delta = value(n + k) - value(n - k);
    num += (float)k * delta;
  }
  return num / norm;
}

}  // namespace emobase
}  // namespace smilehip
