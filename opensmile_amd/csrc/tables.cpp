// Host-side table generation (see tables.hpp). Each function names the
// reference lines whose precision recipe it follows.
#include "tables.hpp"

#include <cmath>

#include "glibc_float.hpp"

namespace smilehip {

static int64_t next_pow2(int64_t x) {
  int64_t y = 1;
  while (y < x) y <<= 1;
  return y;
}

// Framing integers: src/core/winToVecProcessor.cpp:435-456 (round(frameSize/T)),
// T from src/iocore/waveSource.cpp:190; FFT length and the rescaled
// frameSizeSec: src/dspcore/transformFft.cpp:66-96,119-137.
int make_geometry(const smilehip_lld_config &c, Geometry &g) {
  if (!(c.sample_rate >= 1.0) || !(c.frame_size_sec > 0.0) || c.frame_step_sec < 0.0)
    return SMILEHIP_ERR_INVALID;
  const double T = 1.0 / static_cast<double>(static_cast<long>(c.sample_rate));
  g.period = T;
  g.N = std::lround(c.frame_size_sec / T);
  const double step = (c.frame_step_sec == 0.0) ? c.frame_size_sec : c.frame_step_sec;
  g.H = std::lround(step / T);
  if (c.force_frame_size > 0) g.N = c.force_frame_size;   // single-component plan: size of the input field
  if (g.H == 0) g.H = g.N;
  if (g.N < 1) return SMILEHIP_ERR_INVALID;
  g.frame_period = step;
  int64_t nfft = g.N;
  double fss = c.frame_size_sec;
  if ((nfft & (nfft - 1)) != 0) {
    nfft = next_pow2(g.N);
    fss *= static_cast<double>(nfft) / static_cast<double>(g.N);
  }
  if (nfft < 4) nfft = 4;
  g.Nfft = nfft;
  g.K = nfft / 2 + 1;
  g.fft_frame_size_sec = (c.force_fft_frame_size_sec > 0.0) ? c.force_fft_frame_size_sec : fss;
  return SMILEHIP_OK;
}

// Window shapes: src/smileutil/smileUtil.c:1218-1350 evaluated in double, gain
// folded in double (src/dspcore/windower.cpp:193-197), then the per-use
// (FLOAT_DMEM) cast of windower.cpp:226 applied once here.
int make_window(const smilehip_lld_config &c, int64_t N, std::vector<float> &w) {
  std::vector<double> d(static_cast<size_t>(N));
  const double NN = static_cast<double>(N);
  const double pi = M_PI;
  switch (c.win_func) {
    case SMILEHIP_WIN_RECT:
      for (auto &v : d) v = 1.0;
      break;
    case SMILEHIP_WIN_HANN:
      for (int64_t n = 0; n < N; ++n) d[n] = 0.5 * (1.0 - std::cos((2.0 * pi * double(n)) / (NN - 1.0)));
      break;
    case SMILEHIP_WIN_HAMM:
      for (int64_t n = 0; n < N; ++n) d[n] = 0.54 - 0.46 * std::cos((2.0 * pi * double(n)) / (NN - 1.0));
      break;
    case SMILEHIP_WIN_SINE:
      for (int64_t n = 0; n < N; ++n) d[n] = std::sin((1.0 * pi * double(n)) / (NN - 1.0));
      break;
    case SMILEHIP_WIN_GAUSS: {
      double sigma = c.win_sigma;
      if (sigma <= 0.0) sigma = 0.01;
      if (sigma > 0.5) sigma = 0.5;
      for (int64_t n = 0; n < N; ++n) {
        const double t = (double(n) - (NN - 1.0) / 2.0) / (sigma * (NN - 1.0) / 2.0);
        d[n] = std::exp(-0.5 * (t * t));
      }
      break;
    }
    case SMILEHIP_WIN_TRI:
      for (int64_t n = 0; n < N / 2; ++n) d[n] = 2.0 * double(n + 1) / double(N);
      for (int64_t n = N / 2; n < N; ++n) d[n] = 2.0 * double(N - n) / double(N);
      break;
    case SMILEHIP_WIN_BARTLETT:
      for (int64_t n = 0; n < N / 2; ++n) d[n] = 2.0 * double(n) / double(N - 1);
      for (int64_t n = N / 2; n < N; ++n) d[n] = 2.0 * double(N - 1 - n) / double(N - 1);
      break;
    case SMILEHIP_WIN_LANCZOS:
      for (int64_t n = 0; n < N; ++n) {
        const double y = pi * ((2.0 * double(n)) / (NN - 1.0) - 1.0);
        d[n] = std::sin(y) / y;
      }
      break;
    default:
      return SMILEHIP_ERR_INVALID;
  }
  if (c.win_gain != 1.0)
    for (auto &v : d) v *= c.win_gain;
  w.resize(static_cast<size_t>(N));
  for (int64_t n = 0; n < N; ++n) w[n] = static_cast<float>(d[n]);
  return SMILEHIP_OK;
}

// Mel axis: smileDsp_specScaleTransfFwd, SPECTSCALE_MEL (smileUtil.c:1138-1141)
static double to_mel(double hz) { return hz > 0.0 ? 1127.0 * std::log(1.0 + hz / 700.0) : 0.0; }
// cMelspec::NtoFmel (src/include/lldcore/melspec.hpp:119-122): float product, double mel, float result
static float bin_to_mel(int64_t n, float F0) { return static_cast<float>(to_mel(double(float(n) * F0))); }

// HTK-style triangular bank stored as one weight per bin + channel map:
// cMelspec::computeFilters, src/lldcore/melspec.cpp:184-238 and :391-449.
int make_mel(const smilehip_lld_config &c, const Geometry &g, MelBank &m) {
  const int64_t K = g.K;
  const int nB = c.n_bands;
  if (nB < 1 || K < nB) return SMILEHIP_ERR_INVALID;
  m.n_bands = nB;
  m.coef.assign(static_cast<size_t>(K), 0.0f);
  m.chan.assign(static_cast<size_t>(K), -3);
  m.centres.assign(static_cast<size_t>(nB + 2), 0.0f);

  const float Nf = static_cast<float>((K - 1) * 2);
  const float F0 = static_cast<float>(1.0 / g.fft_frame_size_sec);
  const float Fs = static_cast<float>(Nf / g.fft_frame_size_sec);
  const float M = static_cast<float>(nB);
  float lo = c.lofreq, hi = c.hifreq;
  if ((lo < 0.0) || (lo > Fs / 2.0) || (lo > hi)) lo = 0.0;
  if ((hi < lo) || (hi > Fs / 2.0) || (hi <= 0.0)) hi = Fs / 2.0f;
  const float LoF = static_cast<float>(to_mel(double(lo)));
  const float HiF = static_cast<float>(to_mel(double(hi)));
  int64_t nLo = std::lround(double(lo / F0));
  int64_t nHi = std::lround(double(hi / F0));
  if (nLo > K) nLo = K;
  if (nHi > K) nHi = K;
  if (nLo < 0) nLo = 0;
  if (nHi < 0) nHi = 0;
  m.nLo = nLo;
  m.nHi = nHi;

  const float bw = (HiF - LoF) / (M + 1.0f);
  for (int b = 0; b <= nB + 1; ++b) m.centres[b] = LoF + float(b) * bw;

  int mm = 0;
  for (int64_t n = 0; n < K; ++n) {
    if ((n <= nLo) || (n >= nHi)) {
      m.chan[n] = -3;
    } else {
      while (m.centres[mm] < bin_to_mel(n, F0)) {
        if (mm > nB) break;
        ++mm;
      }
      m.chan[n] = mm - 2;
    }
  }
  mm = 0;
  for (int64_t n = nLo; n < nHi; ++n) {
    const float nM = bin_to_mel(n, F0);
    while ((nM > m.centres[mm + 1]) && (mm <= nB)) ++mm;
    m.coef[n] = (m.centres[mm + 1] - nM) / (m.centres[mm + 1] - m.centres[mm]);
  }

  // Per-band bin ranges. processVector (melspec.cpp:544-553) walks the bins in
  // ascending order and adds p*w to band chan[n] (if > -1) and p - p*w to band
  // chan[n]+1 (if chan[n] > -2 and < nB-1); chan[] is non-decreasing, so each
  // band receives first a run of "rising" bins then a run of "falling" bins.
  m.rise_lo.assign(nB, 0); m.rise_hi.assign(nB, 0);
  m.fall_lo.assign(nB, 0); m.fall_hi.assign(nB, 0);
  for (int b = 0; b < nB; ++b) {
    int64_t rl = -1, rh = -1, fl = -1, fh = -1;
    for (int64_t n = nLo; n < nHi; ++n) {
      const int ch = m.chan[n];
      if (ch <= -2) continue;
      if (ch == b - 1 && ch < nB - 1) { if (rl < 0) rl = n; rh = n + 1; }
      if (ch == b && ch > -1)         { if (fl < 0) fl = n; fh = n + 1; }
    }
    if (rl < 0) rl = rh = 0;
    if (fl < 0) fl = fh = 0;
    // contiguity is what the device loops rely on
    for (int64_t n = rl; n < rh; ++n) if (m.chan[n] != b - 1) return SMILEHIP_ERR_INVALID;
    for (int64_t n = fl; n < fh; ++n) if (m.chan[n] != b) return SMILEHIP_ERR_INVALID;
    if (rh > rl && fh > fl && fl < rh) return SMILEHIP_ERR_INVALID;
    m.rise_lo[b] = int32_t(rl); m.rise_hi[b] = int32_t(rh);
    m.fall_lo[b] = int32_t(fl); m.fall_hi[b] = int32_t(fh);
  }
  // HTK sample scaling, melspec.cpp:559-570
  m.scale = 1.0f;
  if (c.mel_htk_compatible) m.scale = c.use_power ? float(32767.0 * 32767.0) : float(32767.0);
  return SMILEHIP_OK;
}

// DCT-II rows + lifter: cMfcc::initTables, src/lldcore/mfcc.cpp:136-170; output
// ordering and the single float product lifter*factor: mfcc.cpp:246-273.
int make_dct(const smilehip_lld_config &c, DctTables &d) {
  const int nB = c.n_bands;
  d.n_bands = nB;
  d.first = c.first_mfcc;
  d.last = c.last_mfcc;
  d.n_mfcc = d.last - d.first + 1;
  if (d.n_mfcc < 1 || d.first < 0) return SMILEHIP_ERR_INVALID;
  const bool htk = c.mfcc_htk_compatible != 0;
  d.melfloor = htk ? 1.0f : c.melfloor;              // mfcc.cpp:88-91
  d.log_floor = std::log(d.melfloor);                // mfcc.cpp:241
  std::vector<float> costable(size_t(nB) * size_t(d.n_mfcc));
  const double fnM = double(nB);
  for (int i = d.first; i <= d.last; ++i) {
    const double fi = double(i);
    for (int mI = 0; mI < nB; ++mI)
      costable[size_t(mI) + size_t(i - d.first) * nB] =
          float(std::cos(double(M_PI) * (fi / fnM) * (double(mI) + 0.5)));
  }
  d.lifter.assign(d.n_mfcc, 1.0f);
  if (c.cep_lifter > 0.0f) {
    for (int i = d.first; i <= d.last; ++i)
      d.lifter[i - d.first] = 1.0f + c.cep_lifter / 2.0f * std::sin(float(M_PI) * float(i) / c.cep_lifter);
  }
  const float factor = float(std::sqrt(2.0 / double(nB)));
  d.cos_rows.assign(size_t(nB) * size_t(d.n_mfcc), 0.0f);
  d.gain.assign(d.n_mfcc, 0.0f);
  for (int i = d.first; i <= d.last; ++i) {
    const int r = i - d.first;       // output position
    int i0 = r;
    if (htk && d.first == 0) i0 = (i == d.last) ? 0 : r + 1;   // c0 goes last
    for (int mI = 0; mI < nB; ++mI) d.cos_rows[size_t(r) * nB + mI] = costable[size_t(mI) + size_t(i0) * nB];
    d.gain[r] = d.lifter[i0] * factor;
  }
  return SMILEHIP_OK;
}

// deltaRegression.cpp:77-79
float delta_norm(int W) {
  float norm = 0.0f;
  for (int i = 1; i <= W; ++i) norm += float(i) * float(i);
  norm *= 2.0;
  return norm;
}

}  // namespace smilehip

namespace smilehip {

// cSpecScale::dataProcessorCustomFinalise (src/dsp/specScale.cpp:228-300), smileMath_cspline_init /
// smileMath_csplint_init (src/smileutil/smileUtilSpline.c:139-155, 296-342), the level meta data cPitchShs reads
// in setupNewNames (src/lld/pitchShs.cpp:178-204) and its per-harmonic shifts (:235-243). All in double, rounded
// where the reference rounds (the meta data travels as FLOAT_DMEM).
int make_f0_tables(int64_t K, double fft_frame_size_sec, int n_harmonics, float compression, double min_f, F0Host &h) {
  if (K < 4 || n_harmonics < 1 || n_harmonics > 17 || !(min_f > 0.0)) return SMILEHIP_ERR_INVALID;
  const double fsSec = (double)(float)fft_frame_size_sec;
  const double deltaF = 1.0 / fsSec;
  const double minF = min_f;
  const double maxF = deltaF * (double)(K - 1);
  const double l2 = std::log(2.0);
  const double fmin_t = std::log(minF) / l2, fmax_t = std::log(maxF) / l2;
  const double step_t = (fmax_t - fmin_t) / (double)(K - 1);
  std::vector<double> x(static_cast<size_t>(K));
  for (int64_t i = 1; i < K; ++i) x[i] = std::log((double)i * deltaF) / l2;
  x[0] = 2.0 * x[1] - x[2];
  h.sp_rec.assign(size_t(K) * 4, 0.0);
  h.sp_d1.assign(size_t(K), 1.0);
  h.sp_d2.assign(size_t(K), 1.0);
  double dec_prev = 0.0;                                  // y2[0] = 0 (natural boundary)
  for (int64_t i = 1; i < K - 1; ++i) {
    const double sigma = (x[i] - x[i - 1]) / (x[i + 1] - x[i - 1]);
    h.sp_d1[i] = (x[i + 1] - x[i]) * (x[i + 1] - x[i - 1]);
    h.sp_d2[i] = (x[i] - x[i - 1]) * (x[i + 1] - x[i - 1]);
    const double p = 1.0 / (sigma * dec_prev + 2.0);
    const double dec = (sigma - 1.0) * p;
    h.sp_rec[4 * i + 0] = sigma;
    h.sp_rec[4 * i + 1] = p;
    h.sp_rec[4 * i + 2] = dec;
    dec_prev = dec;
  }
  h.ip_k.assign(size_t(K), 0);
  h.ip_co.assign(size_t(K) * 3, 0.0);
  int64_t hi = 1;
  for (int64_t i = 0; i < K; ++i) {
    const double xt = fmin_t + (double)i * step_t;
    if (i == 0 && xt < x[0]) return SMILEHIP_ERR_INVALID;
    while (hi < K && x[hi] < xt) hi++;
    if (hi == K) return SMILEHIP_ERR_INVALID;             // the reference's csplint_init fails here too
    const int64_t lo = hi - 1;
    const double range = x[hi] - x[lo];
    if (range == 0.0) return SMILEHIP_ERR_INVALID;
    const double a = (x[hi] - xt) / range, b = 1.0 - a, r2 = range * range / 6.0;
    h.ip_k[i] = (int32_t)lo;
    h.ip_co[3 * i + 0] = a;
    h.ip_co[3 * i + 1] = (a * a * a - a) * r2;
    h.ip_co[3 * i + 2] = (b * b * b - b) * r2;
  }
  const double nOct = std::log(maxF / minF) / l2;
  const double nPPO = (double)K / nOct;
  const double atan_s = nPPO * (std::log(65.0 / 50.0) / l2) - 1.0;
  h.audw.assign(size_t(K), 0.0);
  for (int64_t i = 0; i < K; ++i) h.audw[i] = 0.5 + std::atan(3.0 * ((double)i + 1 - atan_s) / nPPO) / M_PI;
  // the same constants as the thread-per-frame sweep reads them: one record per target point, and how many target
  // points sit above each source bin (the search above only moves `hi` up: ip_k is non-decreasing)
  h.ip_rec.assign(size_t(K) * 4, 0.0);
  h.ip_cnt.assign(size_t((K + 15) / 16 * 16), 0);
  h.sw_rec.assign(size_t(K) * 8, 0.0);
  for (int64_t i = 0; i < K; ++i) {
    h.sw_rec[8 * i + 0] = h.sp_rec[4 * i + 0]; h.sw_rec[8 * i + 1] = h.sp_rec[4 * i + 1]; h.sw_rec[8 * i + 2] = h.sp_rec[4 * i + 2];
    h.sw_rec[8 * i + 3] = h.sp_d1[i]; h.sw_rec[8 * i + 4] = 1.0 / h.sp_d1[i];
    h.sw_rec[8 * i + 5] = h.sp_d2[i]; h.sw_rec[8 * i + 6] = 1.0 / h.sp_d2[i];
  }
  for (int64_t i = 0; i < K; ++i) {
    h.ip_rec[4 * i + 0] = h.ip_co[3 * i + 0];
    h.ip_rec[4 * i + 1] = h.ip_co[3 * i + 1];
    h.ip_rec[4 * i + 2] = h.ip_co[3 * i + 2];
    h.ip_rec[4 * i + 3] = h.audw[i];
    if (i > 0 && h.ip_k[i] < h.ip_k[i - 1]) return SMILEHIP_ERR_INVALID;
    h.ip_cnt[h.ip_k[i]] += 1;
  }
  // what cPitchShs sees: FLOAT_DMEM meta data
  const float m_fmin = (float)minF, m_ppo = (float)nPPO, m_fmint = (float)fmin_t, m_fmaxt = (float)fmax_t;
  double base = std::exp(std::log((double)m_fmin) / (double)m_fmint);
  if (std::fabs(base - 2.0) < 0.00001) base = 2.0;
  h.log_base = std::log(base);
  h.Fmint = m_fmint;
  h.Fstept = (m_fmaxt - m_fmint) / (float)(K - 1);
  h.n_harm = n_harmonics;
  float sc = compression;
  for (int i = 2; i < n_harmonics + 1; ++i) {
    h.shift[i - 2] = (int32_t)std::floor((double)m_ppo * (std::log((double)i) / l2));
    h.scale[i - 2] = sc;
    sc *= compression;
  }
  return SMILEHIP_OK;
}

// smileDsp_specScaleTransfFwd (src/smileutil/smileUtil.c:1097-1147) for the scales cSpecScale::myFetchConfig can select
static double specscale_fwd(double x, int scale, double param) {
  switch (scale) {
    case SMILEHIP_SPECSCALE_LOG:
      if (x > 0) return std::log(x) / std::log(param);
      return 0.0;
    case SMILEHIP_SPECSCALE_SEMITONE:
      if (x / param > 1.0) return 12.0 * (std::log(x / param) / std::log(2.0));
      return 0.0;
    case SMILEHIP_SPECSCALE_BARK_OLD:
      if (x > 0) return (26.81 / (1.0 + 1960.0 / x)) - 0.53;
      return 0.0;
    case SMILEHIP_SPECSCALE_BARK:
      if (x > 0) {
        const double zz = (26.81 / (1.0 + 1960.0 / x)) - 0.53;
        if (zz < 2) return (0.85 * zz + 0.3);
        else if (zz > 20.1) return (1.22 * zz - 0.22 * 20.1);
        return zz;
      }
      return 0.0;
    case SMILEHIP_SPECSCALE_MEL:
      if (x > 0.0) return 1127.0 * std::log(1.0 + x / 700.0);
      return 0.0;
    default:
      return x;
  }
}

// cSpecScale::myFetchConfig's clamps (src/dsp/specScale.cpp:151-186), setupNewNames' deltaF and nPointsTarget (:214-217),
// dataProcessorCustomFinalise (:248-321), smileMath_cspline_init / smileMath_csplint_init (src/smileutil/smileUtilSpline.c:138-153,
// 295-342) and the data-independent half of smileMath_cspline (:172-184: y2 of the forward sweep never sees the spectrum). Where
// the reference's own setup is undefined -- a source axis that does not increase, NaN tables, a failed csplint_init whose null
// cache processVector then dereferences, one target point -- the geometry is refused by name.
int make_specscale_tables(const smilehip_specscale_opts &o, int64_t n_src, double frame_size_sec, SpecScaleHost &h, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  const int scale = o.scale;
  if (scale != SMILEHIP_SPECSCALE_LOG && scale != SMILEHIP_SPECSCALE_SEMITONE && scale != SMILEHIP_SPECSCALE_LINEAR &&
      scale != SMILEHIP_SPECSCALE_BARK && scale != SMILEHIP_SPECSCALE_BARK_OLD && scale != SMILEHIP_SPECSCALE_MEL) {
    *why = "unknown target scale";
    return SMILEHIP_ERR_INVALID;
  }
  if (n_src < 4 || n_src > 8193) { *why = "4 .. 8193 source bins are built"; return SMILEHIP_ERR_INVALID; }
  if (!(frame_size_sec > 0.0)) { *why = "the level's frameSizeSec must be positive"; return SMILEHIP_ERR_INVALID; }
  const int64_t n_tgt = o.n_points_target <= 0 ? n_src : (int64_t)o.n_points_target;
  if (n_tgt == 1) { *why = "nPointsTarget = 1: the target axis' step is a division by zero"; return SMILEHIP_ERR_INVALID; }
  if (n_tgt > 16384) { *why = "2 .. 16384 target points are built"; return SMILEHIP_ERR_INVALID; }
  double param = 0.0;
  if (scale == SMILEHIP_SPECSCALE_LOG) {
    param = o.param;
    if ((param <= 0.0) || (param == 1.0)) param = 2.0;
  } else if (scale == SMILEHIP_SPECSCALE_SEMITONE) {
    param = o.param;
  }
  const int nMag = (int)n_src, nPointsTarget = (int)n_tgt;
  const double deltaF = 1.0 / (double)(float)frame_size_sec;
  double minF = o.min_f, maxF = o.max_f;
  if (minF < 1.0) minF = 1.0;
  const double samplF = deltaF * (double)(nMag - 1);
  if ((maxF <= minF) || (maxF > samplF)) maxF = samplF;
  const double fmin_t = specscale_fwd(minF, scale, param);
  const double fmax_t = specscale_fwd(maxF, scale, param);
  const double deltaF_t = (fmax_t - fmin_t) / (nPointsTarget - 1);
  h.n_src = nMag; h.n_tgt = nPointsTarget;
  h.min_f = minF; h.max_f = maxF; h.fmin_t = fmin_t; h.fmax_t = fmax_t;
  std::vector<double> &x = h.f_t;
  x.assign((size_t)nMag, 0.0);
  if (scale == SMILEHIP_SPECSCALE_LOG) {
    for (int i = 1; i < nMag; i++) x[i] = specscale_fwd((double)i * (double)deltaF, scale, param);
    x[0] = 2.0 * x[1] - x[2];
  } else {
    for (int i = 0; i < nMag; i++) x[i] = specscale_fwd((double)i * (double)deltaF, scale, param);
  }
  for (int i = 1; i < nMag; i++)
    if (!(x[i] > x[i - 1])) {                             // (also catches NaN / Inf axes: a log base whose logarithm underflows, ...)
      *why = "the source bins do not increase on the target axis (sem: firstNote at or above the bin spacing; bao: a bin spacing below about 39.5 Hz)";
      return SMILEHIP_ERR_INVALID;
    }
  h.spline.assign((size_t)nMag * 5, 0.0);
  double y2_prev = 0.0;                                   // y2[0] = 0 (natural boundary, y1p = 1e30)
  for (int i = 1; i < nMag - 1; i++) {
    const double sigma = (x[i] - x[i - 1]) / (x[i + 1] - x[i - 1]);
    const double diff1 = (x[i + 1] - x[i]) * (x[i + 1] - x[i - 1]);
    const double diff2 = (x[i] - x[i - 1]) * (x[i + 1] - x[i - 1]);
    if (diff1 == 0.0 || diff2 == 0.0 || !std::isfinite(diff1) || !std::isfinite(diff2)) {
      *why = "the source bins lie too close on the target axis: a spline interval's width underflows";
      return SMILEHIP_ERR_INVALID;
    }
    const double p = 1.0 / (sigma * y2_prev + 2.0);
    const double y2 = (sigma - 1.0) * p;
    double *r = &h.spline[(size_t)i * 5];
    r[0] = sigma; r[1] = diff1; r[2] = diff2; r[3] = p; r[4] = y2;
    y2_prev = y2;
  }
  h.ip_k.assign((size_t)nPointsTarget, 0);
  h.ip_rec.assign((size_t)nPointsTarget * 4, 0.0);
  const double xt_first = fmin_t + (double)0 * deltaF_t, xt_last = fmin_t + (double)(nPointsTarget - 1) * deltaF_t;
  if (!std::isfinite(xt_first) || !std::isfinite(xt_last)) { *why = "the target axis is not finite"; return SMILEHIP_ERR_INVALID; }
  if (xt_first < x[0] || xt_last > x[nMag - 1]) {
    *why = "smileMath_csplint_init fails in the reference: a target point lies outside the source axis";
    return SMILEHIP_ERR_INVALID;
  }
  long kupper = 1;
  for (int i = 0; i < nPointsTarget; i++) {
    const double xt = fmin_t + (double)i * deltaF_t;
    while (kupper < nMag && x[kupper] < xt) kupper++;
    if (kupper == nMag) {
      *why = "smileMath_csplint_init fails in the reference: a target point lies outside the source axis";
      return SMILEHIP_ERR_INVALID;
    }
    const long klower = kupper - 1;
    const double range = x[kupper] - x[klower];
    if (range == 0.0) { *why = "smileMath_csplint_init fails in the reference: a source interval of width zero"; return SMILEHIP_ERR_INVALID; }
    const double a = (x[kupper] - xt) / range;
    const double b = 1.0 - a;
    const double range2 = range * range / 6.0;
    h.ip_k[(size_t)i] = (int32_t)klower;
    h.ip_rec[(size_t)i * 4 + 0] = a;
    h.ip_rec[(size_t)i * 4 + 1] = (a * a * a - a) * range2;
    h.ip_rec[(size_t)i * 4 + 2] = (b * b * b - b) * range2;
    h.ip_rec[(size_t)i * 4 + 3] = 1.0;
  }
  h.weighting = (o.auditory_weighting && scale == SMILEHIP_SPECSCALE_LOG && param == 2.0) ? 1 : 0;
  if (h.weighting) {
    const double nOctaves = std::log(maxF / minF) / std::log(2.0);
    const double nPointsPerOctave = nPointsTarget / nOctaves;
    const double atan_s = nPointsPerOctave * (std::log(65.0 / 50.0) / std::log(2.0)) - 1.0;
    for (int i = 0; i < nPointsTarget; i++) {
      const double w = 0.5 + std::atan(3.0 * (i + 1 - atan_s) / nPointsPerOctave) / M_PI;
      if (!std::isfinite(w)) { *why = "the auditory weighting is not finite (a target range of zero octaves)"; return SMILEHIP_ERR_INVALID; }
      h.ip_rec[(size_t)i * 4 + 3] = w;
    }
  }
  return SMILEHIP_OK;
}

// smileDsp_specScaleTransfInv (src/smileutil/smileUtil.c:1158-1199) for the same scales
static double specscale_inv(double x, int scale, double param) {
  switch (scale) {
    case SMILEHIP_SPECSCALE_LOG:
      return std::exp(x * std::log(param));
    case SMILEHIP_SPECSCALE_SEMITONE:
      return param * std::pow(2.0, x / 12.0);
    case SMILEHIP_SPECSCALE_BARK_OLD: {
      const double z0 = (x + 0.53) / 26.81;
      if (z0 != 1.0) return (1960.0 * z0) / (1.0 - z0);
      return 0.0;
    }
    case SMILEHIP_SPECSCALE_BARK: {
      double zz = x;
      if (x > 20.1) zz = (x + 0.22 * 20.1) / 1.22;
      else if (x < 2) zz = (x - 0.3) / 0.85;
      const double z0 = 26.81 / (zz + 0.53);
      if (z0 != 1.0) return 1960.0 / (z0 - 1.0);
      return 0.0;
    }
    case SMILEHIP_SPECSCALE_MEL:
      return 700.0 * (std::exp(x / 1127.0) - 1.0);
    default:
      return x;
  }
}

// f * smileDsp_getSharpnessWeightG(f, SPECTSCALE_BARK, 0.0) (smileUtil.c:1064-1078) for f in Bark
static double sharpness_weight(double bark) {
  const double g = (bark <= 16.0) ? 1.0 : std::pow((bark - 16.0) / 4.0, 1.5849625) + 1.0;
  return bark * g;
}

// cSpectral::processVector's setup (src/lldcore/spectral.cpp): the range bins (:625-647), the band and slope edges in the axis form
// and in the index form (:771-840, :873-946), the slope's axis sums (:1400-1418), where the alpha ratio's and the Hammarberg index'
// walks change band and stop (:995-1089), the sharpness weights (:1438-1468), the floor of the log spectrum (:85-91, :228-237).
// Without an axis the reference's nScale is 0 (:601), so the interior loop of slopes[] (`ii < nScale`, :969) never runs, the
// centroid's axis is the running sum f += F0 from 0 at the range's first bin (:1291-1294) and the sharpness weights continue that
// same f (:1464-1466). What the reference leaves undefined is refused by the option's name.
int make_spectral_axis_tables(const smilehip_spectral_axis_opts &o, int64_t K, double frame_size_sec, const double *frq, int64_t n_scale,
                              SpectralAxisHost &h, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  *why = "";
  const smilehip_spectral_opts &b = o.base;
  if (K < 4 || K > (1 << 20)) { *why = "K: 4 .. 1048576 bins are built"; return SMILEHIP_ERR_INVALID; }
  if (!(frame_size_sec > 0.0)) { *why = "frame_size_sec: the level's frameSizeSec must be positive"; return SMILEHIP_ERR_INVALID; }
  if (o.tonality) { *why = "tonality: not implemented in the reference (it writes 0 and prints an error)"; return SMILEHIP_ERR_INVALID; }
  if (b.n_bands < 0 || b.n_bands > 16) { *why = "bands: 0 .. 16 are built"; return SMILEHIP_ERR_INVALID; }
  if (b.n_slopes < 0 || b.n_slopes > 16) { *why = "slopes: 0 .. 16 are built"; return SMILEHIP_ERR_INVALID; }
  if (b.n_rolloff < 0 || b.n_rolloff > 16) { *why = "rollOff: 0 .. 16 points are built"; return SMILEHIP_ERR_INVALID; }
  for (int i = 0; i < b.n_rolloff; ++i)
    if (!(b.rolloff[i] >= 0.0 && b.rolloff[i] <= 1.0)) { *why = "rollOff: a point outside 0 .. 1"; return SMILEHIP_ERR_INVALID; }
  if (frq && n_scale < K) { *why = "n_scale: an axis shorter than the spectrum (the reference then mixes the two forms)"; return SMILEHIP_ERR_INVALID; }
  if (!frq && n_scale != 0) { *why = "n_scale: must be 0 without an axis"; return SMILEHIP_ERR_INVALID; }
  const int fs = o.frq_scale;
  if (fs != SMILEHIP_SPECSCALE_LINEAR && fs != SMILEHIP_SPECSCALE_LOG && fs != SMILEHIP_SPECSCALE_BARK && fs != SMILEHIP_SPECSCALE_MEL &&
      fs != SMILEHIP_SPECSCALE_SEMITONE && fs != SMILEHIP_SPECSCALE_BARK_OLD) { *why = "frq_scale: unknown scale"; return SMILEHIP_ERR_INVALID; }
  const int Nsrc = (int)K;
  const bool axis = frq != nullptr;
  if (axis)
    for (int i = 0; i < Nsrc; ++i)
      if (!std::isfinite(frq[i]) || (i > 0 && !(frq[i] > frq[i - 1]))) { *why = "frq: the axis does not increase"; return SMILEHIP_ERR_INVALID; }
  if (o.freq_lo < 0 || o.freq_hi < o.freq_lo) { *why = "freqRange: 0 <= lower <= upper"; return SMILEHIP_ERR_INVALID; }
  h = SpectralAxisHost();
  h.K = Nsrc; h.has_axis = axis ? 1 : 0;
  h.n_out = smilehip_spectral_axis_opts_count(&o);
  if (h.n_out < 1) { *why = "no output is switched on"; return SMILEHIP_ERR_INVALID; }
  const double F0 = 1.0 / frame_size_sec;
  // :85-91, :228-237
  if (o.use_log_spectrum) {
    float sf = (float)o.spec_floor;
    if (!(sf > 0.0f) || !std::isfinite(sf)) { *why = "specFloor: must be positive (its logarithm is the floor)"; return SMILEHIP_ERR_INVALID; }
    sf = sf * sf;
    if (!(sf > 0.0f)) { *why = "specFloor: its square underflows"; return SMILEHIP_ERR_INVALID; }
    h.spec_floor = sf;
  } else {
    h.spec_floor = (float)(0.0000001 * 0.0000001);
  }
  h.log_spec_floor = (float)(10.0 * (double)glibc_logf(h.spec_floor) / std::log(10.0));
  h.log_spec_factor = (float)(10.0 / std::log(10.0));
  // :625-647
  if (o.freq_lo == 0 && o.freq_hi == 0) {
    h.lo = 1; h.hi = Nsrc - 1;
  } else {
    if (!axis) { *why = "freqRange: a range other than 0-0 reads the axis"; return SMILEHIP_ERR_INVALID; }
    int lb = -1, ub = -1;
    for (int i = 0; i < Nsrc; i++) {
      if ((double)o.freq_lo >= frq[i]) lb = i;
      if ((double)o.freq_hi > frq[i]) ub = i;
    }
    if (ub == -1 || ub >= Nsrc) ub = Nsrc - 1;
    if (lb < 0) lb = 0;
    if (ub < lb) { *why = "freqRange: the range selects no bin"; return SMILEHIP_ERR_INVALID; }
    h.lo = lb; h.hi = ub;
  }
  const int nBins = h.hi - h.lo + 1;
  // :771-840, :873-946
  for (int k = 0; k < b.n_bands + b.n_slopes; ++k) {
    const bool is_slope = k >= b.n_bands;
    const int lo = is_slope ? b.slope_lo[k - b.n_bands] : b.band_lo[k], hi = is_slope ? b.slope_hi[k - b.n_bands] : b.band_hi[k];
    if (lo < 0 || hi <= lo) { *why = is_slope ? "slopes: lower < upper, both >= 0" : "bands: lower < upper, both >= 0"; return SMILEHIP_ERR_INVALID; }
    double idxL, wghtL, idxR, wghtR;
    if (!axis) {
      idxL = (double)lo / F0;
      wghtL = std::ceil(idxL) - idxL;
      idxR = (double)hi / F0;
      wghtR = idxR - std::floor(idxR);
    } else {
      int ii;
      for (ii = 0; ii < Nsrc; ii++) if (frq[ii] > (double)lo) break;
      if ((ii < Nsrc) && (ii > 0)) wghtL = (frq[ii] - (double)lo) / (frq[ii] - frq[ii - 1]); else wghtL = 1.0;
      idxL = (double)ii - 1.0;
      if (idxL < 0) idxL = 0;
      if (idxL >= Nsrc) idxL = Nsrc;
      for (ii = 0; ii < Nsrc; ii++) if (frq[ii] >= (float)hi) break;
      if ((ii < Nsrc) && (ii > 0)) wghtR = ((double)hi - frq[ii - 1]) / (frq[ii] - frq[ii - 1]); else wghtR = 1.0;
      if ((ii < Nsrc) && (frq[ii] == (float)hi)) idxR = (double)ii; else idxR = (double)ii - 1.0;
      if (idxR >= Nsrc) idxR = Nsrc - 1;
    }
    if (wghtL == 0.0) wghtL = 1.0;
    if (wghtR == 0.0) wghtR = 1.0;
    long iL = (long)std::floor(idxL), iR = (long)std::floor(idxR);
    if (iL >= Nsrc) { iL = iR = Nsrc - 1; wghtR = 0.0; wghtL = 0.0; }
    if (iR >= Nsrc) { iR = Nsrc - 1; wghtR = 1.0; }
    if (iL < 0) iL = 0;
    if (iR < 0) iR = 0;
    if (iR < iL) { *why = is_slope ? "slopes: a band that lies between two bins of this spectrum" : "bands: a band that lies between two bins of this spectrum"; return SMILEHIP_ERR_INVALID; }
    h.iL[k] = (int32_t)iL; h.iR[k] = (int32_t)iR; h.wL[k] = wghtL; h.wR[k] = wghtR; h.Nind[k] = idxR - idxL;
  }
  // :995-1089: both walks end at the first bin above 5 kHz; f is the axis or the running sum f += F0
  {
    double f = 0.0;
    h.ar_n1 = h.hb_n1 = -1;
    int j;
    for (j = 0; j < Nsrc; j++) {
      const double fj = axis ? frq[j] : f;
      if (fj > 5000.0) break;
      if (!(fj < 1000.0) && h.ar_n1 < 0) h.ar_n1 = j;
      if (!(fj < 2000.0) && h.hb_n1 < 0) h.hb_n1 = j;
      f += F0;
    }
    h.ar_n2 = h.hb_n2 = j;
    if (h.ar_n1 < 0) h.ar_n1 = j;
    if (h.hb_n1 < 0) h.hb_n1 = j;
  }
  // the axes the kernel reads
  const bool ctr_group = b.centroid || b.standard_deviation || b.variance || b.skewness || b.kurtosis || b.slope;
  h.ax_m.assign((size_t)Nsrc, 0.0);
  h.ax_ro.assign((size_t)Nsrc, 0.0f);
  double f = 0.0;                                         // :1261, shared by the centroid and the sharpness weights
  if (axis) {
    for (int j = 0; j < Nsrc; ++j) { h.ax_m[j] = frq[j]; h.ax_ro[j] = (float)frq[j]; }
    h.ax_c = h.ax_m;
    h.ax_s = h.ax_m;
  } else {
    h.ax_c.assign((size_t)Nsrc, 0.0);
    h.ax_s.assign((size_t)Nsrc, 0.0);
    for (int j = 0; j < Nsrc; ++j) { h.ax_m[j] = (double)j * F0; h.ax_ro[j] = (float)j * (float)F0; h.ax_s[j] = (double)j; }
    if (ctr_group)
      for (int j = h.lo; j <= h.hi; ++j) { h.ax_c[j] = f; f += F0; }
  }
  // :1400-1418
  if (axis) {
    for (int i = h.lo; i <= h.hi; i++) { h.slope_S2f += frq[i] * frq[i]; h.slope_Sf += frq[i]; }
  } else {
    const double Nind = (double)nBins;
    const double NNm1 = Nind * (Nind - 1.0);
    const double S1 = NNm1 / (double)2.0;
    const double S2 = NNm1 * ((double)2.0 * Nind - (double)1.0) / (double)6.0;
    h.slope_Sf = S1 * F0;
    h.slope_S2f = S2 * F0 * F0;
  }
  // :1438-1468
  h.sharp.assign((size_t)nBins, 0.0);
  if (b.sharpness) {
    for (int j = h.lo; j <= h.hi; j++) {
      double fb;
      if (axis) {
        fb = frq[j];
        if (fs != SMILEHIP_SPECSCALE_BARK) {
          fb = specscale_inv(fb, fs, o.frq_scale_param);
          fb = specscale_fwd(fb, SMILEHIP_SPECSCALE_BARK, 0.0);
        }
      } else {
        fb = specscale_fwd(f, SMILEHIP_SPECSCALE_BARK, 0.0);
        f += F0;
      }
      const double w = sharpness_weight(fb);
      if (!std::isfinite(w)) { *why = "frq_scale: a sharpness weight is not finite on this axis"; return SMILEHIP_ERR_INVALID; }
      h.sharp[(size_t)(j - h.lo)] = w;
    }
  }
  return SMILEHIP_OK;
}

}  // namespace smilehip
