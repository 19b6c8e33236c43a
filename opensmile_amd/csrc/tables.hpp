// Host-side table generation for the LLD chain (product code; independent of
// oracle/). Every table is computed with the reference's own precision
// recipe -- double math, one rounding to float where the reference rounds --
// so that the device kernels consume bit-identical constants.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/smilehip.h"

namespace smilehip {

struct Geometry {
  int64_t N = 0, H = 0, Nfft = 0, K = 0;
  double period = 0.0;          // sample period T = 1/fs
  double frame_period = 0.0;    // H*T as the framer's level period (= frameStep)
  double fft_frame_size_sec = 0.0;
};

struct MelBank {
  int n_bands = 0;
  int64_t nLo = 0, nHi = 0;
  std::vector<float> coef;        // one weight per bin (falling slope of band chan[n])
  std::vector<int32_t> chan;      // band index of the falling slope, -3 = unused bin
  std::vector<float> centres;     // n_bands+2 band edges/centres on the mel axis
  // per-band bin ranges derived from chan[] (device-side iteration order):
  // band b sums bins [rise_lo[b], rise_hi[b]) with (p - p*w) then
  // [fall_lo[b], fall_hi[b]) with p*w -- the reference's bin-ascending order.
  std::vector<int32_t> rise_lo, rise_hi, fall_lo, fall_hi;
  float scale = 1.0f;             // HTK sample-value scaling applied after the sums
};

struct DctTables {
  int n_bands = 0, first = 0, last = 0, n_mfcc = 0;
  std::vector<float> cos_rows;    // n_mfcc rows of n_bands, row r = OUTPUT position r
  std::vector<float> gain;        // per output position: lifter * sqrt(2/nB) (one float product)
  std::vector<float> lifter;      // raw lifter table (sintable), reference order
  float melfloor = 0.0f, log_floor = 0.0f;
};

// ComParE / GeMAPS F0 group: cSpecScale (scale=octave, interpMethod=spline, specSmooth=specEnhance=
// auditoryWeighting=1, minF=25, maxF=-1, nPointsTarget=0) and cPitchShs constants for one spectrum geometry
struct F0Host {
  std::vector<double> sp_rec, sp_d1, sp_d2, ip_co, audw;
  std::vector<int32_t> ip_k;
  std::vector<double> ip_rec;     // [K x 4] a, c, d, auditory weight of target point i: one 32-byte record (lld_f0_sweep)
  std::vector<int32_t> ip_cnt;    // [ceil(K / 16) x 16] target points whose lower source bin is k (ip_k is non-decreasing: they are consecutive)
  std::vector<double> sw_rec;     // [K x 8] sigma, p, dec, d1, RN(1 / d1), d2, RN(1 / d2), 0
  int32_t n_harm = 15;
  int32_t shift[16] = {0};
  float scale[16] = {0};
  float Fmint = 0.f, Fstept = 0.f;
  double log_base = 0.0;
};
// K bins of a spectrum level whose frameSizeSec is fft_frame_size_sec; 0 on success
int  make_f0_tables(int64_t K, double fft_frame_size_sec, int n_harmonics, float compression, double min_f, F0Host &h);

// cSpecScale on any target scale (log / semitone / bark / bao / mel / linear), any number of target points and an explicit maxF:
// the source axis, smileMath_cspline_init's and smileMath_csplint_init's caches and the data-independent half of
// smileMath_cspline's recurrences, as lld_specscale.hip reads them
struct SpecScaleHost {
  int32_t n_src = 0, n_tgt = 0;
  int32_t weighting = 0;          // the auditory weighting survives myFetchConfig (log scale with base exactly 2)
  double min_f = 0.0, max_f = 0.0, fmin_t = 0.0, fmax_t = 0.0;
  std::vector<double> f_t;        // [n_src] the source bins on the target axis
  std::vector<double> spline;     // [n_src x 5] sigma, diff1, diff2, p = 1 / (sigma y2[i-1] + 2), y2[i] of the forward sweep (bins 1 .. n_src-2)
  std::vector<int32_t> ip_k;      // [n_tgt] lower source bin of target point i (non-decreasing)
  std::vector<double> ip_rec;     // [n_tgt x 4] a, c, d, auditory weight (1 where the weighting is off)
};
// n_src bins of a spectrum level whose frameSizeSec is frame_size_sec; 0 on success, otherwise `why` names the cause
int  make_specscale_tables(const smilehip_specscale_opts &o, int64_t n_src, double frame_size_sec, SpecScaleHost &h, const char **why);

// cSpectral on any spectrum (smilehip_spectral_axis_opts): everything of cSpectral::processVector (src/lldcore/spectral.cpp:586-1555)
// that depends on the options and the frequency axis alone, restated in double
struct SpectralAxisHost {
  int32_t K = 0, n_out = 0, has_axis = 0;
  int32_t lo = 0, hi = 0;                                 // specRangeLowerBin / specRangeUpperBin (:625-647)
  int32_t ar_n1 = 0, ar_n2 = 0, hb_n1 = 0, hb_n2 = 0;     // alpha ratio: bins [0, n1) below 1 kHz, [n1, n2) up to 5 kHz; Hammarberg: 2 kHz (:995-1089)
  int32_t iL[32] = {0}, iR[32] = {0};                     // bands[], then slopes[]: edge bins, weights, idxR - idxL (:771-840, :873-946)
  double wL[32] = {0}, wR[32] = {0}, Nind[32] = {0};
  double slope_Sf = 0.0, slope_S2f = 0.0;                 // :1400-1418
  float spec_floor = 0.0f, log_spec_floor = 0.0f, log_spec_factor = 0.0f;   // :85-91, :228-237, :690
  std::vector<double> ax_c, ax_m, ax_s;                   // [K] the axis the centroid (:1263-1299), the moments / flux centroid / extremes and the slopes[] read
  std::vector<float> ax_ro;                               // [K] a roll-off point's value (:1110-1116)
  std::vector<double> sharp;                              // [hi - lo + 1] (:1438-1468)
};
// K bins of a level whose frameSizeSec is frame_size_sec; frq / n_scale: the level's axis or (nullptr, 0); 0 on success, otherwise
// `why` names the option
int  make_spectral_axis_tables(const smilehip_spectral_axis_opts &o, int64_t K, double frame_size_sec, const double *frq, int64_t n_scale,
                               SpectralAxisHost &h, const char **why);

int  make_geometry(const smilehip_lld_config &c, Geometry &g);
int  make_window(const smilehip_lld_config &c, int64_t N, std::vector<float> &w);
int  make_mel(const smilehip_lld_config &c, const Geometry &g, MelBank &m);
int  make_dct(const smilehip_lld_config &c, DctTables &d);
float delta_norm(int W);

}  // namespace smilehip
