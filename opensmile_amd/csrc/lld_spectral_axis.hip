// R11 on any spectrum: cSpectral::processVector (src/lldcore/spectral.cpp:586-1555) with squareInput, useLogSpectrum / specFloor,
// normBandEnergies, alphaRatio, hammarbergIndex, freqRange, oldSlopeScale, buggyRollOff free and the level's own frequency axis
// (or none: the index-based branches), on K = 4 .. 2^20 bins: the one cSpectral operator for every option set but ComParE_2016's and
// GeMAPS' (their wave-parallel kernels: lld_blocks_compare.hpp / lld_gemaps.hip). What depends on the options and the axis alone comes
// from make_spectral_axis_tables (tables.cpp); the kernel reads it through wave-uniform addresses.
// One THREAD per frame, the frames of a launch side by side: every accumulator is the reference's own sequential chain (double, or
// FLOAT_DMEM where it has one), and each lane walks its own row of the matrix, deriving srcM / srcP / srcL of a bin (:661-716) where
// it reads it. A form that staged 64-frame x 32-bin tiles through LDS (coalesced row loads, the derivations once per bin and
// walk, padded columns) was built and measured on the same rows: 7 to 23 % slower on every option set timed
// (profiles/spectral_axis_timing.json), so this one stayed. The four sums of every slopes[] band live in LDS, a column per lane,
// sized by the number of bands. The spectrum is walked twice (three times for the entropy of a log spectrum, whose divisor is a
// second chain over the bins, smileUtil.c:2095-2104); an accumulator's order never depends on which walk it sits in.
#include <hip/hip_runtime.h>

#include "kernel_timing.hpp"
#include "lld_device.hpp"
#include "lld_stage.hpp"

namespace smilehip {
namespace {
// the four sums of slopes[] band b (Sf, S2f, sumA, sumB: :942-982), a column per lane: the first n_slopes x 4 x 64 doubles of the
// workgroup's dynamic LDS
__device__ __forceinline__ double &slope_sum(double *sl, const SpectralAxisDev &G, int q, int b) { return sl[(q * G.n_slopes + b) * 64 + threadIdx.x]; }
// srcP and srcL of one bin from the row itself (:677-716)
__device__ __forceinline__ float spectral_pow(const SpectralAxisDev &G, float x) { return G.square_input ? x * x : x; }
__device__ __forceinline__ float spectral_log(const SpectralAxisDev &G, float p) {
  return (p <= G.spec_floor) ? G.log_spec_floor : G.log_spec_factor * glibc_logf(p);
}

__device__ __forceinline__ float spectral_mag(const SpectralAxisDev &G, float x) {   // :661-676
  if (G.square_input) return x;
  return x > 0.0f ? sqrtf(x) : 0.0f;
}

// One bin's share of bands[B ..] (:843-847: the left edge bin weighted, the bins between, the right edge bin weighted) and of
// rollOff[I ..] (:1104-1118). The slots nest, every index a constant: the first unused slot ends the bin's tests. A loop over the
// sixteen slots tests each one for every bin, a fifth of the launch on avec2011's two bands and four points
// (profiles/spectral_one_operator_timing.json against ..._parent.json); one that leaves at the first unused slot is not unrolled, and
// its running index puts band[] and ro[] behind indexed register moves.
template <int B>
__device__ __forceinline__ void band_bin(const SpectralAxisDev &G, int j, float p, double (&band)[16]) {
  if constexpr (B < 16) {
    if (B >= G.n_bands) return;
    if (j == G.iL[B]) band[B] = (double)p * G.wL[B];
    else if (j > G.iL[B] && j < G.iR[B]) band[B] += (double)p;
    if (j == G.iR[B]) band[B] += (double)p * G.wR[B];
    band_bin<B + 1>(G, j, p, band);
  }
}
template <int I>
__device__ __forceinline__ void rolloff_bin(const SpectralAxisDev &G, int j, float p, double frameSum, double &sumC, float (&ro)[16]) {
  if constexpr (I < 16) {
    if (I >= G.n_rolloff) return;
    if (G.buggy_roll_off == 1 && I > 0) sumC += (double)p;
    if ((ro[I] == 0.0f) && (sumC >= G.rolloff[I] * frameSum)) ro[I] = G.ax_ro[j];
    rolloff_bin<I + 1>(G, j, p, frameSum, sumC, ro);
  }
}

}  // namespace

__global__ void __launch_bounds__(64) lld_spectral_axis(SpectralAxisDev G, const float *src, int64_t ld_src, const float *state, int first,
                                                       float *dst, int64_t ld_dst, int64_t n_frames) {
  extern __shared__ __attribute__((aligned(16))) double dyn_lds[];
  double *sl = dyn_lds;
  const int lane = threadIdx.x;
  const int64_t row0 = (int64_t)blockIdx.x * 64;
  const int64_t t = row0 + lane;
  if (t >= n_frames) return;
  const float *row = src + t * ld_src;
  const float *prow = t > 0 ? row - ld_src : (first ? row : state);   // the frame before (a first frame never looks at it)
  const bool have_prev = t > 0 || !first;
  const int K = G.K, lo = G.lo, hi = G.hi;
  const int nBins = hi - lo + 1;
  const bool use_log = G.use_log != 0;
  const bool flux_family = G.spec_pos_diff || G.spec_diff || G.flux || G.flux_centroid || G.flux_at_flux_centroid;
  // ---- first walk: every bin
  double frameSum = 0.0, sumL = 0.0, sumA = 0.0, fluxA = 0.0;   // :762-767, :1096-1098, :1262-1294, :1171-1176
  double fluxAf = 0.0, sdiff = 0.0, spdiff = 0.0;                // :1177-1189, :1143-1170
  double band[16];
  for (int b = 0; b < 16; ++b) band[b] = 0.0;
  for (int b = 0; b < G.n_slopes; ++b) { slope_sum(sl, G, 0, b) = 0.0; slope_sum(sl, G, 1, b) = 0.0; slope_sum(sl, G, 2, b) = 0.0; slope_sum(sl, G, 3, b) = 0.0; }
  float sum01 = 0.0f, sum15 = 0.0f, max02 = 0.0f, max25 = 0.0f; // :997-1022, :1041-1075: FLOAT_DMEM accumulators
  int maP = lo, miP = lo;
  float vmax = 0.0f, vmin = 0.0f, emin = 0.0f;                   // emin: smileStat_entropy's minimum (smileUtil.c:2087-2093)
  for (int j = 0; j < K; ++j) {
    const float x = row[j];
    const float m = spectral_mag(G, x), p = spectral_pow(G, x);   // srcM, srcP (:661-688)
    const float lp = use_log ? spectral_log(G, p) : p;         // srcLP (:689-721)
    band_bin<0>(G, j, p, band);
    if (G.n_slopes > 0) {
      const double a = G.ax_s[j];                              // frq[j], or j itself where there is no axis (:964-978)
      for (int b = 0; b < G.n_slopes; ++b) {
        const int iL = G.iL[16 + b], iR = G.iR[16 + b];
        const double wL = G.wL[16 + b], wR = G.wR[16 + b];
        if (j < iL || j > iR) continue;                         // (wave-uniform: most bins touch no slope band)
        double Sf = slope_sum(sl, G, 0, b), S2f = slope_sum(sl, G, 1, b), A = slope_sum(sl, G, 2, b), B = slope_sum(sl, G, 3, b);
        if (j == iL) {
          Sf = a * wL;
          S2f = Sf * Sf;
          A = a * wL * (double)lp;
          B = wL * (double)lp;
        } else if (j < iR && G.has_axis) {                     // (without an axis nScale is 0 and `ii < nScale` ends the loop at once, :969)
          S2f += a * a;
          Sf += a;
          A += a * (double)lp;
          B += (double)lp;
        }
        if (j == iR) {
          S2f += a * wR * a * wR;
          Sf += a * wR;
          A += a * wR * (double)lp;
          B += wR * (double)lp;
        }
        slope_sum(sl, G, 0, b) = Sf; slope_sum(sl, G, 1, b) = S2f; slope_sum(sl, G, 2, b) = A; slope_sum(sl, G, 3, b) = B;
      }
    }
    if (G.alpha_ratio) {
      if (j < G.ar_n1) sum01 += p;
      else if (j < G.ar_n2) sum15 += p;
    }
    if (G.hammarberg) {
      if (j < G.hb_n1) { if (p > max02) max02 = p; }
      else if (j < G.hb_n2) { if (p > max25) max25 = p; }
    }
    if (j >= lo && j <= hi) {
      frameSum += (double)p;
      if (use_log) sumL += (double)lp;
      sumA += G.ax_c[j] * (double)lp;
      if (lp < emin) emin = lp;
      if (have_prev && flux_family) {
        const float pm = spectral_mag(G, prow[j]);
        const double d = ((double)m / 1.0 - (double)pm / 1.0);
        if (G.flux || G.flux_centroid) fluxA += d * d;
        if (G.flux_centroid) fluxAf += d * d * G.ax_m[j];
        if (G.spec_diff || G.spec_pos_diff) {                  // (the reference subtracts the two FLOAT_DMEM values as floats here)
          const double myd = (double)(m - pm);
          if (G.spec_diff) sdiff += myd * myd;
          if (G.spec_pos_diff && myd > 0.0) spdiff += myd * myd;
        }
      }
      if (j == lo) { vmax = lp; vmin = lp; }                   // :1314-1322 (the last bin is not looked at)
      else if (j < hi) {
        if (lp < vmin) { vmin = lp; miP = j; }
        if (lp > vmax) { vmax = lp; maP = j; }
      }
    }
  }
  float *o = dst + t * ld_dst;
  int n = 0;
  const double sumB = use_log ? sumL : frameSum;                // :1092-1099 (the same chain over srcP with and without normBandEnergies)
  {
#pragma unroll
    for (int b = 0; b < 16; ++b) {                               // :849-868
      if (b >= G.n_bands) continue;
      if (G.norm_band) o[n++] = (frameSum > 0.0) ? (float)(band[b] / frameSum) : 0.0f;
      else if (use_log) o[n++] = (float)(10.0 * log_d(band[b] / (double)nBins) / G.ln10);
      else o[n++] = (float)(band[b] / (double)nBins);
    }
    for (int b = 0; b < G.n_slopes; ++b) {                       // :979-991
      double Sf = slope_sum(sl, G, 0, b), S2f = slope_sum(sl, G, 1, b), A = slope_sum(sl, G, 2, b);
      if (!G.has_axis) { S2f *= G.F0 * G.F0; Sf *= G.F0; A *= G.F0; }
      const double Nind = G.Nind[16 + b];
      const double deno = (Nind * S2f - Sf * Sf);
      double slope = 0.0;
      if (deno != 0.0) slope = (Nind * A - Sf * slope_sum(sl, G, 3, b)) / deno;
      o[n++] = G.old_slope_scale ? (float)(slope * (Nind - 1.0)) : (float)slope;
    }
    if (G.alpha_ratio) {                                         // :1024-1036
      float a = 0.0f;
      if (sum01 > 0.0f) {
        if (!use_log) a = sum15 / sum01;
        else if (sum15 > G.spec_floor) a = (float)(10.0 * (double)glibc_logf(sum15 / sum01) / G.ln10);
        else a = (float)(10.0 * (double)(glibc_logf(G.spec_floor) - glibc_logf(sum01)) / G.ln10);
      }
      o[n++] = a;
    }
    if (G.hammarberg) {                                          // :1076-1088
      float h = 0.0f;
      if (max25 > 0.0f) {
        if (!use_log) h = max02 / max25;
        else if (max02 > G.spec_floor) h = (float)(10.0 * (double)glibc_logf(max02 / max25) / G.ln10);
        else h = (float)(10.0 * (double)(glibc_logf(G.spec_floor) - glibc_logf(max25)) / G.ln10);
      }
      o[n++] = h;
    }
  }
  float ctr = 0.0f;
  const bool need_ctr = G.centroid || G.standard_deviation || G.variance || G.skewness || G.kurtosis || G.slope;
  if (need_ctr && sumB != 0.0) ctr = (float)(sumA / sumB);       // :1302-1304
  // ---- the entropy's divisor on a spectrum with negative values (smileUtil.c:2095-2110)
  const double entropy_floor = 0.0000001;
  double dn = sumB;
  if (G.entropy && emin < 0.0f) {
    const double mf = entropy_floor + (double)emin;
    for (int j = lo; j <= hi; ++j) {
      const float p = spectral_pow(G, row[j]);
      const float lp = use_log ? spectral_log(G, p) : p;
      if ((double)lp <= mf) dn += mf - (double)lp;
      dn -= (double)emin;
    }
  }
  if (dn < (float)entropy_floor) dn = (float)entropy_floor;
  // ---- second walk: bins lo .. hi
  float ro[16];
  for (int i = 0; i < 16; ++i) ro[i] = 0.0f;
  double sumC = 0.0, ent = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
  float sumAA = 0.0f, ptpSum = 0.0f, lastPeak = -99.0f, gmean = 0.0f;
  int nGm = 0;
  const double l2 = log(2.0);
  const double u = ctr;
  float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f, h3 = 0.0f, h4 = 0.0f;   // srcLP of bins j-4 .. j: the harmonicity's window around bin j-2
  for (int j = lo; j <= hi; ++j) {
    const float p = spectral_pow(G, row[j]);
    const float lp = use_log ? spectral_log(G, p) : p;
    sumC += (double)p;                                         // :1104-1118
    rolloff_bin<0>(G, j, p, frameSum, sumC, ro);
    if (G.entropy) {                                           // smileUtil.c:2112-2122
      double v = lp - emin;
      if (v <= entropy_floor) v = entropy_floor;
      const double ln = v / dn;
      if (ln > 0.0) ent += ln * log_d(ln) / l2;
    }
    if (G.standard_deviation || G.variance || G.skewness || G.kurtosis) {   // :1344-1364
      const double t1 = (G.ax_m[j] - u);
      double mm = t1 * t1 * (double)lp;
      m2 += mm; mm *= t1; m3 += mm; m4 += mm * t1;
    }
    if (G.sharpness) sumAA += (float)(G.sharp_w[j - lo] * (double)p);       // :1455-1457 / :1469-1471
    if (G.harmonicity) {                                       // :1485-1498, the test of bin j-2 once bin j is known
      h0 = h1; h1 = h2; h2 = h3; h3 = h4; h4 = lp;
      const int q = j - 2;
      if (q >= lo + 2 && q < hi - 1) {
        if ((h0 < h2 && h1 < h2 && h2 > h3 && h2 > h4) || (h0 > h2 && h1 > h2 && h2 < h3 && h2 < h4)) {
          if (lastPeak != -99.0f) ptpSum += fabsf(h2 - lastPeak);
          lastPeak = h2;
        }
      }
    }
    if (G.flatness && sumB != 0.0 && lp != 0.0f) { gmean += glibc_logf(fabsf(lp)); nGm++; }   // :1519-1526: log() on a FLOAT_DMEM is logf
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) if (i < G.n_rolloff) o[n++] = ro[i];
  if (flux_family) {                                             // :1124-1254
    if (!have_prev) o[n++] = 0.0f;                               // a field's first frame: ONE zero for the whole family (:1135)
    else {
      const double nR = (double)(hi - lo + 1);
      if (G.spec_diff) { const double d = sdiff / nR; o[n++] = (d > 0.0) ? (float)sqrt(d) : 0.0f; }
      if (G.spec_pos_diff) { const double d = spdiff / nR; o[n++] = (d > 0.0) ? (float)sqrt(d) : 0.0f; }
      if (G.flux) {
        const double flux = (nBins > 0) ? fluxA / (double)nBins : 0.0;
        o[n++] = (flux > 0.0) ? (float)sqrt(flux) : 0.0f;
      }
      if (G.flux_centroid || G.flux_at_flux_centroid) {
        const double fluxCentr = (fluxA > 0.0) ? fluxAf / fluxA : 0.0;
        if (G.flux_centroid) o[n++] = (float)fluxCentr;
        if (G.flux_at_flux_centroid) {                           // :1209-1247: the flux of the five bins around the centroid's bin
          const float *prev = prow;
          int bin = hi;
          for (int j = lo; j <= hi; ++j) if (G.ax_m[j] >= fluxCentr) { bin = j; break; }
          int start = bin - 2, end = bin + 2;
          if (start < lo) start = lo;
          if (end > hi) end = hi;
          double myF = 0.0;
          for (int j = start; j <= end; ++j) {
            const double d = ((double)spectral_mag(G, row[j]) / 1.0 - (double)spectral_mag(G, prev[j]) / 1.0);
            myF += d * d;
          }
          if (end - start + 1 > 0) myF /= (double)(end - start + 1); else myF = 0.0;
          o[n++] = (float)myF;
        }
      }
    }
  }
  if (G.centroid) o[n++] = ctr;
  if (G.max_pos) o[n++] = (float)G.ax_m[maP];                    // :1323-1329
  if (G.min_pos) o[n++] = (float)G.ax_m[miP];
  if (G.entropy) o[n++] = (float)(-ent);
  if (G.standard_deviation || G.variance || G.skewness || G.kurtosis) {
    const double sigma2 = (sumB != 0.0) ? m2 / sumB : 0.0;
    if (G.standard_deviation) o[n++] = (sigma2 > 0.0) ? (float)sqrt(sigma2) : 0.0f;
    if (G.variance) o[n++] = (float)sigma2;
    if (G.skewness) o[n++] = (sigma2 <= 0.0) ? 0.0f : (float)(m3 / (sumB * sigma2 * sqrt(sigma2)));
    if (G.kurtosis) o[n++] = (sigma2 == 0.0) ? 0.0f : (float)(m4 / (sumB * sigma2 * sigma2));
  }
  if (G.slope) {                                                 // :1399-1427
    const double Nind = (double)nBins;
    const double deno = (Nind * G.slope_S2f - G.slope_Sf * G.slope_Sf);
    double slope = 0.0;
    if (deno != 0.0) slope = (Nind * sumA - G.slope_Sf * sumB) / deno;
    o[n++] = G.old_slope_scale ? (float)(slope * (Nind - 1.0)) : (float)slope;
  }
  if (G.sharpness) {
    float c2 = 0.0f;
    if (frameSum != 0.0) c2 = (float)(sumAA / frameSum);
    o[n++] = (float)(0.11 * c2);
  }
  if (G.harmonicity) {                                           // :1499-1512
    ptpSum /= 2.0;
    if (G.norm_band && sumB != 0.0) {
      if (use_log) ptpSum /= (float)fabs(sumB);
      else ptpSum /= (float)(frameSum);
    } else {
      ptpSum /= (float)nBins;
    }
    o[n++] = ptpSum;
  }
  if (G.flatness) {                                              // :1515-1543: the geometric mean over the arithmetic one
    float sf = 0.0f;
    if (sumB != 0.0) {
      if (nGm > 0) gmean /= (float)nGm;
      gmean = glibc_expf(gmean);
      sf = gmean / (float)fabs(sumB / (double)nBins);
    }
    o[n++] = G.log_flatness ? ((sf > 0.0f) ? glibc_logf(sf) : 0.0f) : sf;
  }
  while (n < G.n_out) o[n++] = 0.0f;                             // (a field's first frame with more than one of the flux family on: the
                                                                 // reference's vector keeps its calloc'd zeros in the last slots)
}

// the last frame's row becomes the stream's state (the next launch's flux)
__global__ void lld_spectral_axis_keep(const float *row, float *state, int K) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < K) state[i] = row[i];
}

hipError_t stage_spectral_axis(const SpectralAxisDev &G, const float *src, int64_t ld_src, float *state, int first, float *dst,
                               int64_t ld_dst, int64_t n_frames, hipStream_t s) {
  if (n_frames <= 0) return hipSuccess;
  const size_t sl_bytes = (size_t)G.n_slopes * 4 * 64 * sizeof(double);
  SMILEHIP_KLAUNCH(lld_spectral_axis, dim3((unsigned)((n_frames + 63) / 64)), dim3(64), sl_bytes, s, G, src, ld_src, state, first, dst, ld_dst,
                   n_frames);
  if ((G.flux || G.spec_diff || G.spec_pos_diff || G.flux_centroid || G.flux_at_flux_centroid) && state)
    SMILEHIP_KLAUNCH(lld_spectral_axis_keep, dim3((unsigned)((G.K + 255) / 256)), dim3(256), 0, s, src + (n_frames - 1) * ld_src, state, G.K);
  return hipGetLastError();
}

}  // namespace smilehip
