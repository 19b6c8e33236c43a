// config/spectrum/spectrogram.conf (SMILEHIP_CHAIN_SPECTROGRAM) as row functions: the row count behind the framer and one output cell
// of cFFTmagphase in each of the five forms the component has. __host__ __device__ like lld_audspec_ops.hpp:
// tests/test_spectrogram_host.py compiles this header with g++ (tests/helpers/spectrogram_check.cpp) and holds it to the real binary's
// levels bit for bit without a GPU; lld_spectrogram.hip calls the very same functions from both forms of the frame kernel.
//
// What the components do per frame, as read in their source and measured against the binary (tests/golden/make_golden_spectrogram.py):
//  * [frame:cFramer] frameMode = fixed, frameCenterSpecial = left writes (n - N) / H + 1 frames for n >= N samples, none below
//    (measured at 0, N - 1, N, N + H - 1 and N + H samples); row t carries the time t * frameStep: rows_of.
//  * [win:cWindower] (windower.cpp:204-218): x[n] * win[n] + offset; there is no pre-emphasis.
//  * [fft:cTransformFFT] zero-pads to the next power of two, symmetrically by default (transformFft.cpp:35).
//  * [fftmag:cFFTmagphase] (fftmagphase.cpp:215-255), Nsrc = the transform length, fN = (FLOAT_DMEM)Nsrc:
//      magnitude                      |re| at the two edge bins, sqrt(re re + im im) between them
//      normalise                      ((FLOAT_DMEM)1.0 / fN) times that
//      power                          the edge bins' |re| squared, re re + im im between them
//      normalise + power              the edge bins' ((1 / fN) |re|) squared (bin 0 without the fabs: the same square),
//                                     ((FLOAT_DMEM)1.0 / (fN fN)) (re re + im im) between them
//      dBpsd (implies normalise)      MAX(mindBp, dBpnorm + 20 log10((1 / fN) |re|)) at the edges, MAX(mindBp, dBpnorm +
//                                     10 log10((1 / (fN fN)) (re re + im im))) between them; MAX(a, b) is ((a) > (b)) ? (a) : (b)
//                                     (smileUtil.h:44), so a NaN value passes through. log10 on FLOAT_DMEM is log10f.
//    mindBp is raised to dBpnorm - 120 when it lies below that (:95-97), both kept as FLOAT_DMEM: clamp_min_dbp.
// No operation here may be contracted into a fused multiply-add (the library is built with -ffp-contract=off; the helper too).
#pragma once
#include <cmath>
#include <cstdint>

#include "glibc_float.hpp"

namespace smilehip {
namespace spectrogram {

enum Form : int32_t { kMagnitude = 0, kSpecDens = 1, kPowSpec = 2, kPowSpecDens = 3, kDbPsd = 4 };

// the constants of one plan's form: what cFFTmagphase::myFetchConfig and processVector build before the bin loop
struct FormConsts {
  int32_t form;        // Form
  float inv_n;         // (FLOAT_DMEM)1.0 / (FLOAT_DMEM)Nsrc
  float inv_n2;        // (FLOAT_DMEM)1.0 / ((FLOAT_DMEM)Nsrc * (FLOAT_DMEM)Nsrc)
  float dbp_norm;
  float min_dbp;       // behind the clamp
};

// rows of the level lld for an utterance of n_samples samples (frame N, step H)
GLF_HD int64_t rows_of(int64_t n_samples, int64_t N, int64_t H) { return n_samples >= N ? (n_samples - N) / H + 1 : 0; }

// cFFTmagphase::myFetchConfig (:93-97)
GLF_HD float clamp_min_dbp(float dbp_norm, float min_dbp) {
  if (min_dbp - dbp_norm < -120.0) min_dbp = -120 + dbp_norm;
  return min_dbp;
}

// the MAGPHASE flag bits (1 magnitude, 4 normalise, 8 power, 16 dBpsd) as a form; -1: a set without magnitude or with other bits.
// dBpsd wins over normalise and power, as the component's branches are ordered (:215-248).
GLF_HD int form_of_flags(int32_t flags) {
  if (!(flags & 1) || (flags & ~(1 | 4 | 8 | 16))) return -1;
  if (flags & 16) return kDbPsd;
  return (flags & 4) ? ((flags & 8) ? kPowSpecDens : kSpecDens) : ((flags & 8) ? kPowSpec : kMagnitude);
}

GLF_HD FormConsts form_consts(int form, int64_t Nfft, float dbp_norm, float min_dbp) {
  FormConsts F;
  const float fN = (float)Nfft;
  F.form = form;
  F.inv_n = (float)1.0 / fN;
  F.inv_n2 = (float)1.0 / (fN * fN);
  F.dbp_norm = dbp_norm;
  F.min_dbp = clamp_min_dbp(dbp_norm, min_dbp);
  return F;
}

// one output cell: (re, im) of the bin (im is not read at the two edge bins, whose value the transform packs into re)
template <int FORM>
GLF_HD float bin_value_form(float re, float im, bool edge, const FormConsts &F) {
  const float a = __builtin_fabsf(re), p = re * re + im * im;
  if (FORM == kMagnitude) return edge ? a : sqrtf(p);
  if (FORM == kSpecDens) return F.inv_n * (edge ? a : sqrtf(p));
  if (FORM == kPowSpec) return edge ? a * a : p;
  if (FORM == kPowSpecDens) {
    const float e = F.inv_n * a;
    return edge ? e * e : F.inv_n2 * p;
  }
  const float v = edge ? F.dbp_norm + (float)20.0 * glibc_log10f(F.inv_n * a) : F.dbp_norm + (float)10.0 * glibc_log10f(F.inv_n2 * p);
  return F.min_dbp > v ? F.min_dbp : v;                    // MAX(mindBp, v): a NaN v passes through
}
GLF_HD float bin_value(float re, float im, bool edge, const FormConsts &F) {
  switch (F.form) {
    case kSpecDens: return bin_value_form<kSpecDens>(re, im, edge, F);
    case kPowSpec: return bin_value_form<kPowSpec>(re, im, edge, F);
    case kPowSpecDens: return bin_value_form<kPowSpecDens>(re, im, edge, F);
    case kDbPsd: return bin_value_form<kDbPsd>(re, im, edge, F);
    default: return bin_value_form<kMagnitude>(re, im, edge, F);
  }
}

// a frame of the level lld from a frame of the level fft (cTransformFFT's packing: re0, reM, re1, im1, ...)
GLF_HD void spectrum_row(const float *fft, int64_t Nfft, const FormConsts &F, float *dst) {
  const int64_t M = Nfft / 2;
  dst[0] = bin_value(fft[0], 0.0f, true, F);
  for (int64_t k = 1; k < M; ++k) dst[k] = bin_value(fft[2 * k], fft[2 * k + 1], false, F);
  dst[M] = bin_value(fft[1], 0.0f, true, F);
}

}  // namespace spectrogram
}  // namespace smilehip
