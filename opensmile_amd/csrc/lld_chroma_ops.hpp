// config/chroma/chroma_fft.conf behind cFFTmagphase: cTonespec (src/lld/tonespec.cpp) and cChroma (src/lld/chroma.cpp) as row
// functions. __host__ __device__ like lld_prosody_acf_ops.hpp: tests/test_chroma_fft_host.py compiles this header and the table
// builder (chroma_tables.cpp) with g++ (tests/helpers/chroma_check.cpp) and holds them to the real binary's levels bit for bit
// without a GPU; lld_chroma.hip calls the very same functions from the fused frame kernel and from the two operators.
//
// What the two components do per frame, as read in their source and measured against the binary
// (tests/golden/make_golden_chroma_fft.py):
//  * [tonespec:cTonespec] processVector (tonespec.cpp:390-441): with usePower the magnitudes are squared into a float copy
//    (:405-412); bins firstBin .. lastBin whose key is 1 .. nNotes add src[i] * filterMap[i] -- the product rounded to float --
//    to their note's float accumulator in bin order (:418-422); a note with pitchClassNbins > 0 is divided by (float)nbins and,
//    with usePower, replaced by its float square root (0 if it is not >= 0), a note without bins is 0 (:424-434). binKey is
//    monotone (computeFilters' walk, :210-227), so a note's bins are one run: the tables hold, per note, the run's first bin,
//    its length and nbins (which is the run's length: both are counted over firstBin .. lastBin, :254-258).
//  * [chroma:cChroma] processVector (chroma.cpp:86-118): class i is the float sum of src[j * octaveSize + i] over the octaves j in
//    order, starting from 0; sum is a double that takes the classes in order; silFlag is set by any class sum < silThresh
//    (a float, :71); the output is dst[i] / (float)sum, or zeros if sum == 0 or the flag is set.
//  * [framer:cFramer] with noPostEOIprocessing = 1 writes (n - N) / H + 1 frames for n >= N samples, none below, and every level
//    behind it holds as many: rows_of.
// No operation here may be contracted into a fused multiply-add (the library is built with -ffp-contract=off; the helper too).
#pragma once
#include <cstdint>

#include "glibc_float.hpp"

#if defined(__HIPCC__)
#define CHROMA_SQRTF(x) sqrtf(x)
#else
#include <cmath>
#define CHROMA_SQRTF(x) std::sqrt((float)(x))
#endif

namespace smilehip {
namespace chroma {

constexpr int kMaxNotes = 120;       // nOctaves <= 10
constexpr int kMaxOctaveSize = 64;   // one lane per class in the fused kernel

// per note: the run of bins it sums (first, count) and pitchClassNbins as the divisor; one 16-byte record
struct NoteRec {
  int32_t first, count, nbins, reserved;
};

// rows of every level behind the framer for an utterance of n_samples samples (frame N, step H)
GLF_HD int64_t rows_of(int64_t n_samples, int64_t N, int64_t H) { return n_samples >= N ? (n_samples - N) / H + 1 : 0; }

// one note of cTonespec's output: src = the frame's magnitudes, fmap = filterMap (dbA folded in), r = the note's record
GLF_HD float tonespec_note(const float *src, const float *fmap, const NoteRec &r, int use_power) {
  float acc = 0.0f;
  for (int i = r.first; i < r.first + r.count; ++i) {
    const float s = src[i];
    const float v = use_power ? s * s : s;
    const float t = v * fmap[i];
    acc += t;
  }
  if (r.nbins <= 0) return 0.0f;
  acc = acc / (float)r.nbins;
  if (use_power) acc = (acc >= 0.0f) ? CHROMA_SQRTF(acc) : 0.0f;
  return acc;
}

// a frame of the tonespec level: n_notes values
GLF_HD void tonespec_row(const float *src, const float *fmap, const NoteRec *rec, int n_notes, int use_power, float *dst) {
  for (int k = 0; k < n_notes; ++k) dst[k] = tonespec_note(src, fmap, rec[k], use_power);
}

// class i of cChroma before the normalisation: the octaves in order
GLF_HD float chroma_class(const float *ts, int n_octaves, int octave_size, int i) {
  float d = 0.0f;
  for (int j = 0; j < n_octaves; ++j) d += ts[j * octave_size + i];
  return d;
}

// a frame of the chroma level: octave_size values from n_src = n_octaves * octave_size tonespec values
GLF_HD void chroma_row(const float *ts, int n_src, int octave_size, float sil_thresh, float *dst) {
  const int n_octaves = n_src / octave_size;
  double sum = 0.0;
  int sil = 0;
  for (int i = 0; i < octave_size; ++i) {
    const float d = chroma_class(ts, n_octaves, octave_size, i);
    if (d < sil_thresh) sil = 1;
    sum += (double)d;
    dst[i] = d;
  }
  const bool keep = sum != 0.0 && !sil;
  const float fs = (float)sum;
  for (int i = 0; i < octave_size; ++i) dst[i] = keep ? dst[i] / fs : 0.0f;
}

}  // namespace chroma
}  // namespace smilehip
