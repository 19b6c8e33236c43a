// config/chroma/chroma_filt.conf in front of cChroma: cTonefilt (src/lld/tonefilt.cpp), a bank of decaying sine / cosine
// correlators run over the samples themselves, as row functions. __host__ __device__ like lld_chroma_ops.hpp:
// tests/test_chroma_filt_host.py compiles this header and tonefilt_tables.cpp with g++ (tests/helpers/tonefilt_check.cpp) and holds
// them to the real binary's levels bit for bit without a GPU; lld_tonefilt.hip calls the very same functions.
//
// What the component does, as read in its source and measured against the binary (tests/golden/make_golden_chroma_filt.py):
//  * configureWriter (tonefilt.cpp:106-130): P = (long)round(outputPeriod / T) samples per block, T = the wave level's period
//    1.0 / (double)sampleRate (waveSource.cpp:190); outputPeriod < T gives P = 1. The reader takes blocks of P samples, step P:
//    block_len. At the end of input the reader hands out one more block if samples are left over: those samples, then the LAST
//    SAMPLE REPEATED up to P (cDataMemoryLevel::getMatrix pads with the last frame, dataMemoryLevel.cpp:1698-1708), and doFilter
//    runs over all P. An utterance of n samples so gives ceil(n / P) rows, as measured on 0, 1, P - 1, P, P + 1, 2P - 1, 2P, 2P + 1
//    samples, and sample index k >= n reads x[n - 1]: rows_of, padded_index.
//  * setupNewNames (:180-189), all in double: freq[n] = firstNote * pow(2.0, n / 12.0),
//    decayF[n] = decayFN + (decayF0 - decayFN) * (freq[n] - freq[0]) / freq[nNotes - 1], with the clamps of myFetchConfig (:73-90):
//    make_tonefilt_tables (tonefilt_tables.cpp).
//  * doFilter (:204-226) per note and per sample n of a block that starts at sample pos, state s, c in double over the whole input:
//        time = (double)(pos + n) * inputPeriod
//        s = decayF * s + (1.0 - decayF) * sin(2.0 * M_PI * f * time) * (double)x[n]
//        c = decayF * c + (1.0 - decayF) * cos(2.0 * M_PI * f * time) * (double)x[n]
//    left to right, every product and sum rounded on its own: step. At the end of the block y = (float)sqrt(c * c + s * s), then
//    y *= 10.0, a float times a double constant rounded to float: emit.
// The trigonometric function is a template parameter: the host build passes LibmSinCos -- the C library's sin and cos, what the
// binary calls, so the host rows are the binary's bit for bit --, the device passes DevSinCos (sincos_d, lld_sincos_d.hpp): double
// states that are not the binary's bits, float rows that are (README "Parity").
// None of the reference's own expressions may be contracted into a fused multiply-add (-ffp-contract=off; the helper too).
#pragma once
#include <cstdint>

#include "glibc_float.hpp"
#include "lld_sincos_d.hpp"

#if !defined(__HIPCC__)
#include <cmath>
#endif

namespace smilehip {
namespace tonefilt {

constexpr int kMaxNotes = 120;       // the tonespec level's width limit (chroma::kMaxNotes)
constexpr double kTwoPi = 2.0 * 3.14159265358979323846;   // 2.0 * M_PI

// per note: what doFilter reads, 32 bytes
struct NoteTab {
  double w;      // 2.0 * M_PI * freq (the first product of the argument, left to right)
  double decay;  // decayF
  double gain;   // 1.0 - decayF
  double freq;
};

struct State {
  double s, c;
};

struct DevSinCos {
  GLF_HD SinCosD operator()(double x) const { return sincos_d(x); }
};
#if !defined(__HIPCC__)
struct LibmSinCos {
  SinCosD operator()(double x) const {
    volatile double vx = x;          // the C library's functions on a run-time operand
    SinCosD o;
    o.s = std::sin(vx);
    o.c = std::cos(vx);
    return o;
  }
};
#endif

// the wave level's period (waveSource.cpp:190) and the block length (tonefilt.cpp:106-125)
GLF_HD double input_period(double sample_rate) { return 1.0 / (double)(long)sample_rate; }
GLF_HD int64_t block_len(double sample_rate, double output_period) {
  const double T = input_period(sample_rate);
  if (!(output_period > 0.0)) output_period = 0.1;         // myFetchConfig (:70)
  if (output_period < T) return 1;
  const int64_t P = (int64_t)__builtin_round(output_period / T);
  return P < 0 ? 0 : P;
}
// rows of the tonespec and chroma levels for an utterance of n samples
GLF_HD int64_t rows_of(int64_t n_samples, int64_t P) { return P > 0 && n_samples > 0 ? (n_samples + P - 1) / P : 0; }
// the sample the recursion reads at index k < rows_of(n, P) * P of an input of n > 0 samples
GLF_HD int64_t padded_index(int64_t k, int64_t n_samples) { return k < n_samples ? k : n_samples - 1; }
// the largest argument the recursion passes to sin / cos on an input of n_samples samples
GLF_HD double max_argument(double w_max, int64_t n_samples, double period) { return w_max * ((double)n_samples * period); }

// one sample: x at index `idx` of the input (pos + n), passed as the double the reference converts it to (exact below 2^53; a
// kernel counts it up by 1.0 instead of converting a 64-bit integer per sample)
template <class SinCos>
GLF_HD void step(State &st, const NoteTab &nt, float x, double idx, double period, const SinCos &sc) {
  const double time = idx * period;
  const SinCosD v = sc(nt.w * time);
  const double xd = (double)x;
  const double ds = nt.decay * st.s, dc = nt.decay * st.c;
  const double gs = nt.gain * v.s, gc = nt.gain * v.c;
  const double as = gs * xd, ac = gc * xd;
  st.s = ds + as;
  st.c = dc + ac;
}

GLF_HD float emit(const State &st) {
  const double cc = st.c * st.c, ss = st.s * st.s;
#if defined(__HIPCC__)
  const float y = (float)sqrt(cc + ss);
#else
  const float y = (float)std::sqrt(cc + ss);
#endif
  return (float)((double)y * 10.0);
}

}  // namespace tonefilt
}  // namespace smilehip
