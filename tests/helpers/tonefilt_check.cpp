// Host build of opensmile_amd/csrc/lld_tonefilt_ops.hpp, lld_sincos_d.hpp and tonefilt_tables.cpp (tests/helpers/tonefilt_host.py
// compiles them with g++): cTonefilt's tables and its rows from samples with the C library's sin / cos -- what the binary calls --,
// the same recursion with every libm result moved one ulp (the measure D of what the device's own sine and cosine may change),
// and sincos_d itself next to sinl / cosl.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../opensmile_amd/csrc/lld_tonefilt_ops.hpp"
#include "../../opensmile_amd/csrc/tonefilt_tables.hpp"

using namespace smilehip;

extern "C" int64_t tonefilt_block_len(double rate, double output_period) { return tonefilt::block_len(rate, output_period); }
extern "C" int64_t tonefilt_rows_of(int64_t n, int64_t P) { return tonefilt::rows_of(n, P); }
extern "C" double tonefilt_domain() { return kSincosDomain; }

// the tables of smilehip_tonefilt_op_tables, from this build; returns nNotes or a negative value
extern "C" int tonefilt_tables(int n_notes, double first_note, double decay_f0, double decay_fn, double output_period, double rate,
                               int64_t *block_len, double *freq, double *decay, double *w) {
  const smilehip_tonefilt_opts o = {n_notes, 0, first_note, decay_f0, decay_fn, output_period};
  TonefiltHost h;
  const int rc = make_tonefilt_tables(o, rate, h, nullptr);
  if (rc) return rc < 0 ? rc : -rc;
  if (block_len) *block_len = h.P;
  for (int n = 0; n < h.n_notes; ++n) {
    if (freq) freq[n] = h.tab[(size_t)n].freq;
    if (decay) decay[n] = h.tab[(size_t)n].decay;
    if (w) w[n] = h.tab[(size_t)n].w;
  }
  return h.n_notes;
}

namespace {
// xorshift64*: the seeded signs of the one-ulp perturbation
struct Rng {
  uint64_t s;
  uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; }
};
struct PerturbedSinCos {
  mutable Rng r;
  SinCosD operator()(double x) const {
    SinCosD v = tonefilt::LibmSinCos()(x);
    const uint64_t b = r.next();
    v.s = std::nextafter(v.s, (b & 1) ? INFINITY : -INFINITY);
    v.c = std::nextafter(v.c, (b & 2) ? INFINITY : -INFINITY);
    return v;
  }
};
template <class SC>
void run(const TonefiltHost &h, const float *x, int64_t n_blocks, int64_t pos, double *s, double *c, float *ts, const SC &sc) {
  for (int t = 0; t < h.n_notes; ++t) {                    // doFilter: notes outside, samples inside
    tonefilt::State st = {s[t], c[t]};
    for (int64_t b = 0; b < n_blocks; ++b) {
      for (int64_t n = 0; n < h.P; ++n) tonefilt::step(st, h.tab[(size_t)t], x[b * h.P + n], (double)(pos + b * h.P + n), h.period, sc);
      if (ts) ts[b * h.n_notes + t] = tonefilt::emit(st);
    }
    s[t] = st.s;
    c[t] = st.c;
  }
}
}  // namespace

// x: n_blocks * P float samples that start at sample `pos`; s, c [nNotes] in and out; ts: n_blocks x nNotes (optional).
// mode 0: libm; 1: libm with every result moved one ulp, sign from `seed`; 2: sincos_d. Returns nNotes or a negative value.
extern "C" int tonefilt_blocks(int n_notes, double first_note, double decay_f0, double decay_fn, double output_period, double rate, const float *x,
                               int64_t n_blocks, int64_t pos, double *s, double *c, float *ts, int mode, uint64_t seed) {
  const smilehip_tonefilt_opts o = {n_notes, 0, first_note, decay_f0, decay_fn, output_period};
  TonefiltHost h;
  const int rc = make_tonefilt_tables(o, rate, h, nullptr);
  if (rc) return rc < 0 ? rc : -rc;
  if (mode == 0) run(h, x, n_blocks, pos, s, c, ts, tonefilt::LibmSinCos());
  else if (mode == 1) { PerturbedSinCos p; p.r.s = seed | 1; run(h, x, n_blocks, pos, s, c, ts, p); }
  else run(h, x, n_blocks, pos, s, c, ts, tonefilt::DevSinCos());
  return h.n_notes;
}

// sincos_d of this build next to sinl / cosl: err[0], err[1] = the largest error of sine and cosine in ulps of the true value's
// binade, at[0], at[1] = where; s, c (optional) receive the values
extern "C" void tonefilt_sincos_check(const double *x, int64_t n, double *s, double *c, double *err, double *at) {
  err[0] = err[1] = 0.0;
  at[0] = at[1] = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    const SinCosD v = sincos_d(x[i]);
    if (s) s[i] = v.s;
    if (c) c[i] = v.c;
    const long double ts = sinl((long double)x[i]), tc = cosl((long double)x[i]);
    const long double got[2] = {(long double)v.s, (long double)v.c}, want[2] = {ts, tc};
    for (int k = 0; k < 2; ++k) {
      if (want[k] == 0.0L) { if (got[k] != 0.0L) { err[k] = INFINITY; at[k] = x[i]; } continue; }
      int e;
      frexpl(want[k], &e);                                 // |want| in [2^(e-1), 2^e): ulp = 2^(e - 53)
      const double u = (double)fabsl(ldexpl(got[k] - want[k], 53 - e));
      if (u > err[k]) { err[k] = u; at[k] = x[i]; }
    }
  }
}
// ulp errors of given values (a device's) against sinl / cosl, the same measure
extern "C" void tonefilt_sincos_err(const double *x, const double *s, const double *c, int64_t n, double *err, double *at) {
  err[0] = err[1] = 0.0;
  at[0] = at[1] = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    const long double got[2] = {(long double)s[i], (long double)c[i]}, want[2] = {sinl((long double)x[i]), cosl((long double)x[i])};
    for (int k = 0; k < 2; ++k) {
      if (want[k] == 0.0L) { if (got[k] != 0.0L) { err[k] = INFINITY; at[k] = x[i]; } continue; }
      int e;
      frexpl(want[k], &e);
      const double u = (double)fabsl(ldexpl(got[k] - want[k], 53 - e));
      if (u > err[k]) { err[k] = u; at[k] = x[i]; }
    }
  }
}
