// cTonefilt's tables (tonefilt_tables.hpp), all in double as the component keeps them; pow is the C library's on run-time operands
// (nothing folded or replaced by exp2 at compile time), no product feeds a sum in one operation (-ffp-contract=off).
#include "tonefilt_tables.hpp"

#include <cmath>

namespace smilehip {

namespace {
double lib_pow(double b, double e) {
  volatile double vb = b, ve = e;
  return std::pow(vb, ve);
}
}  // namespace

int make_tonefilt_tables(const smilehip_tonefilt_opts &o, double sample_rate, TonefiltHost &h, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  h = TonefiltHost();
  if (!(sample_rate >= 1.0) || !std::isfinite(sample_rate)) { *why = "sample_rate must be at least 1 Hz"; return SMILEHIP_ERR_INVALID; }
  if (!std::isfinite(o.first_note) || !std::isfinite(o.decay_f0) || !std::isfinite(o.decay_fn) || !std::isfinite(o.output_period)) {
    *why = "firstNote, decayF0, decayFN and outputPeriod must be finite numbers";
    return SMILEHIP_ERR_INVALID;
  }
  // myFetchConfig (tonefilt.cpp:69-90)
  double outputPeriod = o.output_period;
  if (outputPeriod <= 0.0) outputPeriod = 0.1;
  double decayFN = o.decay_fn;
  if (decayFN < 0.0) decayFN = 0.0;
  if (decayFN > 1.0) decayFN = 1.0;
  double decayF0 = o.decay_f0;
  if (decayF0 < decayFN) decayF0 = decayFN;
  if (decayF0 < 0.0) decayF0 = 0.0;
  if (decayF0 > 1.0) decayF0 = 1.0;
  double firstNote = o.first_note;
  if (firstNote <= 0.0) firstNote = 1.0;
  int nNotes = o.n_notes;
  if (nNotes < 1) nNotes = 1;
  if (nNotes > tonefilt::kMaxNotes) { *why = "nNotes must be at most 120"; return SMILEHIP_ERR_INVALID; }
  h.n_notes = nNotes;
  h.period = tonefilt::input_period(sample_rate);
  h.P = tonefilt::block_len(sample_rate, outputPeriod);
  if (h.P < 1 || h.P > (int64_t)1 << 30) { *why = "outputPeriod must give blocks of 1 .. 2^30 samples"; return SMILEHIP_ERR_INVALID; }
  h.output_period = outputPeriod < h.period ? h.period : outputPeriod;   // configureWriter (:121-127)
  // setupNewNames (:180-189)
  h.tab.resize((size_t)nNotes);
  for (int n = 0; n < nNotes; ++n) h.tab[(size_t)n].freq = firstNote * lib_pow(2.0, (double)n / 12.0);
  for (int n = 0; n < nNotes; ++n) {
    tonefilt::NoteTab &t = h.tab[(size_t)n];
    const double a = decayF0 - decayFN, b = t.freq - h.tab[0].freq;
    const double ab = a * b;
    const double q = ab / h.tab[(size_t)nNotes - 1].freq;
    t.decay = decayFN + q;
    t.gain = 1.0 - t.decay;
    t.w = tonefilt::kTwoPi * t.freq;
  }
  return SMILEHIP_OK;
}

int tonefilt_check_domain(const TonefiltHost &h, int64_t n_samples) {
  double w = 0.0;
  for (const tonefilt::NoteTab &t : h.tab) w = std::fabs(t.w) > w ? std::fabs(t.w) : w;
  return tonefilt::max_argument(w, n_samples, h.period) <= kSincosDomain ? SMILEHIP_OK : SMILEHIP_ERR_INVALID;
}

}  // namespace smilehip
