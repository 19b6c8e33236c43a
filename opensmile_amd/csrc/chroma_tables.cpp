// cTonespec's tables (chroma_tables.hpp). Every operand keeps the type the reference gives it: FLOAT_DMEM is float, the libm calls
// are the ones a C++11 translation unit resolves (pow(float, float) and log(float) are the float overloads, as the level fixtures
// of tests/golden/make_golden_chroma_fft.py confirm), and no product feeds a sum in one operation (-ffp-contract=off).
#include "chroma_tables.hpp"

#include <cmath>

namespace smilehip {

namespace {
// the C library's functions on run-time operands: nothing here is folded or replaced by another function (exp2, exp10) at compile time
double lib_pow(double b, double e) {
  volatile double vb = b, ve = e;
  return std::pow(vb, ve);
}
double lib_exp(double x) {
  volatile double vx = x;
  return std::exp(vx);
}
float lib_logf(float x) {
  volatile float vx = x;
  return std::log(vx);
}

// computeDBA (src/dsp/dbA.cpp:110-126)
void compute_dba(std::vector<float> &x, int64_t n, float F0) {
  x.assign((size_t)n, 0.0f);
  float curF = 0.0f;
  const double p12200 = 12200.0 * 12200.0, p206 = 20.6 * 20.6, p1077 = 107.7 * 107.7, p7379 = 737.9 * 737.9;   // pow(c, 2.0)
  for (int64_t i = 0; i < n; ++i) {
    const float cf2 = curF * curF;                         // (FLOAT_DMEM)pow(curF, 2.0f)
    const float cf4 = cf2 * cf2;                           // pow(cf2, 2.0f): the float overload
    float tmp = (float)(p12200 * (double)cf4) / ((cf2 + (float)p206) * (cf2 + (float)p12200));
    tmp /= (float)(std::sqrt((double)cf2 + p1077) * std::sqrt((double)cf2 + p7379));
    x[(size_t)i] = (float)lib_pow(10.0, (10.0 * (double)lib_logf(tmp) + 2.0) / 10.0);   // log(float): logf; log(0) gives 0
    curF += F0;
  }
}
}  // namespace

int make_tonespec_tables(const smilehip_tonespec_opts &o, int64_t n_src, double frame_size_sec, TonespecHost &h, const char **why) {
  const char *dummy;
  if (!why) why = &dummy;
  if (o.n_octaves < 1 || o.n_octaves * 12 > chroma::kMaxNotes) { *why = "nOctaves must be 1 .. 10"; return SMILEHIP_ERR_INVALID; }
  if (!(o.first_note > 0.0) || !std::isfinite(o.first_note)) { *why = "firstNote must be a positive frequency"; return SMILEHIP_ERR_INVALID; }
  if (o.filter_type < SMILEHIP_TONESPEC_GAUSS || o.filter_type > SMILEHIP_TONESPEC_RECT) { *why = "filterType must be gau, tri, trp or rec"; return SMILEHIP_ERR_INVALID; }
  if (n_src < 2 || n_src > 8192) { *why = "the input must have 2 .. 8192 bins"; return SMILEHIP_ERR_INVALID; }
  if (!(frame_size_sec > 0.0) || !std::isfinite(frame_size_sec)) { *why = "the level's frameSizeSec must be positive"; return SMILEHIP_ERR_INVALID; }
  const int nNotes = o.n_octaves * 12;
  const int64_t blocksize = n_src;
  h = TonespecHost();
  h.n_src = (int32_t)n_src;
  h.n_notes = nNotes;

  // setPitchclassFreq (tonespec.cpp:147-167)
  const float firstNote = (float)o.first_note;             // :96
  std::vector<float> &pcf = h.pitch_class_freq;
  pcf.assign((size_t)nNotes + 2, 0.0f);
  const float firstNote0 = firstNote / (float)lib_pow(2.0, 1.0 / 12.0);
  pcf[0] = firstNote0;
  double n = 0.0;
  for (int i = 1; i < nNotes + 2; ++i) {
    n += 1.0;
    pcf[(size_t)i] = firstNote0 * (float)lib_pow(2.0, n / 12.0);
  }

  // computeFilters (:171-367)
  const float F0 = (float)(1.0 / frame_size_sec);
  h.F0 = F0;
  std::vector<float> db;
  if (o.dba) compute_dba(db, blocksize, F0);
  int firstBin = (int)std::ceil((double)(pcf[0] + pcf[1]) / (2.0 * (double)F0));
  int lastBin = (int)std::floor((double)(pcf[(size_t)nNotes] + pcf[(size_t)nNotes + 1]) / (2.0 * (double)F0));
  if (firstBin < 1) firstBin = 1;
  if (lastBin >= blocksize) lastBin = (int)blocksize - 1;
  h.first_bin = firstBin;
  h.last_bin = lastBin;

  h.bin_key.assign((size_t)blocksize, 0);
  int curNote = 0;
  for (int64_t i = 0; i < blocksize; ++i) {                // :213-227
    if (curNote > nNotes) curNote = nNotes;
    const float f = (float)i * F0;
    float distance0 = std::fabs(pcf[(size_t)curNote] - f);
    int note1 = curNote;
    float distance1 = std::fabs(pcf[(size_t)++note1] - f);
    while (distance0 > distance1) {
      if (note1 > nNotes) break;
      distance0 = distance1;
      distance1 = std::fabs(pcf[(size_t)++note1] - f);
    }
    curNote = note1 - 1;
    h.bin_key[(size_t)i] = curNote;
  }
  h.nbins.assign((size_t)nNotes + 2, 0);
  for (int i = firstBin; i <= lastBin; ++i)                // :254-258
    if (h.bin_key[(size_t)i] >= 0) h.nbins[(size_t)h.bin_key[(size_t)i]]++;

  std::vector<float> &fm = h.filter_map;
  fm.assign((size_t)blocksize, 0.0f);
  if (o.filter_type != SMILEHIP_TONESPEC_RECT) {           // :275-326 (a rectangular filter leaves the map at zero)
    for (int b = 1; b < nNotes - 1; ++b) {
      const float start_freq = (pcf[(size_t)b - 1] + pcf[(size_t)b]) / 2.0f;
      const float end_freq = (pcf[(size_t)b] + pcf[(size_t)b + 1]) / 2.0f;
      const float start_bin = start_freq / F0, end_bin = end_freq / F0;
      const float middle_bin = pcf[(size_t)b] / F0;
      int i_start_bin = (int)std::ceil(start_bin), i_end_bin = (int)std::floor(end_bin);
      const int i_middle_bin = (int)std::round(pcf[(size_t)b] / F0);
      if (i_start_bin > i_end_bin) continue;
      if (i_end_bin >= blocksize) i_end_bin = (int)blocksize - 1;
      if (i_start_bin >= blocksize) i_start_bin = (int)blocksize - 1;
      if (i_start_bin < 1) i_start_bin = 1;
      if (o.filter_type == SMILEHIP_TONESPEC_TRI || o.filter_type == SMILEHIP_TONESPEC_TRI_POWERED) {
        for (int i = i_start_bin; i < i_middle_bin && i < blocksize; ++i) {
          float v = 1.0f - ((middle_bin - (float)i) / (middle_bin - start_bin));
          if (v > 1.0f) v = 2.0f - v;
          fm[(size_t)i] = v;
        }
        for (int i = i_middle_bin < 0 ? 0 : i_middle_bin; i <= i_end_bin; ++i) {
          float v = 1.0f - (((float)i - middle_bin) / (end_bin - middle_bin));
          if (v > 1.0f) v = 2.0f - v;
          fm[(size_t)i] = v;
        }
      }
      if (o.filter_type == SMILEHIP_TONESPEC_GAUSS) {
        for (int i = i_start_bin; i <= i_end_bin; ++i) {
          const double dist_val = (double)(end_bin - start_bin);
          if (dist_val > 0.0) {
            const double x_val = (double)i - (double)middle_bin;
            const double delta = dist_val / 15.0;
            fm[(size_t)i] = (float)((10.0 / 4.0) * (1.0 / std::sqrt(2.0 * M_PI)) * lib_exp(-0.5 * (1.0 / delta) * (1.0 / delta) * (x_val * x_val)));
          }
        }
      }
    }
  }
  if (o.filter_type == SMILEHIP_TONESPEC_TRI_POWERED)
    for (int64_t i = 0; i < blocksize; ++i) fm[(size_t)i] *= fm[(size_t)i];
  for (int i = 0; i < firstBin && i < blocksize; ++i) fm[(size_t)i] = 0.0f;       // :347-352
  for (int64_t i = (int64_t)lastBin + 1; i < blocksize; ++i) fm[(size_t)i] = 0.0f;
  if (o.dba)                                               // :354-359: the curve is read from its element 0, bin firstBin + k gets the weight of k * F0
    for (int i = firstBin, k = 0; i <= lastBin; ++i, ++k) fm[(size_t)i] *= db[(size_t)k];

  // the kernel's layout: output note k sums the bins firstBin .. lastBin whose key is k + 1 (:418-422), one run
  h.rec.assign((size_t)nNotes, chroma::NoteRec{0, 0, 0, 0});
  for (int i = lastBin; i >= firstBin; --i) {
    const int key = h.bin_key[(size_t)i];
    if (key > 0 && key <= nNotes) {
      chroma::NoteRec &r = h.rec[(size_t)key - 1];
      r.first = i;
      r.count++;
    }
  }
  for (int k = 0; k < nNotes; ++k) h.rec[(size_t)k].nbins = h.nbins[(size_t)k + 1];
  return SMILEHIP_OK;
}

}  // namespace smilehip
