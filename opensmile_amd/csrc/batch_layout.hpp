// What a batch of packed utterances is, as index arithmetic on the host: frames, output rows and func_in rows per utterance, and
// the work lists the kernels walk (frame tiles, window-chain tiles, 20 ms runs, the delta-fused fast kernel's tiles,
// cPitchJitter's items). Plain C++: no device header, no environment. smilehip_batch_create fills the spec from its plan and
// uploads the vectors; tests/test_batch_layout_host.py runs the same function without a device.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <vector>

#include "../../include/smilehip.h"
#include "lld_emobase_ops.hpp"
#include "lld_tile_rec.hpp"
#include "lld_tonefilt_ops.hpp"

namespace smilehip {

struct BatchLayoutSpec {
  int chain_kind = SMILEHIP_CHAIN_MFCC;
  int64_t N = 0, H = 0;                // frame length and hop in samples
  double period = 0.0;                 // sample period
  int row_extra = 0;                   // rows an utterance with frames holds beyond them (plan_row_extra)
  bool fused_delta_eligible = false;   // the plan's half of "this batch runs the delta-fused fast kernel"
  int64_t fast_slots = 8;              // wave slots of the fast kernel: max(1, blocks) * 8
  int64_t tile_frames = 0;             // frames per tile of the frame kernel
  int64_t dtile_rows = 0;              // rows per tile of the window-chain kernel
  int short_T = 0;                     // utterances of 1 .. short_T frames are lld_chain_short's
  int jitter_chunk = 0;                // frames per cPitchJitter work item
  int run_frames_override = 0;         // >= 1: frames per 20 ms run instead of compare_run_frames()
};

struct BatchLayout {
  std::vector<int64_t> samp_off, frame_off, row_off;   // [n_utt + 1]
  std::vector<int64_t> fin_off;                        // eGeMAPS: [n_utt + 1] rows of func_in, T20 + 1 per utterance with a 60 ms frame
  std::vector<int32_t> short_utts;
  bool all_even = true;                                // every utterance with frames starts at an even sample offset
  int64_t total_frames = 0, total_rows = 0;
  std::vector<int32_t> tile_utt, tile_t0, dtile_utt, dtile_t0;
  std::vector<TileRec> tile_rec;
  std::vector<int32_t> run_utt, run_t0;                // ComParE A+B, whole ComParE, eGeMAPS
  int32_t run_frames = 8;
  std::vector<FTileRec> ftiles;                        // MFCC / PLP: non-empty when the batch runs the delta-fused fast kernel
  std::vector<int32_t> jit_utt, jit_t0;                // F0 group
  std::vector<int32_t> frame_utt;                      // IS09, prosodyAcf, chroma_fft, audspec, spectrogram, emobase: the utterance of every frame
};

constexpr int kRunFramesMin = 8;   // frames per 20 ms run when the caller names none (lld_compare.hip / lld_gemaps.hip)

// Frames per run for a batch of `total_frames` 20 ms frames: a run costs one transform more than its frames (the warm-up frame),
// 12.5 % at 8; the longest of 8 / 16 / 32 / 64 that still leaves >= 65 536 runs (21 per wave slot of the device).
inline int compare_run_frames(int64_t total_frames) {
  int L = kRunFramesMin;
  while (L < 64 && total_frames / (2 * L) >= 65536) L *= 2;
  return L;
}

inline int64_t layout_num_frames(int64_t len, int64_t N, int64_t H) { return len < N ? 0 : (len - N) / H + 1; }
// chroma_filt has no framer: cTonefilt reads blocks of N = H samples and, at the end of input, one more that holds the samples left
// over (tonefilt::rows_of, lld_tonefilt_ops.hpp)
inline int64_t layout_num_frames(const BatchLayoutSpec &s, int64_t len) {
  return s.chain_kind == SMILEHIP_CHAIN_CHROMA_FILT ? tonefilt::rows_of(len, s.H) : layout_num_frames(len, s.N, s.H);
}
inline int64_t samples_60ms(double period) { return std::lround(0.060 / period); }
inline int64_t samples_40ms(double period) { return std::lround(0.040 / period); }   // emobase.conf [fr40:cFramer]

// Output rows of an utterance of `len` samples / T frames. The 20 ms chains hold rows = T60 + 1, T60 = frames of the 60 ms
// framer ([is13_frame60]; what both egemapsv02_lldsetE_smo and egemapsv02_lldsetF_smo hold): none if T60 < 4 (ComParE) / < 1 (eGeMAPS).
inline int64_t layout_rows(const BatchLayoutSpec &s, int64_t len, int64_t T) {
  const bool compare = s.chain_kind == SMILEHIP_CHAIN_COMPARE_AB || s.chain_kind == SMILEHIP_CHAIN_COMPARE;
  // prosodyShs: cPitchSmoother's level holds T - 1 frames (no output for its first call), the smoother adds its end-of-input rows
  if (s.chain_kind == SMILEHIP_CHAIN_PROSODY_SHS) return T >= 2 ? T - 1 + s.row_extra : 0;
  // emobase: the smoother reads four levels of T (25 ms) frames and one of T40 <= T; the shortest decides (emobase::rows_of)
  if (s.chain_kind == SMILEHIP_CHAIN_EMOBASE) return emobase::rows_of(T, layout_num_frames(len, samples_40ms(s.period), s.H), (int)s.row_extra);
  // (IS09 and prosodyAcf: T + smaWin / 2 rows, prosody_acf::rows_of; chroma_fft and chroma_filt: T rows, chroma::rows_of / tonefilt::rows_of;
  //  audspec: T rows, audspec::rows_of; spectrogram: T rows, spectrogram::rows_of)
  if (!compare && s.chain_kind != SMILEHIP_CHAIN_EGEMAPS) return T > 0 ? T + s.row_extra : 0;
  const int64_t T60 = layout_num_frames(len, samples_60ms(s.period), s.H);
  return T60 >= (compare ? 4 : 1) ? T60 + 1 : 0;
}

// The fast kernel with the two regression stages inside (lld_mfcc512<..., DELTA>): tiles as long as the batch allows -- a tile
// pays one pass of four frames before it (inside an utterance) and one behind it. L = the tile length whose estimate
// ceil(tiles / wave slots) x (L / 4 + 2) passes is smallest; an utterance is cut into equal parts of at most L frames
// (multiples of four: a frame's lane group is its index mod 4).
inline void layout_fused_tiles(const BatchLayoutSpec &s, const int64_t *h_off, int32_t n_utt, BatchLayout &out) {
  const auto parts_of = [&](int64_t T, int64_t L) { return (T + L - 1) / L; };
  int64_t bestL = 32;
  double best = 1e300;
  // (the count of distinct utterance lengths, not the count of utterances, is what the 505 candidate lengths are tried on)
  std::map<int64_t, int64_t> hist;
  for (int32_t u = 0; u < n_utt; ++u) {
    const int64_t T = out.frame_off[u + 1] - out.frame_off[u];
    if (T > 0) hist[T]++;
  }
  for (int64_t L = 32; L <= 2048; L += 4) {
    int64_t n = 0;
    for (const auto &h : hist) n += h.second * ((h.first <= s.short_T) ? 1 : parts_of(h.first, L));
    const double cost = double((n + s.fast_slots - 1) / s.fast_slots) * double(L / 4 + 2);
    if (cost <= best) { best = cost; bestL = L; }
  }
  for (int32_t u = 0; u < n_utt; ++u) {
    const int64_t T = out.frame_off[u + 1] - out.frame_off[u];
    if (T <= 0) continue;
    const int64_t parts = (T <= s.short_T) ? 1 : parts_of(T, bestL);
    const int64_t len = (((T + parts - 1) / parts) + 3) & ~int64_t(3);
    for (int64_t t0 = 0; t0 < T; t0 += len) {
      const int64_t t1 = std::min<int64_t>(T, t0 + len), p0 = t0 > 0 ? t0 - 4 : 0;
      FTileRec r;
      r.samp0 = h_off[u] + p0 * s.H;
      r.row0 = out.frame_off[u] + p0;
      const int64_t last = (t1 + 3) & ~int64_t(3);      // first frame of the last pass: the one behind the tile's last frame (rows are written one pass late)
      r.n_frames = (int32_t)(last - p0 + 4);
      r.live_n = (int32_t)(T - p0);
      r.e0 = (int32_t)(t0 - p0);
      r.e1 = (int32_t)(t1 - p0);
      r.lo = (int32_t)(-p0);
      r.delta_on = T > s.short_T;
      out.ftiles.push_back(r);
    }
  }
  std::stable_sort(out.ftiles.begin(), out.ftiles.end(), [](const FTileRec &a, const FTileRec &c) { return a.n_frames > c.n_frames; });   // long tiles first
}

// Returns 0, or u + 1 for the first utterance u whose offsets decrease (out is then unfinished).
inline int batch_layout(const BatchLayoutSpec &s, const int64_t *h_off, int32_t n_utt, BatchLayout &out) {
  out = BatchLayout();
  out.samp_off.assign(h_off, h_off + (n_utt ? n_utt + 1 : 0));
  if (n_utt == 0) out.samp_off.assign(1, 0);
  out.frame_off.assign(size_t(n_utt) + 1, 0);
  out.row_off.assign(size_t(n_utt) + 1, 0);
  const bool compare = s.chain_kind == SMILEHIP_CHAIN_COMPARE_AB || s.chain_kind == SMILEHIP_CHAIN_COMPARE;
  const bool egemaps = s.chain_kind == SMILEHIP_CHAIN_EGEMAPS;
  if (egemaps) out.fin_off.assign(size_t(n_utt) + 1, 0);
  {                                                      // the run length of the 20 ms frame kernels (lld_compare.hip / lld_gemaps.hip)
    int64_t total_T = 0;
    for (int32_t u = 0; u < n_utt; ++u) total_T += layout_num_frames(s, h_off[u + 1] - h_off[u]);
    out.run_frames = s.run_frames_override >= 1 ? s.run_frames_override : compare_run_frames(total_T);
  }
  for (int32_t u = 0; u < n_utt; ++u) {
    const int64_t len = h_off[u + 1] - h_off[u];
    if (len < 0) return u + 1;
    const int64_t T = layout_num_frames(s, len);
    const int64_t rows = layout_rows(s, len, T);
    if (compare || egemaps)
      for (int64_t t0 = 0; t0 < T; t0 += out.run_frames) {
        out.run_utt.push_back(u);
        out.run_t0.push_back((int32_t)t0);
      }
    if (egemaps) out.fin_off[u + 1] = out.fin_off[u] + (rows > 0 ? T + 1 : 0);
    out.frame_off[u + 1] = out.frame_off[u] + T;
    out.row_off[u + 1] = out.row_off[u] + rows;
    if (T > 0 && T <= s.short_T) out.short_utts.push_back(u);
    if (T > 0 && (h_off[u] & 1)) out.all_even = false;
    for (int64_t t0 = 0; t0 < T; t0 += s.tile_frames) {
      out.tile_utt.push_back(u);
      out.tile_t0.push_back((int32_t)t0);
      TileRec r;
      r.samp0 = h_off[u] + t0 * s.H;
      r.row0 = out.frame_off[u] + t0;
      r.n_frames = (int32_t)std::min<int64_t>(s.tile_frames, T - t0);
      r.pad = 0;
      out.tile_rec.push_back(r);
    }
    for (int64_t t0 = 0; t0 < rows; t0 += s.dtile_rows) {
      out.dtile_utt.push_back(u);
      out.dtile_t0.push_back((int32_t)t0);
    }
  }
  out.total_frames = out.frame_off[n_utt];
  out.total_rows = out.row_off[n_utt];
  if ((s.chain_kind == SMILEHIP_CHAIN_IS09 || s.chain_kind == SMILEHIP_CHAIN_PROSODY_ACF || s.chain_kind == SMILEHIP_CHAIN_CHROMA_FFT ||
       s.chain_kind == SMILEHIP_CHAIN_AUDSPEC || s.chain_kind == SMILEHIP_CHAIN_SPECTROGRAM || s.chain_kind == SMILEHIP_CHAIN_EMOBASE) &&
      out.total_frames > 0) {
    out.frame_utt.resize((size_t)out.total_frames);
    for (int32_t u = 0; u < n_utt; ++u) std::fill(out.frame_utt.begin() + out.frame_off[u], out.frame_utt.begin() + out.frame_off[u + 1], u);
  }
  if (s.fused_delta_eligible && out.total_frames > 0 && out.all_even)   // (all_even: the dword loads of the aligned instance)
    layout_fused_tiles(s, h_off, n_utt, out);
  if (s.chain_kind == SMILEHIP_CHAIN_COMPARE_F0) {
    // cPitchJitter's work items: jitter_chunk consecutive frames of one utterance each, all first chunks, then all second chunks, ...
    // (the chains that begin in a chunk can run to the utterance's end: the longest possible ones are launched first)
    int64_t maxT = 0;
    for (int32_t u = 0; u < n_utt; ++u) maxT = std::max(maxT, out.frame_off[u + 1] - out.frame_off[u]);
    for (int64_t t0 = 0; t0 < maxT; t0 += s.jitter_chunk)
      for (int32_t u = 0; u < n_utt; ++u)
        if (t0 < out.frame_off[u + 1] - out.frame_off[u]) { out.jit_utt.push_back(u); out.jit_t0.push_back((int32_t)t0); }
  }
  return 0;
}

}  // namespace smilehip
