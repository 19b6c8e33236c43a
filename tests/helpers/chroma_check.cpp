// Host build of opensmile_amd/csrc/lld_chroma_ops.hpp and chroma_tables.cpp (tests/helpers/chroma_host.py compiles both with g++):
// cTonespec's tables, its rows from magnitude rows, cChroma's rows from those -- what lld_chroma_frame and the two operators compute
// on the device, held to the real binary's levels by tests/test_chroma_fft_host.py.
#include <cstdint>
#include <cstring>

#include "../../opensmile_amd/csrc/chroma_tables.hpp"
#include "../../opensmile_amd/csrc/lld_chroma_ops.hpp"

using namespace smilehip;

extern "C" int64_t chroma_rows_of(int64_t n_samples, int64_t N, int64_t H) { return chroma::rows_of(n_samples, N, H); }

// the tables of smilehip_tonespec_op_tables, from this build; returns nNotes or a negative value
extern "C" int chroma_tables(int n_octaves, float first_note, int filter_type, int use_power, int dba, int64_t n_src, double frame_size_sec,
                             float *pitch_class_freq, int32_t *bin_key, int32_t *nbins, float *filter_map, int32_t *note_rec, int32_t *first_last) {
  const smilehip_tonespec_opts o = {n_octaves, first_note, filter_type, use_power, dba};
  TonespecHost h;
  const int rc = make_tonespec_tables(o, n_src, frame_size_sec, h, nullptr);
  if (rc) return rc < 0 ? rc : -rc;
  if (pitch_class_freq) std::memcpy(pitch_class_freq, h.pitch_class_freq.data(), h.pitch_class_freq.size() * sizeof(float));
  if (bin_key) std::memcpy(bin_key, h.bin_key.data(), h.bin_key.size() * sizeof(int32_t));
  if (nbins) std::memcpy(nbins, h.nbins.data(), h.nbins.size() * sizeof(int32_t));
  if (filter_map) std::memcpy(filter_map, h.filter_map.data(), h.filter_map.size() * sizeof(float));
  if (note_rec) std::memcpy(note_rec, h.rec.data(), h.rec.size() * sizeof(chroma::NoteRec));
  if (first_last) { first_last[0] = h.first_bin; first_last[1] = h.last_bin; }
  return h.n_notes;
}

// mag: n_frames x n_src -> ts: n_frames x nNotes; returns nNotes or a negative value
extern "C" int chroma_tonespec_rows(int n_octaves, float first_note, int filter_type, int use_power, int dba, int64_t n_src, double frame_size_sec,
                                    const float *mag, int64_t n_frames, float *ts) {
  const smilehip_tonespec_opts o = {n_octaves, first_note, filter_type, use_power, dba};
  TonespecHost h;
  const int rc = make_tonespec_tables(o, n_src, frame_size_sec, h, nullptr);
  if (rc) return rc < 0 ? rc : -rc;
  for (int64_t t = 0; t < n_frames; ++t)
    chroma::tonespec_row(mag + t * n_src, h.filter_map.data(), h.rec.data(), h.n_notes, use_power != 0, ts + t * h.n_notes);
  return h.n_notes;
}

// ts: n_frames x n_src -> out: n_frames x octave_size
extern "C" void chroma_chroma_rows(const float *ts, int64_t n_frames, int n_src, int octave_size, float sil_thresh, float *out) {
  for (int64_t t = 0; t < n_frames; ++t) chroma::chroma_row(ts + t * n_src, n_src, octave_size, sil_thresh, out + t * octave_size);
}
