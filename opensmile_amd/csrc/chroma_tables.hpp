// Host tables of cTonespec (src/lld/tonespec.cpp:147-367, computeDBA of src/dsp/dbA.cpp:110-126): what depends on the options and
// the magnitude level's geometry alone, computed once per plan / operator. Host only and free of HIP, so that
// tests/helpers/chroma_check.cpp compiles it with g++ next to lld_chroma_ops.hpp.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/smilehip.h"
#include "lld_chroma_ops.hpp"

namespace smilehip {

struct TonespecHost {
  int32_t n_src = 0, n_notes = 0, first_bin = 0, last_bin = 0;
  float F0 = 0.0f;                          // the bin width (float)(1.0 / frameSizeSec) of the level read (tonespec.cpp:196)
  std::vector<float> pitch_class_freq;      // [n_notes + 2] (:147-167)
  std::vector<int32_t> bin_key;             // [n_src] (:210-227)
  std::vector<int32_t> nbins;               // [n_notes + 2] pitchClassNbins, counted over first_bin .. last_bin (:254-258)
  std::vector<float> filter_map;            // [n_src] with the first/last-bin cut and the dbA weights (:268-359)
  std::vector<chroma::NoteRec> rec;         // [n_notes] the kernel's layout: the run of bins of output note k (key k + 1)
};

// n_src bins of a magnitude level whose frameSizeSec is frame_size_sec; 0 on success, otherwise `why` names the option
int make_tonespec_tables(const smilehip_tonespec_opts &o, int64_t n_src, double frame_size_sec, TonespecHost &h, const char **why);

}  // namespace smilehip
