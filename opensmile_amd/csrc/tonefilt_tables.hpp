// Host tables of cTonefilt (src/lld/tonefilt.cpp:65-98, 180-189): what depends on the options alone, computed once per plan /
// operator. Host only and free of HIP, so that tests/helpers/tonefilt_check.cpp compiles it with g++ next to lld_tonefilt_ops.hpp.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/smilehip.h"
#include "lld_tonefilt_ops.hpp"

namespace smilehip {

struct TonefiltHost {
  int32_t n_notes = 0;
  int64_t P = 0;                            // samples per block (tonefilt::block_len)
  double period = 0.0;                      // inputPeriod
  double output_period = 0.0;               // the level's period behind the component
  std::vector<tonefilt::NoteTab> tab;       // [n_notes]
};

// 0 on success, otherwise `why` names the option
int make_tonefilt_tables(const smilehip_tonefilt_opts &o, double sample_rate, TonefiltHost &h, const char **why);
// the input lengths sincos_d's domain admits: 0 where n_samples of input stay inside, SMILEHIP_ERR_INVALID otherwise
int tonefilt_check_domain(const TonefiltHost &h, int64_t n_samples);

}  // namespace smilehip
