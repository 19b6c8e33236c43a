// opensmile_amd/csrc/batch_layout.hpp compiled for the host: runs batch_layout() on one offset list and hands every vector of the
// result to tests/test_batch_layout_host.py as int64 columns.
#include <cstring>
#include <string>

#include "../../opensmile_amd/csrc/batch_layout.hpp"

using namespace smilehip;

namespace {
struct Result {
  int rc = 0;
  std::map<std::string, std::vector<int64_t>> v;
};
template <typename T>
std::vector<int64_t> widen(const std::vector<T> &a) { return std::vector<int64_t>(a.begin(), a.end()); }
}  // namespace

extern "C" {

// spec_i: chain_kind, N, H, row_extra, fused_delta_eligible, fast_slots, tile_frames, dtile_rows, short_T, jitter_chunk, run_frames_override
void *blc_run(const int64_t *spec_i, double period, const int64_t *h_off, int32_t n_utt) {
  BatchLayoutSpec s;
  s.chain_kind = (int)spec_i[0];
  s.N = spec_i[1];
  s.H = spec_i[2];
  s.period = period;
  s.row_extra = (int)spec_i[3];
  s.fused_delta_eligible = spec_i[4] != 0;
  s.fast_slots = spec_i[5];
  s.tile_frames = spec_i[6];
  s.dtile_rows = spec_i[7];
  s.short_T = (int)spec_i[8];
  s.jitter_chunk = (int)spec_i[9];
  s.run_frames_override = (int)spec_i[10];
  BatchLayout L;
  auto *r = new Result();
  r->rc = batch_layout(s, h_off, n_utt, L);
  if (r->rc) return r;
  auto &v = r->v;
  v["samp_off"] = L.samp_off; v["frame_off"] = L.frame_off; v["row_off"] = L.row_off; v["fin_off"] = L.fin_off;
  v["short_utts"] = widen(L.short_utts);
  v["scalars"] = {L.all_even ? 1 : 0, L.total_frames, L.total_rows, L.run_frames};
  v["tile_utt"] = widen(L.tile_utt); v["tile_t0"] = widen(L.tile_t0);
  v["dtile_utt"] = widen(L.dtile_utt); v["dtile_t0"] = widen(L.dtile_t0);
  v["run_utt"] = widen(L.run_utt); v["run_t0"] = widen(L.run_t0);
  v["jit_utt"] = widen(L.jit_utt); v["jit_t0"] = widen(L.jit_t0);
  v["frame_utt"] = widen(L.frame_utt);
  for (const TileRec &t : L.tile_rec) v["tile_rec"].insert(v["tile_rec"].end(), {t.samp0, t.row0, t.n_frames, t.pad});
  for (const FTileRec &t : L.ftiles)
    v["ftiles"].insert(v["ftiles"].end(), {t.samp0, t.row0, t.n_frames, t.live_n, t.e0, t.e1, t.lo, t.delta_on});
  return r;
}
int blc_rc(const void *h) { return static_cast<const Result *>(h)->rc; }
int64_t blc_size(const void *h, const char *name) {
  const auto &v = static_cast<const Result *>(h)->v;
  const auto it = v.find(name);
  return it == v.end() ? 0 : (int64_t)it->second.size();
}
void blc_copy(const void *h, const char *name, int64_t *dst) {
  const auto &v = static_cast<const Result *>(h)->v;
  const auto it = v.find(name);
  if (it != v.end() && !it->second.empty()) std::memcpy(dst, it->second.data(), it->second.size() * sizeof(int64_t));
}
void blc_free(void *h) { delete static_cast<Result *>(h); }
int blc_compare_run_frames(int64_t total_frames) { return compare_run_frames(total_frames); }

}  // extern "C"
