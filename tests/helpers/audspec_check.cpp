// Host build of opensmile_amd/csrc/lld_audspec_ops.hpp on the plan's own tables (make_geometry / make_mel of libsmilehip.so;
// tests/helpers/audspec_host.py compiles this file with g++ and links it to the library): cMelspec's rows from magnitude rows, cPlp's
// auditory-spectrum rows from those -- what lld_audspec_frame computes on the device in both of its forms, held to the real binary's
// levels by tests/test_audspec_host.py.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../opensmile_amd/csrc/lld_audspec_ops.hpp"
#include "../../opensmile_amd/csrc/tables.hpp"

using namespace smilehip;

namespace {
// the caller's struct as far as its struct_size reaches, zeros behind it (the header's struct_size rules)
smilehip_lld_config full(const smilehip_lld_config *c) {
  smilehip_lld_config f;
  std::memset(&f, 0, sizeof(f));
  std::memcpy(&f, c, c->struct_size < sizeof(f) ? c->struct_size : sizeof(f));
  return f;
}
struct Tables {
  Geometry g;
  MelBank m;
  std::vector<int32_t> rng;
  std::vector<float> eql;
};
int build(const smilehip_lld_config *cfg, Tables &t) {
  const smilehip_lld_config c = full(cfg);
  int rc;
  if ((rc = make_geometry(c, t.g)) || (rc = make_mel(c, t.g, t.m))) return rc < 0 ? rc : -rc;
  t.rng.resize(size_t(4) * t.m.n_bands);
  t.eql.resize(size_t(t.m.n_bands));
  for (int b = 0; b < t.m.n_bands; ++b) {
    t.rng[4 * b + 0] = t.m.rise_lo[b]; t.rng[4 * b + 1] = t.m.rise_hi[b];
    t.rng[4 * b + 2] = t.m.fall_lo[b]; t.rng[4 * b + 3] = t.m.fall_hi[b];
    t.eql[b] = audspec::eql_htk(t.m.centres[b + 1]);
  }
  return 0;
}
}  // namespace

extern "C" int64_t audspec_rows_of(int64_t n_samples, int64_t N, int64_t H) { return audspec::rows_of(n_samples, N, H); }

// geo: N, H, Nfft, K; returns the number of bands or a negative value
extern "C" int audspec_geometry(const smilehip_lld_config *cfg, int64_t *geo, float *eql) {
  Tables t;
  if (const int rc = build(cfg, t)) return rc;
  geo[0] = t.g.N; geo[1] = t.g.H; geo[2] = t.g.Nfft; geo[3] = t.g.K;
  if (eql) std::memcpy(eql, t.eql.data(), t.eql.size() * sizeof(float));
  return t.m.n_bands;
}

// mag: n_frames x K -> mel: n_frames x n_bands; returns the number of bands or a negative value
extern "C" int audspec_mel_rows(const smilehip_lld_config *cfg, const float *mag, int64_t n_frames, int64_t K, float *mel) {
  Tables t;
  if (const int rc = build(cfg, t)) return rc;
  if (K != t.g.K) return -1000;
  std::vector<float> pw(size_t(K) + 1);
  for (int64_t f = 0; f < n_frames; ++f)
    audspec::mel_row(mag + f * K, (int)K, cfg->use_power, t.m.coef.data(), t.rng.data(), t.m.n_bands, t.m.scale, pw.data(), mel + f * t.m.n_bands);
  return t.m.n_bands;
}

// mel: n_frames x n_bands -> aud: n_frames x n_bands (melfloor 1.0: cPlp with htkcompatible)
extern "C" int audspec_aud_rows(const smilehip_lld_config *cfg, const float *mel, int64_t n_frames, float *aud) {
  Tables t;
  if (const int rc = build(cfg, t)) return rc;
  for (int64_t f = 0; f < n_frames; ++f)
    audspec::aud_row(mel + f * t.m.n_bands, t.eql.data(), t.m.n_bands, 1.0f, cfg->plp_compression, aud + f * t.m.n_bands);
  return t.m.n_bands;
}

// the frame's samples behind pre-emphasis and window, as both forms of the kernel form them: x[N] -> y[N]
extern "C" void audspec_frame_samples(const float *x, const float *win, int64_t N, int preemph, int de, float k, float offset, float *y) {
  const float one_minus_k = 1 - k;
  for (int64_t n = 0; n < N; ++n) y[n] = audspec::frame_sample(x[n], x[n ? n - 1 : 0], n == 0, preemph, de, k, one_minus_k, win[n], offset);
}
