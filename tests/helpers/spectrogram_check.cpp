// Host build of opensmile_amd/csrc/lld_spectrogram_ops.hpp as a stand-alone program (tests/helpers/spectrogram_host.py compiles this
// file with g++ -ffp-contract=off; nothing of the library is linked): cFFTmagphase's rows from cTransformFFT's rows in each of the
// five forms, the row rule and the mindBp clamp -- what lld_spectrogram_frame computes on the device in both of its forms, held to the
// real binary's levels by tests/test_spectrogram_host.py.
//
//   spectrogram_check rows <n_samples> <N> <H>                     prints spectrogram::rows_of
//   spectrogram_check clamp <dbp_norm> <min_dbp>                   prints mindBp behind the clamp, as the bits of the float (hex)
//   spectrogram_check form <flags>                                 prints spectrogram::form_of_flags
//   spectrogram_check spectrum <form> <Nfft> <dbp_norm> <min_dbp> <in.f32> <out.f32>
//        in: n_frames x Nfft floats (the level fft, host byte order) -> out: n_frames x (Nfft / 2 + 1) floats (the level lld)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../opensmile_amd/csrc/lld_spectrogram_ops.hpp"

using namespace smilehip;

int main(int argc, char **argv) {
  if (argc == 5 && !strcmp(argv[1], "rows")) {
    printf("%lld\n", (long long)spectrogram::rows_of(atoll(argv[2]), atoll(argv[3]), atoll(argv[4])));
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "clamp")) {
    const float v = spectrogram::clamp_min_dbp(strtof(argv[2], nullptr), strtof(argv[3], nullptr));
    uint32_t u;
    memcpy(&u, &v, 4);
    printf("%08x\n", u);
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "form")) {
    printf("%d\n", spectrogram::form_of_flags((int32_t)atoi(argv[2])));
    return 0;
  }
  if (argc == 8 && !strcmp(argv[1], "spectrum")) {
    const int form = atoi(argv[2]);
    const int64_t nfft = atoll(argv[3]);
    if (form < spectrogram::kMagnitude || form > spectrogram::kDbPsd || nfft < 2 || (nfft & 1)) return 2;
    const spectrogram::FormConsts F = spectrogram::form_consts(form, nfft, strtof(argv[4], nullptr), strtof(argv[5], nullptr));
    FILE *fi = fopen(argv[6], "rb");
    if (!fi) return 3;
    std::vector<float> in;
    float buf[4096];
    size_t got;
    while ((got = fread(buf, sizeof(float), 4096, fi)) > 0) in.insert(in.end(), buf, buf + got);
    fclose(fi);
    if (in.size() % (size_t)nfft) return 4;
    const int64_t n_frames = (int64_t)(in.size() / (size_t)nfft), K = nfft / 2 + 1;
    std::vector<float> out((size_t)(n_frames * K));
    for (int64_t f = 0; f < n_frames; ++f) spectrogram::spectrum_row(in.data() + f * nfft, nfft, F, out.data() + f * K);
    FILE *fo = fopen(argv[7], "wb");
    if (!fo) return 5;
    const bool ok = fwrite(out.data(), sizeof(float), out.size(), fo) == out.size();
    return fclose(fo) == 0 && ok ? 0 : 6;
  }
  fprintf(stderr, "usage: spectrogram_check rows|clamp|form|spectrum ...\n");
  return 1;
}
