// config/chroma/chroma_filt.conf (SMILEHIP_CHAIN_CHROMA_FILT): cTonefilt's sine filter bank as a scan over the samples, and the
// same scan as a stream operator (smilehip_tonefilt_op_blocks).
//
// lld_tonefilt_scan: ONE LANE PER CHAIN. Chain g = n_notes u + t is note t of utterance u; chains are numbered across waves, so a
// wave straddles utterances of different lengths and its lanes finish at different times (the loop bound is the lane's own). A
// lane walks its utterance's samples in order and runs tonefilt::step per sample -- two double states, the double sine and cosine
// of one argument (sincos_d) -- and at every P-th sample writes tonefilt::emit to its column of the tonespec level. There is no LDS
// and no communication between lanes: the work is pure FP64 VALU, about 1.6e5 sequential steps per 10 s of audio at 16 kHz, and one
// file occupies n_notes / 64 waves however long it is (splitting a chain in time would change how its sums round).
// Lanes of one utterance read the same address; a lane fetches kAhead samples at a time, one group ahead of the one it works on,
// so that the only memory latency in the loop is hidden behind kAhead steps of arithmetic. Every load carries an index clamped
// into the lane's own samples, which is also the reference's rule for the last block of an utterance (the last sample repeated).
#include <hip/hip_runtime.h>

#include "kernel_timing.hpp"
#include "lld_device.hpp"
#include "lld_launch.hpp"
#include "lld_params.hpp"
#include "lld_tonefilt_ops.hpp"

namespace smilehip {

namespace {
constexpr int kAhead = 4;            // samples per fetch group

// the scan of one chain over n steps that start at sample index pos0 of the input, on the samples x[0 .. len), len >= 1: step k reads
// x[tonefilt::padded_index(k, len)] (the last block of an utterance repeats its last sample; n is a multiple of P and
// n - P < len <= n). Rows go to dst, dst + ld, ...
template <class PCM>
__device__ __forceinline__ void tonefilt_scan(tonefilt::State &st, const tonefilt::NoteTab nt, const PCM &x, int64_t len, int64_t n, int64_t pos0,
                                              int32_t P, double period, float *dst, int64_t ld) {
  const tonefilt::DevSinCos sc;
  double idx = (double)pos0;
  int32_t left = P;
  float cur[kAhead], nxt[kAhead];
#pragma unroll
  for (int i = 0; i < kAhead; ++i) cur[i] = x[tonefilt::padded_index(i, len)];
  for (int64_t j = 0; j < n; j += kAhead) {
#pragma unroll
    for (int i = 0; i < kAhead; ++i) {
      nxt[i] = x[tonefilt::padded_index(j + kAhead + i, len)];
    }
#pragma unroll
    for (int i = 0; i < kAhead; ++i) {
      if (j + i < n) {
        tonefilt::step(st, nt, cur[i], idx, period, sc);
        idx += 1.0;
        if (--left == 0) {
          *dst = tonefilt::emit(st);
          dst += ld;
          left = P;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kAhead; ++i) cur[i] = nxt[i];
  }
}
}  // namespace

// the chain: chains [0, n_utt n_notes), 64 per workgroup
template <class PCM>
__global__ void __launch_bounds__(64) lld_tonefilt_scan(TonefiltParams Q, PCM pcm) {
  const int64_t g = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (g >= (int64_t)Q.n_utt * Q.n_notes) return;
  const int32_t u = (int32_t)(g / Q.n_notes), t = (int32_t)(g - (int64_t)u * Q.n_notes);
  const int64_t row0 = Q.frame_off[u], rows = Q.frame_off[u + 1] - row0;
  if (rows <= 0) return;
  tonefilt::State st = {0.0, 0.0};
  const int64_t s0 = Q.samp_off[u], len = Q.samp_off[u + 1] - s0;   // (rows > 0: len >= 1)
  tonefilt_scan(st, Q.tab[t], pcm + s0, len, rows * (int64_t)Q.P, 0, Q.P, Q.period, Q.tonespec + row0 * Q.n_notes + t, Q.n_notes);
}

// the operator: one lane per note, state in global memory
__global__ void __launch_bounds__(64) lld_tonefilt_blocks(TonefiltParams Q, const float *samples, int64_t n_blocks, int64_t pos0,
                                                          tonefilt::State *state, float *dst) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= Q.n_notes) return;
  tonefilt::State st = state[t];
  PcmF32In x;
  x.f = samples;
  tonefilt_scan(st, Q.tab[t], x, n_blocks * (int64_t)Q.P, n_blocks * (int64_t)Q.P, pos0, Q.P, Q.period, dst + t, Q.n_notes);
  state[t] = st;
}

// sincos_d on n doubles (smilehip_sincos_d_values: tests / diagnostics)
__global__ void __launch_bounds__(256) lld_sincos_d_values(const double *x, int64_t n, double *sn, double *cs) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const SinCosD v = sincos_d(x[i]);
  sn[i] = v.s;
  cs[i] = v.c;
}

hipError_t stage_sincos_d(const double *x, int64_t n, double *sn, double *cs, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (!x || !sn || !cs || (n + 255) / 256 > 0x7fffffffLL) return hipErrorInvalidValue;
  SMILEHIP_KLAUNCH(lld_sincos_d_values, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, sn, cs);
  return hipGetLastError();
}

static bool tonefilt_params_ok(const TonefiltParams &Q) {
  return Q.tab && Q.n_notes >= 1 && Q.n_notes <= tonefilt::kMaxNotes && Q.P >= 1 && Q.period > 0.0;
}

hipError_t launch_tonefilt(const TonefiltParams &Q, const int16_t *pcm, const float *pcm_f32, hipStream_t s) {
  if (Q.n_utt <= 0 || Q.total_frames <= 0) return hipSuccess;
  if (!tonefilt_params_ok(Q) || !Q.samp_off || !Q.frame_off || !Q.tonespec || !(pcm || pcm_f32)) return hipErrorInvalidValue;
  const int64_t chains = (int64_t)Q.n_utt * Q.n_notes, grid = (chains + 63) / 64;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  if (pcm_f32) {
    PcmF32In p; p.f = pcm_f32;
    SMILEHIP_KLAUNCH((lld_tonefilt_scan<PcmF32In>), dim3((unsigned)grid), dim3(64), 0, s, Q, p);
  } else {
    Pcm16In p; p.s = pcm;
    SMILEHIP_KLAUNCH((lld_tonefilt_scan<Pcm16In>), dim3((unsigned)grid), dim3(64), 0, s, Q, p);
  }
  return hipGetLastError();
}

hipError_t stage_tonefilt_blocks(const TonefiltParams &Q, const float *samples, int64_t n_blocks, int64_t pos0, tonefilt::State *state,
                                 float *dst, hipStream_t s) {
  if (n_blocks <= 0) return hipSuccess;
  if (!tonefilt_params_ok(Q) || !samples || !state || !dst || pos0 < 0) return hipErrorInvalidValue;
  SMILEHIP_KLAUNCH(lld_tonefilt_blocks, dim3((unsigned)((Q.n_notes + 63) / 64)), dim3(64), 0, s, Q, samples, n_blocks, pos0, state, dst);
  return hipGetLastError();
}

}  // namespace smilehip
