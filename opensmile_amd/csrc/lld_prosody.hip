// config/prosody/prosodyShs.conf behind cPitchShs (SMILEHIP_CHAIN_PROSODY_SHS): cPitchSmoother, cIntensity and cContourSmoother as
// ONE kernel over the output rows. The frame kernels in front of it are the F0 group's (lld_f0.hip: lld_f0_spec, lld_f0_sweep,
// lld_f0_cand), which leave the cPitchShs rows of every frame in F0Params::shs.
//
// An output row is a function of a few frames of ONE utterance (lld_prosody_ops.hpp says why that holds for cPitchSmoother's
// one-frame-delay smoother too, and what the rows are): the rows are independent. One lane per output row, a workgroup per tile
// of 128 rows of one utterance (the window-chain kernel's tiles: the utterance and the tile's first row are two wave-uniform
// loads, no search). Each lane forms what it needs itself: per smoothed position three replayed smoother calls (two floats of a
// candidate row each) and one PCM sample with one double pow. Handing neighbours' values across lanes would save two of three
// of them and cost an LDS round trip the kernel does not otherwise need; the kernel is a few thousandths of the chain's time
// (DESIGN.md). No LDS, no scratch: nothing is indexed by a lane-dependent value but global memory.
#include <hip/hip_runtime.h>

#include "kernel_timing.hpp"
#include "lld_launch.hpp"
#include "lld_params.hpp"
#include "lld_prosody_ops.hpp"

namespace smilehip {

namespace {
constexpr int kTailRows = 128;                            // = chain_tile_rows(): rows per workgroup

template <class PCM>
__device__ __forceinline__ void prosody_tail_body(const ProsodyParams &R, const PCM &pcm) {
  const int tile = (int)blockIdx.x;
  const int u = R.tile_utt[tile];                        // (wave-uniform)
  const int n = R.tile_t0[tile] + (int)threadIdx.x;      // this lane's row within the utterance
  const int64_t f0 = R.frame_off[u], r0 = R.row_off[u];
  const int T = (int)(R.frame_off[u + 1] - f0);
  const int rows = (int)(R.row_off[u + 1] - r0);
  if (T < 2 || n >= rows) return;
  prosody::RowConsts c;
  c.voicing_cutoff = R.voicing_cutoff; c.W = R.W; c.H = R.H; c.reserved = 0; c.win0 = R.win0; c.win_sum = R.win_sum;
  float o3[3];
  prosody::row(c, R.shs + f0 * 21, pcm + R.samp_off[u], T, n, o3);
  float *o = R.out + (r0 + n) * R.ld_out;
#pragma unroll
  for (int q = 0; q < 3; ++q) o[q] = o3[q];
}
}  // namespace

template <bool S16>
__global__ void __launch_bounds__(kTailRows) lld_prosody_tail(ProsodyParams R) {
  if constexpr (S16) { Pcm16In p; p.s = R.pcm; prosody_tail_body(R, p); }
  else { PcmF32In p; p.f = R.pcm_f32; prosody_tail_body(R, p); }
}

hipError_t launch_prosody_tail(const ProsodyParams &R, hipStream_t s) {
  if (R.n_tiles <= 0) return hipSuccess;
  if (R.W < 1 || R.W > 4 || R.H < 1 || chain_tile_rows() != kTailRows || !R.shs || !R.out || R.ld_out < 3 || !(R.pcm || R.pcm_f32))
    return hipErrorInvalidValue;
  if (R.pcm_f32) SMILEHIP_KLAUNCH(lld_prosody_tail<false>, dim3((unsigned)R.n_tiles), dim3(kTailRows), 0, s, R);
  else SMILEHIP_KLAUNCH(lld_prosody_tail<true>, dim3((unsigned)R.n_tiles), dim3(kTailRows), 0, s, R);
  return hipGetLastError();
}

}  // namespace smilehip
