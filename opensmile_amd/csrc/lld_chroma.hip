// config/chroma/chroma_fft.conf (SMILEHIP_CHAIN_CHROMA_FFT): window, transform, magnitudes, cTonespec and cChroma per frame, and the
// two components as operators on strided rows.
//
// lld_chroma_frame does, per frame: gauss window -> forward reference-order transform -> magnitudes into an LDS row ->
// chroma::tonespec_note per note (a lane owns a note and walks its run of bins in bin order: the reference's order of additions) ->
// chroma::chroma_class per class -> the double sum and the silence flag in class order, the same in every lane -> the row.
// The tonespec level goes to the batch's scratch as well (smilehip_batch_chroma_taps).
//
// Two forms, those of lld_acf_pitch_frame (lld_prosody_acf.hip):
//  * wave per frame (Nfft = 512 / 1024: 8, 11.025, 16 kHz): the transform is lld_ooura_wave.hpp's register-resident network with M
//    known at compile time, fed from global memory (consecutive lanes take consecutive sample pairs). A frame's LDS is z[M] pairs |
//    mg[M + 4] | ts[128]: 6.5 KB at M = 512. Four waves per workgroup, persistent: window, transform tables, filterMap and the note
//    records are staged once per workgroup, one barrier, none afterwards.
//    The per-note walk reads mg and filterMap at a different bin in every lane (ds_read_b32, banks by bin mod 32 within a half
//    wave): two notes whose runs start a multiple of 32 bins apart collide, one extra LDS cycle per step; the walk is as long as the
//    longest run (13 bins at 16 kHz, the top octave). With 72 notes lanes 0 .. 7 take a second note, 64 .. 71, the longest runs,
//    after their first, which are the shortest (the lowest notes have one bin or none).
//  * workgroup per frame (any other length, 2048 / 4096 at 22.05 .. 48 kHz): ooura_forward on BlockG, one thread per note.
// Every global load carries an index clamped into the frame; what lies outside is selected away afterwards.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "kernel_timing.hpp"
#include "lld_blocks.hpp"
#include "lld_chroma_ops.hpp"
#include "lld_device.hpp"
#include "lld_launch.hpp"
#include "lld_params.hpp"

namespace smilehip {

namespace {
constexpr int kChromaWaves = 4;                            // waves (= frames in flight) per workgroup of the wave form
constexpr int kTsPad = 128;                                // floats of a frame's tonespec row in LDS (chroma::kMaxNotes <= 128)
static_assert(chroma::kMaxNotes <= kTsPad && chroma::kMaxOctaveSize <= 64, "a lane per class, a row per frame");
__host__ __device__ constexpr int chroma_wave_floats(int M) { return 2 * M + (M + 4) + kTsPad; }   // z | mg | ts
__host__ __device__ inline int chroma_table_floats(int K, int n_notes) { return ((K + 3) & ~3) + 4 * ((n_notes + 3) & ~3); }   // filterMap | records

// the windowed sample pair i of the frame (R2 / R3; pad_left zeros in front with zeroPadSymmetric, zeros behind the frame)
template <class PCM>
__device__ __forceinline__ float2 chroma_load_pair(const LldParams &P, const PCM &x, const float *win, int i) {
  const int n0 = 2 * i - P.pad_left, n1 = n0 + 1, last = P.N - 1;
  const int c0 = n0 < 0 ? 0 : (n0 > last ? last : n0), c1 = n1 < 0 ? 0 : (n1 > last ? last : n1);
  const float y0 = x[c0] * win[c0] + P.win_offset, y1 = x[c1] * win[c1] + P.win_offset;
  return make_float2((n0 >= 0 && n0 <= last) ? y0 : 0.0f, (n1 >= 0 && n1 <= last) ? y1 : 0.0f);
}

// filterMap and the note records from global memory into LDS (all threads of the workgroup; the caller's barrier follows)
__device__ __forceinline__ void chroma_stage_tables(const ChromaParams &Q, int K, float *s_fmap, chroma::NoteRec *s_rec, int tid, int nthreads) {
  for (int i = tid; i < K; i += nthreads) s_fmap[i] = Q.fmap[i];
  for (int i = tid; i < Q.n_notes; i += nthreads) s_rec[i] = Q.rec[i];
}

// cChroma on the frame's tonespec row for a group of >= octave_size lanes that all hold the class sums of lanes 0 .. octave_size - 1
// in `cls` (LDS): the double sum and the flag in class order, the same in every thread; thread i < octave_size returns its value
__device__ __forceinline__ float chroma_finish(const float *cls, int octave_size, float sil_thresh, int i) {
  double sum = 0.0;
  bool sil = false;
  for (int c = 0; c < octave_size; ++c) {
    const float v = cls[c];
    sil = sil || v < sil_thresh;
    sum += (double)v;
  }
  const float d = cls[i < octave_size ? i : 0];
  return (sum != 0.0 && !sil) ? d / (float)sum : 0.0f;
}

template <class PCM, int MC>
__device__ __forceinline__ void chroma_frame_wave(const LldParams &P, const ChromaParams &Q, const PCM &pcm, const float *win,
                                                  const OouraTab &oo, const float *fmap, const chroma::NoteRec *rec, int64_t row, float *wm) {
  constexpr int M = MC;
  float2 *z = reinterpret_cast<float2 *>(wm);
  float *mg = wm + 2 * M;
  float *ts = mg + (M + 4);
  const int lane = threadIdx.x & 63;
  const int u = P.frame_utt[row];                          // (wave-uniform)
  const int64_t t = row - P.frame_off[u];
  const PCM x = pcm + (P.samp_off[u] + t * (int64_t)P.H);
  oo_wave_forward<MC>(z, oo, lane, [&](int i) { return chroma_load_pair(P, x, win, i); });
  for (int k = lane; k <= M; k += 64) mg[k] = bin_magnitude(oo_wave_bin<MC>(z, oo, k), k == 0 || k == M);   // R5
  WaveG::sync();
  for (int note = lane; note < Q.n_notes; note += 64) {
    const float v = chroma::tonespec_note(mg, fmap, rec[note], Q.use_power);
    ts[note] = v;
    Q.tonespec[row * (int64_t)Q.n_notes + note] = v;
  }
  WaveG::sync();
  const int n_oct = Q.n_notes / Q.octave_size;
  const float d = lane < Q.octave_size ? chroma::chroma_class(ts, n_oct, Q.octave_size, lane) : 0.0f;
  WaveG::sync();                                           // (the class sums replace the head of ts)
  if (lane < Q.octave_size) ts[lane] = d;
  WaveG::sync();
  const float o = chroma_finish(ts, Q.octave_size, Q.sil_thresh, lane);
  if (lane < Q.octave_size) P.out[row * P.ld_out + lane] = o;
  WaveG::sync();                                           // (the wave's next frame writes these buffers)
}
}  // namespace

// one WAVE per frame, persistent workgroups of kChromaWaves waves; LDS: window | transform tables | filterMap | records | frame buffers
template <class PCM, int MC>
__global__ void __launch_bounds__(kChromaWaves * 64) lld_chroma_frame_wave(LldParams P, ChromaParams Q, PCM pcm) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int Npad = (P.N + 3) & ~3, Kpad = (P.K + 3) & ~3;
  float *s_win = smem;
  for (int i = threadIdx.x; i < P.N; i += kChromaWaves * 64) s_win[i] = P.window[i];
  float *s_oo = smem + Npad;
  const OouraTab oo = oo_stage_tables(P.oo, s_oo, threadIdx.x, kChromaWaves * 64);
  float *s_fmap = s_oo + oo_table_floats(P.oo);
  chroma::NoteRec *s_rec = reinterpret_cast<chroma::NoteRec *>(s_fmap + Kpad);
  chroma_stage_tables(Q, P.K, s_fmap, s_rec, threadIdx.x, kChromaWaves * 64);
  __syncthreads();                                         // the only workgroup barrier
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float *wm = s_fmap + chroma_table_floats(P.K, Q.n_notes) + wave * chroma_wave_floats(MC);
  const int64_t stride = (int64_t)gridDim.x * kChromaWaves;
  for (int64_t row = (int64_t)blockIdx.x * kChromaWaves + wave; row < P.total_frames; row += stride)
    chroma_frame_wave<PCM, MC>(P, Q, pcm, s_win, oo, s_fmap, s_rec, row, wm);
}

// one WORKGROUP per frame (any transform length the LDS holds); LDS: z[M] pairs | mg[Kpad] | ts[kTsPad]; the tables stay in global memory
template <class PCM>
__global__ void __launch_bounds__(256) lld_chroma_frame_block(LldParams P, ChromaParams Q, PCM pcm) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int M = P.Nfft >> 1, Kpad = (P.K + 3) & ~3;
  float2 *z = reinterpret_cast<float2 *>(smem);
  float *mg = smem + 2 * M;
  float *ts = mg + Kpad;
  const int64_t row = (int64_t)blockIdx.x;
  const int u = P.frame_utt[row];
  const int64_t t = row - P.frame_off[u];
  const PCM x = pcm + (P.samp_off[u] + t * (int64_t)P.H);
  ooura_forward<BlockG>(z, P.oo, [&](int i) { return chroma_load_pair(P, x, P.window, i); });
  for (int k = threadIdx.x; k <= M; k += 256) mg[k] = bin_magnitude(ooura_bin(z, P.oo, k), k == 0 || k == M);   // R5
  __syncthreads();
  const int tid = threadIdx.x;
  if (tid < Q.n_notes) {
    const float v = chroma::tonespec_note(mg, Q.fmap, Q.rec[tid], Q.use_power);
    ts[tid] = v;
    Q.tonespec[row * (int64_t)Q.n_notes + tid] = v;
  }
  __syncthreads();
  const int n_oct = Q.n_notes / Q.octave_size;
  const float d = tid < Q.octave_size ? chroma::chroma_class(ts, n_oct, Q.octave_size, tid) : 0.0f;
  __syncthreads();
  if (tid < Q.octave_size) ts[tid] = d;
  __syncthreads();
  if (tid < Q.octave_size) P.out[row * P.ld_out + tid] = chroma_finish(ts, Q.octave_size, Q.sil_thresh, tid);
}

// ---- the operators: rows of magnitudes -> rows of notes (one thread per note), rows of notes -> rows of classes (one thread per row)
__global__ void __launch_bounds__(128) lld_tonespec_rows(const float *fmap, const chroma::NoteRec *rec, int n_notes, int use_power,
                                                         const float *src, int64_t ld_src, float *dst, int64_t ld_dst) {
  const int64_t row = (int64_t)blockIdx.x;
  const int note = threadIdx.x;
  if (note < n_notes) dst[row * ld_dst + note] = chroma::tonespec_note(src + row * ld_src, fmap, rec[note], use_power);
}
__global__ void __launch_bounds__(64) lld_chroma_rows(int n_src, int octave_size, float sil_thresh, const float *src, int64_t ld_src, float *dst,
                                                      int64_t ld_dst, int64_t n_frames) {
  const int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (row < n_frames) chroma::chroma_row(src + row * ld_src, n_src, octave_size, sil_thresh, dst + row * ld_dst);
}

namespace {
size_t chroma_wave_lds_bytes(const LldParams &P, const ChromaParams &Q, int M) {
  return sizeof(float) * ((size_t)((P.N + 3) & ~3) + (size_t)oo_table_floats(P.oo) + (size_t)chroma_table_floats(P.K, Q.n_notes) +
                          (size_t)kChromaWaves * chroma_wave_floats(M));
}
template <class PCM, int MC>
hipError_t launch_wave(const LldParams &P, const ChromaParams &Q, const PCM &pcm, hipStream_t s) {
  const size_t bytes = chroma_wave_lds_bytes(P, Q, MC);
  if (bytes > 160 * 1024) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&lld_chroma_frame_wave<PCM, MC>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return e;
  int64_t grid = (P.total_frames + kChromaWaves - 1) / kChromaWaves;
  const int64_t cap = chroma_wave_grid_cap(current_device_cus(), (int64_t)bytes);
  if (grid > cap) grid = cap;
  SMILEHIP_KLAUNCH((lld_chroma_frame_wave<PCM, MC>), dim3((unsigned)grid), dim3(kChromaWaves * 64), bytes, s, P, Q, pcm);
  return hipGetLastError();
}
template <class PCM>
hipError_t launch_block(const LldParams &P, const ChromaParams &Q, const PCM &pcm, hipStream_t s) {
  const int M = P.Nfft / 2, Kpad = (P.K + 3) & ~3;
  const size_t bytes = sizeof(float) * (size_t)(2 * M + Kpad + kTsPad);
  if (bytes > 160 * 1024) return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&lld_chroma_frame_block<PCM>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return e;
  SMILEHIP_KLAUNCH((lld_chroma_frame_block<PCM>), dim3((unsigned)P.total_frames), dim3(256), bytes, s, P, Q, pcm);
  return hipGetLastError();
}
template <class PCM>
hipError_t launch_frames(const LldParams &P, const ChromaParams &Q, const PCM &pcm, hipStream_t s) {
  // SMILEHIP_CHROMA=block (A/B switch, tools/chroma_timing.py): the workgroup form where the wave form would run
  const char *form = getenv("SMILEHIP_CHROMA");
  const bool block = form && !strcmp(form, "block");
  if (P.Nfft == 1024 && !block) return launch_wave<PCM, 512>(P, Q, pcm, s);
  if (P.Nfft == 512 && !block) return launch_wave<PCM, 256>(P, Q, pcm, s);
  return launch_block<PCM>(P, Q, pcm, s);
}
}  // namespace

// persistent workgroups: as many as the LDS admits per CU, four waves per SIMD at most
int64_t chroma_wave_grid_cap(int n_cu, int64_t lds_bytes) {
  int64_t per_cu = lds_bytes > 0 ? (int64_t)(160 * 1024) / lds_bytes : 1;
  if (per_cu > 16 / kChromaWaves) per_cu = 16 / kChromaWaves;
  if (per_cu < 1) per_cu = 1;
  return (int64_t)(n_cu > 0 ? n_cu : 256) * per_cu;
}

hipError_t launch_chroma(const LldParams &P, const ChromaParams &Q, hipStream_t s) {
  if (P.total_frames <= 0) return hipSuccess;
  if (!P.oo.tw || !P.frame_utt || !P.window || !P.out || !Q.tonespec || !Q.fmap || !Q.rec || !(P.pcm || P.pcm_f32)) return hipErrorInvalidValue;
  if (P.Nfft < 64 || P.Nfft > 8192 || P.N < 1 || P.N > P.Nfft || P.K != P.Nfft / 2 + 1 || P.oo.M != P.Nfft / 2 ||
      P.pad_left < 0 || P.pad_left + P.N > P.Nfft || P.total_frames > 0x7fffffffLL)
    return hipErrorInvalidValue;
  if (Q.n_notes < 1 || Q.n_notes > chroma::kMaxNotes || Q.octave_size < 1 || Q.octave_size > chroma::kMaxOctaveSize ||
      Q.n_notes % Q.octave_size || P.ld_out < Q.octave_size)
    return hipErrorInvalidValue;
  if (P.pcm_f32) { PcmF32In p; p.f = P.pcm_f32; return launch_frames(P, Q, p, s); }
  Pcm16In p; p.s = P.pcm;
  return launch_frames(P, Q, p, s);
}

hipError_t stage_tonespec(const float *fmap, const chroma::NoteRec *rec, int n_src, int n_notes, int use_power, const float *src, int64_t ld_src,
                          float *dst, int64_t ld_dst, int64_t n_frames, hipStream_t s) {
  if (n_frames <= 0) return hipSuccess;
  if (n_notes < 1 || n_notes > 128 || n_frames > 0x7fffffffLL || ld_src < n_src || ld_dst < n_notes) return hipErrorInvalidValue;
  SMILEHIP_KLAUNCH(lld_tonespec_rows, dim3((unsigned)n_frames), dim3(128), 0, s, fmap, rec, n_notes, use_power, src, ld_src, dst, ld_dst);
  return hipGetLastError();
}

hipError_t stage_chroma(int n_src, int octave_size, float sil_thresh, const float *src, int64_t ld_src, float *dst, int64_t ld_dst,
                        int64_t n_frames, hipStream_t s) {
  if (n_frames <= 0) return hipSuccess;
  if (octave_size < 1 || n_src < octave_size || n_src % octave_size || ld_src < n_src || ld_dst < octave_size) return hipErrorInvalidValue;
  SMILEHIP_KLAUNCH(lld_chroma_rows, dim3((unsigned)((n_frames + 63) / 64)), dim3(64), 0, s, n_src, octave_size, sil_thresh, src, ld_src, dst,
                   ld_dst, n_frames);
  return hipGetLastError();
}

}  // namespace smilehip
