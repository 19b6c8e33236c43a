// cSpecScale::processVector (src/dsp/specScale.cpp:326-377) for ANY target scale, number of target points and maxF: the general
// operator behind smilehip_specscale_op_* (the octave axis of the F0 chains keeps its own kernels, lld_f0.hip). The tables are
// make_specscale_tables' (tables.cpp); every operation below is the reference's double operation in the reference's order
// (-ffp-contract=off: no fused multiply-adds), so the rows equal the reference's bit for bit.
// Three kernels per chunk of rows, with y (the enhanced, smoothed spectrum) and u / y2 (the spline's second derivatives) as doubles
// in the operator's scratch:
//   lld_specscale_prep    a workgroup per row, lanes along the bins: (double)src, smileDsp_specEnhanceSHS, smileDsp_specSmoothSHS
//                         (src/smileutil/smileUtil.c:1965-2014) and the parallel half of smileMath_cspline (src/smileutil/
//                         smileUtilSpline.c:185): 6 * ut.
//   lld_specscale_sweep   a LANE per row, 64 rows per wave: smileMath_cspline's two recurrences (:181-202), sequential along the bins
//                         as they must be; the per-bin constants are wave-uniform (scalar loads).
//   lld_specscale_interp  a lane per target point: smileMath_csplint (:344-357), the conversion to float, the auditory weighting.
// Scratch layout: the 64 rows of a tile keep each 8-bin block side by side -- element (row r, bin i) of a chunk lies at
// (((r / 64) * nb8 + i / 8) * 64 + r % 64) * 8 + i % 8. The sweep's wave moves 4 KB of consecutive memory per block (a 64-byte
// line per lane), the row-wise kernels write and read whole 64-byte lines.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#include "lld_stage.hpp"

namespace smilehip {

__device__ __forceinline__ size_t ss_index(int64_t r, int i, int nb8) {
  return ((size_t)((r >> 6) * nb8 + (i >> 3)) * 64 + (size_t)(r & 63)) * 8 + (size_t)(i & 7);
}

// dynamic LDS: raw[n_src] floats, and with the enhancement on | enh[n_src] floats | peak[n_src] bytes (ss_prep_lds)
__global__ void __launch_bounds__(256) lld_specscale_prep(SpecScaleDev S, const float *src, int64_t ld_src, int64_t n_rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_ss[];
  __shared__ int s_cnt, s_first, s_last;
  const int n = S.n_src;
  const int64_t row = blockIdx.x;
  if (row >= n_rows) return;
  float *raw = reinterpret_cast<float *>(smem_ss);
  float *enh = raw + n;
  unsigned char *peak = reinterpret_cast<unsigned char *>(enh + n);
  const float *x = src + row * ld_src;
  if (threadIdx.x == 0) { s_cnt = 0; s_first = n; s_last = -1; }
  for (int i = threadIdx.x; i < n; i += 256) raw[i] = x[i];     // y = (double)src[i]: a float widened is exact, the row stays floats here
  __syncthreads();
  const float *e = raw;
  if (S.enhance) {
    // smileDsp_specEnhanceSHS: the local maxima (first and last bin: strict on their one side), then between two consecutive
    // maxima everything further than two bins from both is zeroed; nothing before the first or after the last. With exactly ONE
    // maximum the reference reads posmax[1] of its zero-initialised list: everything from bin 3 on is zeroed.
    int cnt = 0, first = n, last = -1;
    for (int i = threadIdx.x; i < n; i += 256) {
      bool p;
      if (i == 0) p = raw[0] > raw[1];
      else if (i == n - 1) p = raw[n - 1] > raw[n - 2];
      else p = raw[i] > raw[i - 1] && raw[i] >= raw[i + 1];
      peak[i] = p ? 1 : 0;
      if (p) { ++cnt; first = min(first, i); last = max(last, i); }
    }
    if (cnt) { atomicAdd(&s_cnt, cnt); atomicMin(&s_first, first); atomicMax(&s_last, last); }
    __syncthreads();
    cnt = s_cnt; first = s_first; last = s_last;
    for (int i = threadIdx.x; i < n; i += 256) {
      bool z = false;
      if (cnt >= 2) {
        bool near = false;
        for (int j = max(i - 2, 0); j <= min(i + 2, n - 1); ++j) near = near || peak[j];
        z = i > first && i < last && !near;
      } else if (cnt == 1) {
        z = i >= 3;
      }
      enh[i] = z ? 0.0f : raw[i];
    }
    __syncthreads();
    e = enh;
  }
  // smileDsp_specSmoothSHS: in place with the OLD left neighbour (0.0 before bin 0); the last bin is untouched
  const bool smooth = S.smooth != 0;
  const auto y_at = [&](int j) -> double {
    const double ai = (double)e[j];
    if (!smooth || j >= n - 1) return ai;
    const double aim1 = j > 0 ? (double)e[j - 1] : 0.0;
    return (aim1 + 2.0 * ai + (double)e[j + 1]) / 4.0;
  };
  const int nb8 = S.nb8;
  for (int i = threadIdx.x; i < 8 * nb8; i += 256) {
    double y0 = 0.0, u6 = 0.0;
    if (i < n) {
      y0 = y_at(i);
      if (i >= 1 && i <= n - 2) {                                // smileMath_cspline: ut, and the 6.0 * ut of u[i]
        const double ym = y_at(i - 1), yp = y_at(i + 1);
        const double ut = (yp - y0) / S.spline[5 * i + 1] - (y0 - ym) / S.spline[5 * i + 2];
        u6 = 6.0 * ut;
      }
    }
    const size_t at = ss_index(row, i, nb8);                     // (the bins that pad the last block are written too: zeros)
    S.y[at] = y0;
    S.u[at] = u6;
  }
}

// One row per lane, one 64-row tile per wave. A round is one 8-bin block: the lane's 64-byte line; the next block's line is
// requested before the current block's dependent chain runs.
constexpr int kSsSweepWaves = 4;
__global__ void __launch_bounds__(kSsSweepWaves * 64) lld_specscale_sweep(SpecScaleDev S, int64_t n_rows) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t tile = (int64_t)blockIdx.x * kSsSweepWaves + wave;
  if (tile * 64 >= n_rows) return;
  const bool active = tile * 64 + lane < n_rows;
  const int n = S.n_src, nb8 = S.nb8;
  // the tables through the constant address space (read-only for the kernel's lifetime): wave-uniform addresses, scalar loads
  typedef const __attribute__((address_space(4))) double *ConstD;
  const ConstD sp = (ConstD)(uintptr_t)S.spline;                 // [bin][5]: sigma, diff1, diff2, p, y2 of the forward sweep
  double2 *line = reinterpret_cast<double2 *>(S.u + ((size_t)tile * nb8 * 64 + lane) * 8);   // block b: + b * 256 (double2)
  const auto load = [&](double (&c)[8], int b) {
    if (active) {
#pragma unroll
      for (int q = 0; q < 4; ++q) { const double2 v = line[(size_t)b * 256 + q]; c[2 * q] = v.x; c[2 * q + 1] = v.y; }
    }
  };
  const auto store = [&](const double (&c)[8], int b) {
    if (active) {
#pragma unroll
      for (int q = 0; q < 4; ++q) line[(size_t)b * 256 + q] = make_double2(c[2 * q], c[2 * q + 1]);
    }
  };
  double cur[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, nxt[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  // u[0] = 0; u[i] = p * (6.0 * ut - sigma * u[i - 1]), i = 1 .. n-2 (smileUtilSpline.c:172-187; p and y2[i] = (sigma - 1) * p
  // do not depend on the spectrum: the table's)
  double up = 0.0;
  load(cur, 0);
  for (int b = 0; b < nb8; ++b) {
    if (b + 1 < nb8) load(nxt, b + 1);
    const int i0 = 8 * b;
    if (b > 0 && i0 + 7 <= n - 2) {
#pragma unroll
      for (int q = 0; q < 8; ++q) { const ConstD r = sp + 5 * (i0 + q); up = r[3] * (cur[q] - r[0] * up); cur[q] = up; }
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int i = i0 + q;
        if (i >= 1 && i <= n - 2) { const ConstD r = sp + 5 * i; up = r[3] * (cur[q] - r[0] * up); cur[q] = up; }
      }
    }
    store(cur, b);
#pragma unroll
    for (int q = 0; q < 8; ++q) cur[q] = nxt[q];
  }
  // natural boundary (ynp = 1e30): qn = un = 0; y2[n-1] = (un - qn * u[n-2]) / (qn * y2[n-2] + 1.0) (:189-199)
  double yn = (0.0 - 0.0 * up) / (0.0 * sp[5 * (n - 2) + 4] + 1.0);
  // y2[j] = y2[j] * y2[j + 1] + u[j], j = n-2 .. 0 (:200-202)
  load(cur, nb8 - 1);
  for (int b = nb8 - 1; b >= 0; --b) {
    if (b > 0) load(nxt, b - 1);
    const int i0 = 8 * b;
    if (i0 + 7 <= n - 2) {
#pragma unroll
      for (int q = 7; q >= 0; --q) { yn = sp[5 * (i0 + q) + 4] * yn + cur[q]; cur[q] = yn; }
    } else {
#pragma unroll
      for (int q = 7; q >= 0; --q) {
        const int i = i0 + q;
        if (i == n - 1) cur[q] = yn;
        else if (i <= n - 2) { yn = sp[5 * i + 4] * yn + cur[q]; cur[q] = yn; }
      }
    }
    store(cur, b);
#pragma unroll
    for (int q = 0; q < 8; ++q) cur[q] = nxt[q];
  }
}

// smileMath_csplint (smileUtilSpline.c:344-357), dst[i] = (FLOAT_DMEM)out[i] and the auditory weighting (specScale.cpp:352-373)
__global__ void __launch_bounds__(256) lld_specscale_interp(SpecScaleDev S, float *dst, int64_t ld_dst, int64_t n_rows, int n_blk) {
  const int64_t row = blockIdx.x / n_blk;
  const int i = (int)(blockIdx.x % n_blk) * 256 + threadIdx.x;
  if (row >= n_rows || i >= S.n_tgt) return;
  const int k = S.ip_k[i];
  const double a = S.ip_rec[4 * i], c = S.ip_rec[4 * i + 1], d = S.ip_rec[4 * i + 2];
  const double b = 1.0 - a;
  const size_t lo = ss_index(row, k, S.nb8), hi = ss_index(row, k + 1, S.nb8);
  const double out = a * S.y[lo] + b * S.y[hi] + c * S.u[lo] + d * S.u[hi];
  float v = (float)out;
  if (S.weighting) v = v > 0.0f ? (float)((double)v * S.ip_rec[4 * i + 3]) : 0.0f;
  dst[row * ld_dst + i] = v;
}

// dynamic LDS of lld_specscale_prep: the row as floats; with the enhancement also the enhanced row and the peak flags
static size_t ss_prep_lds(const SpecScaleDev &S) { return (size_t)S.n_src * (S.enhance ? 9 : 4); }

// once per operator: spectra above 5 461 bins with the enhancement on need more dynamic LDS than a kernel gets by default
hipError_t stage_specscale_general_prepare(const SpecScaleDev &S) {
  static std::mutex m;
  static size_t granted = 48 * 1024;                             // (the attribute belongs to the kernel, not to an operator: it only ever grows)
  const size_t lds = ss_prep_lds(S);
  std::lock_guard<std::mutex> lock(m);
  if (lds <= granted) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&lld_specscale_prep), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) granted = lds;
  return e;
}

hipError_t stage_specscale_general(const SpecScaleDev &S0, const float *src, int64_t ld_src, float *dst, int64_t ld_dst, int64_t n_frames,
                                   hipStream_t s) {
  if (n_frames <= 0) return hipSuccess;
  SpecScaleDev S = S0;
  const size_t lds = ss_prep_lds(S);
  const int n_blk = (S.n_tgt + 255) / 256;
  for (int64_t r0 = 0; r0 < n_frames; r0 += S.chunk_rows) {      // (the chunks of a stream follow one another: the scratch is free again)
    const int64_t nr = std::min<int64_t>(S.chunk_rows, n_frames - r0);
    hipLaunchKernelGGL(lld_specscale_prep, dim3((unsigned)nr), dim3(256), lds, s, S, src + r0 * ld_src, ld_src, nr);
    hipLaunchKernelGGL(lld_specscale_sweep, dim3((unsigned)(((nr + 63) / 64 + kSsSweepWaves - 1) / kSsSweepWaves)), dim3(kSsSweepWaves * 64), 0, s, S, nr);
    hipLaunchKernelGGL(lld_specscale_interp, dim3((unsigned)(nr * n_blk)), dim3(256), 0, s, S, dst + r0 * ld_dst, ld_dst, nr, n_blk);
  }
  return hipGetLastError();
}

}  // namespace smilehip
