// Block-level (256 threads, Nfft = 512) building blocks of the ComParE descriptors, shared by the
// fused kernel (lld_compare.hip) and the per-component operators (lld_stage2_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "lld_params.hpp"

namespace smilehip {

// sums of NV doubles over the 256 threads of the block (4 waves); every thread gets the totals.
// red: 4*NV doubles of LDS. The order differs from the reference's sequential loops, the
// accumulator type (double) does not.
template <int NV>
__device__ __forceinline__ void block_sum_n(double (&v)[NV], double *red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_down(v[i], off, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) red[wave * NV + i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = ((red[i] + red[NV + i]) + red[2 * NV + i]) + red[3 * NV + i];
  __syncthreads();
}

// Two float sums in index order, one addition after the other -- what the reference's FLOAT_DMEM accumulators do (sharpness
// spectral.cpp:1435-1471, harmonicity :1485-1499, alpha ratio :997-1022). A float sum cannot be re-associated without changing
// its bits, so ONE thread walks the terms (the two chains interleave: two independent dependency chains); n a multiple of 4,
// a and b 16-byte aligned.
__device__ __forceinline__ void seq_sum2_f32(const float *a, const float *b, int n, float &s0, float &s1) {
  float x = 0.0f, y = 0.0f;
  float4 u = *reinterpret_cast<const float4 *>(a), v = *reinterpret_cast<const float4 *>(b);
  for (int i = 4; i <= n; i += 4) {
    float4 un = u, vn = v;                               // the next block's loads are in flight while this block's adds run
    if (i < n) { un = *reinterpret_cast<const float4 *>(a + i); vn = *reinterpret_cast<const float4 *>(b + i); }
    x += u.x; y += v.x;
    x += u.y; y += v.y;
    x += u.z; y += v.z;
    x += u.w; y += v.w;
    u = un; v = vn;
  }
  s0 = x; s1 = y;
}

// sum of x[lo .. hi) in index order, one float addition after the other; the loads run a few elements ahead of the adds
__device__ __forceinline__ float seq_sum_f32(const float *x, int lo, int hi) {
  float s = 0.0f;
  int i = lo;
  for (; i < hi && (i & 3); ++i) s += x[i];
  if (i + 4 <= hi) {
    float4 u = *reinterpret_cast<const float4 *>(x + i);
    for (i += 4; i + 4 <= hi; i += 4) {
      const float4 un = *reinterpret_cast<const float4 *>(x + i);
      s += u.x; s += u.y; s += u.z; s += u.w;
      u = un;
    }
    s += u.x; s += u.y; s += u.z; s += u.w;
  }
  for (; i < hi; ++i) s += x[i];
  return s;
}

// cSpectral's double sums fall in two classes (tests/golden/order_witnesses.npz holds spectra that tell the orders apart,
// tests/test_gpu_order_witnesses.py runs them):
//   sequence-decided  sums whose ORDER can move the float result by more than an ulp, so they are added bin after bin like the
//                     reference's loops, by one thread: the third central moment (skewness, spectral.cpp:1344-1364: on a flat
//                     spectrum its terms cancel and the order decides every bit); frameSum = sumB and the centroid numerator sumA
//                     (:762-767, :1093-1097, :1256-1311: the slope N sumA - Sf sumB cancels on a mirrored spectrum, the float
//                     centroid feeds every moment -- d m3 / d ctr = -3 m2 --, and the running sumB is compared with a share of
//                     its own total for the roll-off points, :1102-1122, where one ulp of a double moves the result by a bin)
//   one-signed        band energies, flux, entropy, second and fourth moment: sums of non-negative terms that keep their fixed
//                     trees. A tree and the chain differ by at most K 2^-53 relative, the float results are equal or adjacent:
//                     within ONE float ulp of the reference, bit-equal except where the exact value lies within ~1e-16 of a float
//                     rounding midpoint.
// sum of x[0 .. n) in index order, one double addition after the other (n even, x 16-byte aligned); the loads run a block ahead.
// (What the chains cost -- registers, occupancy, step time: DESIGN.md 4.3, profiles/order_chains_kernel_resources_diff.txt.)
__device__ __forceinline__ double seq_sum_f64(const double *x, int n) {
  double s = 0.0;
  double2 u = *reinterpret_cast<const double2 *>(x);
  for (int i = 2; i <= n; i += 2) {
    double2 un = u;                                      // the next block's load is in flight while this block's adds run
    if (i < n) un = *reinterpret_cast<const double2 *>(x + i);
    s += u.x;
    s += u.y;
    u = un;
  }
  return s;
}

// frameSum (= sumB) and the centroid numerator sumA in the reference's order, with every running value of sumB kept: ONE thread
// walks the bins, the two chains interleaved. pw1[i]: the power of bin i + 1; x[0 .. n): on entry the terms fj p of bins 1 .. n
// (formed by all threads), on return the inclusive prefix of the powers, x[i] = p_1 + .. + p_(i+1) as the reference's running sumC
// holds it after bin i + 1 (the same additions as sumB's, so x[n - 1] == sumB). n a multiple of 4, x 16-byte aligned; the loads run
// a block ahead of the adds.
__device__ __forceinline__ void seq_chains_f64(const float *pw1, double *x, int n, double &sumB, double &sumA) {
  double sb = 0.0, sa = 0.0;
  double2 a0 = *reinterpret_cast<const double2 *>(x), a1 = *reinterpret_cast<const double2 *>(x + 2);
  float p0 = pw1[0], p1 = pw1[1], p2 = pw1[2], p3 = pw1[3];
  for (int i = 4; i <= n; i += 4) {
    double2 b0 = a0, b1 = a1;
    float q0 = p0, q1 = p1, q2 = p2, q3 = p3;
    if (i < n) {
      b0 = *reinterpret_cast<const double2 *>(x + i); b1 = *reinterpret_cast<const double2 *>(x + i + 2);
      q0 = pw1[i]; q1 = pw1[i + 1]; q2 = pw1[i + 2]; q3 = pw1[i + 3];
    }
    double2 c0, c1;
    sb += (double)p0; sa += a0.x; c0.x = sb;
    sb += (double)p1; sa += a0.y; c0.y = sb;
    sb += (double)p2; sa += a1.x; c1.x = sb;
    sb += (double)p3; sa += a1.y; c1.y = sb;
    *reinterpret_cast<double2 *>(x + i - 4) = c0;
    *reinterpret_cast<double2 *>(x + i - 2) = c1;
    a0 = b0; a1 = b1; p0 = q0; p1 = q1; p2 = q2; p3 = q3;
  }
  sumB = sb; sumA = sa;
}

// The same two chains where there is no room for the sumA terms: the thread forms fj p = (F0 j) p itself. x[0 .. n) receives the
// running sumB; pw1 may lie INSIDE x's memory as long as (float *)(x + i) <= pw1 + i + 4 for every i <= n (the powers of a block are
// read before the previous block's running sums are written).
__device__ __forceinline__ void seq_chains_axis_f64(const float *pw1, double F0, double *x, int n, double &sumB, double &sumA) {
  double sb = 0.0, sa = 0.0, jd = 1.0;
  float p0 = pw1[0], p1 = pw1[1], p2 = pw1[2], p3 = pw1[3];
  for (int i = 4; i <= n; i += 4) {
    float q0 = p0, q1 = p1, q2 = p2, q3 = p3;
    if (i < n) { q0 = pw1[i]; q1 = pw1[i + 1]; q2 = pw1[i + 2]; q3 = pw1[i + 3]; }
    double2 c0, c1;
    sb += (double)p0; sa += (F0 * jd) * (double)p0; c0.x = sb; jd += 1.0;
    sb += (double)p1; sa += (F0 * jd) * (double)p1; c0.y = sb; jd += 1.0;
    sb += (double)p2; sa += (F0 * jd) * (double)p2; c1.x = sb; jd += 1.0;
    sb += (double)p3; sa += (F0 * jd) * (double)p3; c1.y = sb; jd += 1.0;
    *reinterpret_cast<double2 *>(x + i - 4) = c0;
    *reinterpret_cast<double2 *>(x + i - 2) = c1;
    p0 = q0; p1 = q1; p2 = q2; p3 = q3;
  }
  sumB = sb; sumA = sa;
}

// R11 cSpectral::processVector with ComParE_2016's option set ([is13_spectral]: bands 250-650 and
// 1000-4000, roll-off .25/.5/.75/.9, flux, centroid, entropy, variance, skewness, kurtosis, slope,
// sharpness, harmonicity; squareInput = 1, freqRange 0-0, oldSlopeScale = 1; spectral.cpp:586-1560).
// Thread i of 256 owns bin j = i+1. mg / pw: magnitudes and powers of the K = 257 bins, prev: the
// previous frame's magnitudes (ignored when first). red: 64 doubles, cum: 256 doubles, pk_val[4],
// pk_has[4] of LDS scratch. Writes sp[0..14]; thread 0 returns valid frameSum-based values; ends
// with a block barrier. The sums are double like the reference's: the sequence-decided ones added bin after bin by thread 0
// (seq_chains_f64, seq_sum_f64), the one-signed ones combined in a fixed tree order (the two classes: above seq_sum_f64).
__device__ __forceinline__ void spectral_frame(const float *mg, const float *pw, const float *prev, bool first,
                                               const SpectralConsts &C, int K, double *red, double *cum, float *pk_val,
                                               int *pk_has, float *sp) {
  const double F0 = 1.0 / C.fsSec;
  const int lo = 1, hi = K - 1, nBins = K - 1;          // freqRange 0-0 (spectral.cpp:625-627)
  const int tid = threadIdx.x, j = tid + 1;
  const int lane = tid & 63, wave = tid >> 6;
  const float pf = pw[j];
  const double p = (double)pf, fj = F0 * j;
  // frame energy (:762-767) = centroid denominator, centroid numerator (:1256-1330) and the roll-off prefix: the reference's chains
  cum[tid] = fj * p;
  __syncthreads();
  if (tid == 0) {
    double sb, sa;
    seq_chains_f64(pw + 1, cum, 256, sb, sa);
    red[62] = sb; red[63] = sa;                         // (block_sum_n uses red[0 .. 4 NV); its barriers publish these and cum)
  }
  double v1[3];
  { const double myB = (double)mg[j] - (double)prev[j]; v1[0] = first ? 0.0 : myB * myB; }   // flux (:1124-1254)
#pragma unroll
  for (int b = 0; b < 2; ++b) {                         // band energies (:779-853), edges resolved on the host
    auto part = [&](int k) {
      const double pk = (double)pw[k];
      double c = 0.0;
      if (k == C.band_iL[b]) c += pk * C.band_wL[b];
      if (k > C.band_iL[b] && k < C.band_iR[b]) c += pk;
      if (k == C.band_iR[b]) c += pk * C.band_wR[b];
      return c;
    };
    v1[1 + b] = part(j) + (tid == 0 ? part(0) : 0.0);
  }
  block_sum_n<3>(v1, red);
  const double frameSum = red[62], sumA = red[63];
  float ctr = 0.0f;
  if (frameSum != 0.0) ctr = (float)(sumA / frameSum);
  // roll-off (:1102-1122): the first bin whose running sum reaches the share (the running sum never falls: one bin at most)
  {
    const double c = cum[tid];
    const double before = tid ? cum[tid - 1] : -1.0;
    const double rollOff[4] = {0.25, 0.50, 0.75, 0.90};
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const double th = rollOff[i] * frameSum;
      if (c >= th && (tid == 0 || !(before >= th))) sp[2 + i] = (float)(F0 * j);
    }
  }
  // harmonicity (:1484-1513): alternating peaks/valleys, distance to the previous one
  float hc = 0.0f;
  {
    bool flag = false;
    if (j >= lo + 2 && j < hi - 1)
      flag = (pw[j - 2] < pf && pw[j - 1] < pf && pf > pw[j + 1] && pf > pw[j + 2]) ||
             (pw[j - 2] > pf && pw[j - 1] > pf && pf < pw[j + 1] && pf < pw[j + 2]);
    const unsigned long long mask = __ballot(flag);
    const unsigned long long lower = mask & ((1ull << lane) - 1ull);
    const int src = lower ? 63 - __clzll(lower) : 0;
    const float prevw = __shfl(pf, src, 64);
    if (mask && lane == 63 - __clzll(mask)) pk_val[wave] = pf;
    if (lane == 0) pk_has[wave] = mask != 0ull;
    __syncthreads();
    if (flag) {
      if (lower) hc = fabsf(pf - prevw);
      else
        for (int w = wave - 1; w >= 0; --w)
          if (pk_has[w]) { hc = fabsf(pf - pk_val[w]); break; }
    }
  }
  double v2[5], m3t;
  {                                                     // entropy (smileStat_entropy, smileUtil.c:2079-2124; powers: min = 0)
    const double entropy_floor = 0.0000001;
    double dn = frameSum;
    if (dn < (float)entropy_floor) dn = (float)entropy_floor;
    double v = p;
    if (v <= entropy_floor) v = entropy_floor;
    const double ln = v / dn;
    v2[0] = (ln > 0.0) ? ln * log_d(ln) / log(2.0) : 0.0;
    const double t1 = fj - (double)ctr;                 // moments (:1338-1397)
    double m = t1 * t1 * p;
    v2[1] = m; m *= t1; m3t = m; v2[3] = m * t1;
    v2[2] = 0.0;                                        // (third moment: a double chain, below)
    v2[4] = 0.0;                                        // (harmonicity: a float chain, below)
  }
  // sharpness and harmonicity accumulate in FLOAT_DMEM, bin after bin: the terms go to LDS (cum is free after the roll-off:
  // the barrier of the harmonicity section lies behind its last read), thread 0 adds them in order
  float *chain = reinterpret_cast<float *>(cum);
  chain[tid] = (float)(C.sharp_w[tid] * p);             // (FLOAT_DMEM)(sharpnessWeights[j - lo] * (double)srcP[j]), :1455 / :1469
  chain[256 + tid] = hc;                                // |srcLP[j] - lastPeak| of a flagged bin, +0 elsewhere (s + 0 = s), :1493
  block_sum_n<5>(v2, red);
  float sumAA_seq = 0.0f, ptp_seq = 0.0f;
  if (tid == 0) seq_sum2_f32(chain, chain + 256, 256, sumAA_seq, ptp_seq);
  __syncthreads();                                      // (the float chains are consumed: the third moment's terms take their place)
  cum[tid] = m3t;
  __syncthreads();
  if (tid == 0) {
    const double mom3 = seq_sum_f64(cum, 256);
    sp[0] = (float)(v1[1] / (double)nBins);
    sp[1] = (float)(v1[2] / (double)nBins);
    float c2 = 0.0f;
    const float sumAA = sumAA_seq;
    if (frameSum != 0.0) c2 = (float)(sumAA / frameSum);
    sp[13] = (float)(0.11 * c2);
    const double flux = v1[0] / (double)nBins;
    sp[6] = (!first && flux > 0.0) ? (float)sqrt(flux) : 0.0f;
    sp[7] = ctr;
    sp[8] = (float)(-v2[0]);
    const double sumB = frameSum;
    const double sigma2 = (sumB != 0.0) ? v2[1] / sumB : 0.0;
    sp[9] = (float)sigma2;
    sp[10] = (sigma2 <= 0.0) ? 0.0f : (float)(mom3 / (sumB * sigma2 * sqrt(sigma2)));
    sp[11] = (sigma2 == 0.0) ? 0.0f : (float)(v2[3] / (sumB * sigma2 * sigma2));
    const double Nind = (double)nBins;
    const double deno = (Nind * C.slope_S2f - C.slope_Sf * C.slope_Sf);
    double slope = 0.0;
    if (deno != 0.0) slope = (Nind * sumA - C.slope_Sf * sumB) / deno;
    sp[12] = (float)(slope * (Nind - 1.0));              // oldSlopeScale = 1
    float ptpSum = ptp_seq;
    ptpSum /= 2.0f;
    ptpSum /= (float)nBins;
    sp[14] = ptpSum;
  }
  __syncthreads();
}

// ---- the same sums with ONE wave per frame: lane l plays the four threads l, l+64, l+128, l+192 of the block version
// (index w = the block version's wave), so every reduction keeps the block version's tree: shuffle-down inside each group
// of 64, then ((s0 + s1) + s2) + s3 -- the results are bit-identical to block_sum_n / spectral_frame.
template <int NV>
__device__ __forceinline__ void wave_sum4(const double (&v)[4][NV], double (&tot)[NV]) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const double t = ((v[0][i] + v[1][i]) + v[2][i]) + v[3][i];      // (the lane's four terms first, then one tree: see wave_sumw)
    tot[i] = wave_first_d(wave_tree_d(t, [](double a, double b) { return a + b; }));
  }
}

// spectral_frame for one wave, K = 64 W + 1 bins (W = 4: the 512-point spectrum of 20 ms frames at 16 kHz, the tuned case; W = 2 / 8:
// the 256- / 1024-point spectra of other sample rates): no LDS scratch, no barriers. mg / pw / prev as above; sp[0..14] written
// by lane 0 (roll-off points by the lane that owns the crossing bin).
// chain: 128 W floats of LDS scratch (16-byte aligned): the sumA terms / the running sumB, then the two float chains, then the
// third moment's terms.
// (The two classes of sums: above seq_sum_f64. The sequence-decided ones -- frameSum, sumA with the roll-off prefix, the third
// moment -- are added bin after bin by lane 0; the one-signed ones keep a tree. Round 3: the lane's W terms are added first and ONE
// wave tree follows per quantity -- a quarter of the reductions of the block form's per-group trees, which cost ~1200 of the
// kernel's ~4000 instruction slots per frame.)
template <int NV, int W>
__device__ __forceinline__ void wave_sumw(const double (&v)[W][NV], double (&tot)[NV]) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    double t = v[0][i];
#pragma unroll
    for (int w = 1; w < W; ++w) t += v[w][i];
    tot[i] = wave_first_d(wave_tree_d(t, [](double a, double b) { return a + b; }));   // the shuffle-down tree, lld_blocks.hpp
  }
}
template <int W>
__device__ __forceinline__ void spectral_frame_wave(const float *mg, const float *pw, const float *prev, bool first,
                                                    const SpectralConsts &C, int K, float *chain, float *sp) {
  const double F0 = 1.0 / C.fsSec;
  const int lo = 1, hi = K - 1, nBins = K - 1;
  const int lane = threadIdx.x & 63;
  float pf[W], tsh[W];
  double p[W], fj[W], v1[W][3];
  double *chain_d = reinterpret_cast<double *>(chain);
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const int tid = lane + 64 * w, j = tid + 1;
    pf[w] = pw[j];
    p[w] = (double)pf[w];
    fj[w] = F0 * j;
    chain_d[tid] = fj[w] * p[w];                        // centroid numerator terms, for lane 0's chain
    tsh[w] = (float)(C.sharp_w[tid] * p[w]);            // sharpness term, :1455 / :1469
    { const double myB = (double)mg[j] - (double)prev[j]; v1[w][0] = first ? 0.0 : myB * myB; }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      auto part = [&](int k) {
        const double pk = (double)pw[k];
        double c = 0.0;
        if (k == C.band_iL[b]) c += pk * C.band_wL[b];
        if (k > C.band_iL[b] && k < C.band_iR[b]) c += pk;
        if (k == C.band_iR[b]) c += pk * C.band_wR[b];
        return c;
      };
      v1[w][1 + b] = part(j) + (tid == 0 ? part(0) : 0.0);
    }
  }
  // frame energy = centroid denominator, centroid numerator and the roll-off prefix: the reference's chains, lane 0 walks the bins
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  double frameSum = 0.0, sumA = 0.0;
  if (lane == 0) seq_chains_f64(pw + 1, chain_d, 64 * W, frameSum, sumA);
  frameSum = wave_first_d(frameSum);
  sumA = wave_first_d(sumA);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  double t1v[3];
  wave_sumw<3, W>(v1, t1v);
  float ctr = 0.0f;
  if (frameSum != 0.0) ctr = (float)(sumA / frameSum);
  // roll-off (:1102-1122): the first bin whose running sum reaches the share (the running sum never falls: one bin at most)
  {
    const double rollOff[4] = {0.25, 0.50, 0.75, 0.90};
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const int tid = lane + 64 * w, j = tid + 1;
      const double c = chain_d[tid];
      const double before = tid ? chain_d[tid - 1] : -1.0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const double th = rollOff[i] * frameSum;
        if (c >= th && (tid == 0 || !(before >= th))) sp[2 + i] = (float)(F0 * j);
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the running sums have been read: the float chains' terms take their place below)
  __builtin_amdgcn_wave_barrier();
  // harmonicity: alternating peaks/valleys, distance to the previous one
  float hc[W];
  {
    float pk_val[W];
    bool pk_has[W];
    bool flag[W];
    unsigned long long lower[W];
    float prevw[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const int j = lane + 64 * w + 1;
      flag[w] = false;
      if (j >= lo + 2 && j < hi - 1)
        flag[w] = (pw[j - 2] < pf[w] && pw[j - 1] < pf[w] && pf[w] > pw[j + 1] && pf[w] > pw[j + 2]) ||
                  (pw[j - 2] > pf[w] && pw[j - 1] > pf[w] && pf[w] < pw[j + 1] && pf[w] < pw[j + 2]);
      const unsigned long long mask = __ballot(flag[w]);
      lower[w] = mask & ((1ull << lane) - 1ull);
      const int src = lower[w] ? 63 - __clzll((long long)lower[w]) : 0;
      prevw[w] = __shfl(pf[w], src, 64);
      pk_has[w] = mask != 0ull;
      pk_val[w] = __shfl(pf[w], mask ? 63 - __clzll((long long)mask) : 0, 64);
    }
#pragma unroll
    for (int w = 0; w < W; ++w) {
      hc[w] = 0.0f;
      if (flag[w]) {
        if (lower[w]) hc[w] = fabsf(pf[w] - prevw[w]);
        else {
          bool found = false;
#pragma unroll
          for (int w2 = W - 1; w2 >= 0; --w2)
            if (w2 < w && !found && pk_has[w2]) { hc[w] = fabsf(pf[w] - pk_val[w2]); found = true; }
        }
      }
    }
  }
  double v2[W][5], m3t[W];
#pragma unroll
  for (int w = 0; w < W; ++w) {
    const double entropy_floor = 0.0000001;
    double dn = frameSum;
    if (dn < (float)entropy_floor) dn = (float)entropy_floor;
    double v = p[w];
    if (v <= entropy_floor) v = entropy_floor;
    const double ln = v / dn;
    // (ln > 0: a quotient of two values >= 1e-7 that are floats or sums of floats -- a positive normal double, or +inf)
    v2[w][0] = (ln > 0.0) ? ln * log_d<true>(ln, C.log_tab ? static_cast<const double2 *>(C.log_tab) : kLogTab) / log(2.0) : 0.0;
    const double t1 = fj[w] - (double)ctr;
    double m = t1 * t1 * p[w];
    v2[w][1] = m; m *= t1; m3t[w] = m; v2[w][3] = m * t1;
    v2[w][2] = 0.0;                                         // (third moment: a double chain, below)
    v2[w][4] = 0.0;
  }
  double t2v[5];
  wave_sumw<5, W>(v2, t2v);
  // sharpness and harmonicity accumulate in FLOAT_DMEM, bin after bin (:1435-1471, :1485-1499): the terms go to LDS, lane 0
  // adds them in order. (Measured alternative: every lane walking the chains with 512 unrolled v_readlane + v_add was 17 %
  // slower for the whole kernel -- issue slots and registers -- than one lane reading float4s one block ahead.)
#pragma unroll
  for (int w = 0; w < W; ++w) {
    chain[lane + 64 * w] = tsh[w];
    chain[64 * W + lane + 64 * w] = hc[w];                 // |srcLP[j] - lastPeak| of a flagged bin, +0 elsewhere (s + 0 = s)
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  float sumAA_seq = 0.0f, ptp_seq = 0.0f;
  if (lane == 0) seq_sum2_f32(chain, chain + 64 * W, 64 * W, sumAA_seq, ptp_seq);
  // the third moment's terms take the float chains' place (128 W floats = 64 W doubles), bin after bin like the reference's loop
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int w = 0; w < W; ++w) chain_d[lane + 64 * w] = m3t[w];
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (lane == 0) {
    const double mom3 = seq_sum_f64(chain_d, 64 * W);
    sp[0] = (float)(t1v[1] / (double)nBins);
    sp[1] = (float)(t1v[2] / (double)nBins);
    float c2 = 0.0f;
    const float sumAA = sumAA_seq;
    if (frameSum != 0.0) c2 = (float)(sumAA / frameSum);
    sp[13] = (float)(0.11 * c2);
    const double flux = t1v[0] / (double)nBins;
    sp[6] = (!first && flux > 0.0) ? (float)sqrt(flux) : 0.0f;
    sp[7] = ctr;
    sp[8] = (float)(-t2v[0]);
    const double sumB = frameSum;
    const double sigma2 = (sumB != 0.0) ? t2v[1] / sumB : 0.0;
    sp[9] = (float)sigma2;
    sp[10] = (sigma2 <= 0.0) ? 0.0f : (float)(mom3 / (sumB * sigma2 * sqrt(sigma2)));
    sp[11] = (sigma2 == 0.0) ? 0.0f : (float)(t2v[3] / (sumB * sigma2 * sigma2));
    const double Nind = (double)nBins;
    const double deno = (Nind * C.slope_S2f - C.slope_Sf * C.slope_Sf);
    double slope = 0.0;
    if (deno != 0.0) slope = (Nind * sumA - C.slope_Sf * sumB) / deno;
    sp[12] = (float)(slope * (Nind - 1.0));
    float ptpSum = ptp_seq;
    ptpSum /= 2.0f;
    ptpSum /= (float)nBins;
    sp[14] = ptpSum;
  }
}

// R8 cPlp as auditory spectrum, one band (plp.cpp:416-593 with doAud = 1, doIDFT = doLP = 0).
// Without RASTA: melfloor, x equal loudness, power-law compression through double pow (:499-507).
__device__ __forceinline__ float plp_aud_band(float mel, float melfloor, float eql, float compression) {
  float v = mel < melfloor ? melfloor : mel;
  v *= eql;
  return (float)pow((double)v, (double)compression);
}
// newRASTA in the log domain (:434-439 doLog, :468-485 filter, :490-497 log equal loudness and compression,
// :512-517 exp): x = log of the floored band, st = the band's 4 filter taps, init = frames seen (capped at 5)
__device__ __forceinline__ float plp_rasta_band(float x, float (&st)[4], int init, const float *fir, float iir, float eql_log,
                                                float compression) {
  const float out = fir[0] * x + st[0];
  st[0] = fir[1] * x + st[1] + (float)(init >= 5) * iir * out;
  st[1] = fir[2] * x + st[2];
  st[2] = fir[3] * x + st[3];
  st[3] = fir[4] * x;
  x = (init >= 5) ? out : 0.0f;
  x += eql_log;
  x *= compression;
  return glibc_expf(x);                                 // plp.cpp:512-517: exp() on a float is expf
}

}  // namespace smilehip
