// sincos_d: double sine and cosine of one argument with a shared reduction, for the per-sample recursion of cTonefilt
// (lld_tonefilt_ops.hpp). __host__ __device__ and free of table lookups: the host build (tests/helpers/tonefilt_check.cpp) is
// the very same arithmetic, fma for fma, so its accuracy can be measured against long double without a device as well.
//
// DOMAIN: |x| <= kSincosDomain = 2^30 (sin(-0) is +0: the reduction's first fma loses the sign, and the recursion's arguments are
// never negative). Outside of it (and for NaN) the result is unspecified; the callers refuse the work
// (tonefilt::max_argument against kSincosDomain at plan / batch / operator creation, SMILEHIP_ERR_INVALID).
//
// Reduction: k = rint(x 2/pi), |k| < 2^30; r = x - k pi/2 with pi/2 = P1 + P2 + P3 to 2^-161:
//   t = fma(-k, P1, x) is exact: for k != 0, |x| > pi/4, so x is a multiple of 2^-53, and k P1 is one of ulp(P1) = 2^-52 (k is an
//   integer); their difference is a multiple of 2^-53 below 1 in magnitude, so it has at most 53 significant bits (k = 0: t = x);
//   k P2 as an exact pair (p, pe) by fma; t - p by a branch-free two-sum; the tail e - pe - k P3 is below 2^-52 |t - p| + 2^-76 and
//   carries a relative error of 2^-52 itself. The reduced argument is the pair (r, rl), |r| <= pi/4 + 2^-30, known to about
//   2^-105 absolutely -- for |x| <= 2^30 no double comes closer to a multiple of pi/2 than about 2^-62 relative, so the pair's
//   relative error stays below 2^-40.
// Kernels: the minimax polynomials of fdlibm's k_sin.c / k_cos.c (Sun Microsystems, freely distributable) on [-pi/4, pi/4] with
// the tail rl as their second argument; their own error is below 0.51 ulp (sin) and 0.53 ulp (cos) on the exact pair. The total
// stays below 1 ulp; tests/test_gpu_sincos_d.py measures it against sinl / cosl.
#pragma once
#include <cstdint>

#include "glibc_float.hpp"

namespace smilehip {

constexpr double kSincosDomain = 1073741824.0;   // 2^30

struct SinCosD {
  double s, c;
};

GLF_HD SinCosD sincos_d(double x) {
  const double kTwoOverPi = 6.36619772367581382433e-01;   // 0x3FE45F306DC9C883
  const double P1 = 1.57079632679489655800e+00;           // 0x3FF921FB54442D18: pi/2 rounded to double
  const double P2 = 6.12323399573676603587e-17;           // 0x3C91A62633145C07: pi/2 - P1 rounded to double
  const double P3 = -1.49738490485916983294e-33;          // 0xB91F1976B7ED8FBC: pi/2 - P1 - P2 rounded to double
  const double kd = __builtin_rint(x * kTwoOverPi);
  const int q = (int)kd;
  const double t = __builtin_fma(-kd, P1, x);
  const double p = kd * P2;
  const double pe = __builtin_fma(kd, P2, -p);
  const double r1 = t - p;                                 // two-sum of t and -p
  const double bb = r1 - t;
  const double e = (t - (r1 - bb)) - (p + bb);
  const double lo = __builtin_fma(-kd, P3, e - pe);
  const double r = r1 + lo;
  const double rl = (r1 - r) + lo;

  const double z = r * r;
  const double w = z * z;
  // __kernel_sin(r, rl, 1)
  const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
               S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
  const double rs = __builtin_fma(z, __builtin_fma(z, S4, S3), S2) + z * w * __builtin_fma(z, S6, S5);
  const double v = z * r;
  const double sn = r - ((z * (0.5 * rl - v * rs) - rl) - v * S1);
  // __kernel_cos(r, rl)
  const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
               C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
  const double rc = z * __builtin_fma(z, __builtin_fma(z, C3, C2), C1) + w * w * __builtin_fma(z, __builtin_fma(z, C6, C5), C4);
  const double hz = 0.5 * z;
  const double w1 = 1.0 - hz;
  const double cs = w1 + (((1.0 - w1) - hz) + (z * rc - r * rl));

  SinCosD o;
  const double a = (q & 1) ? cs : sn, b = (q & 1) ? sn : cs;
  o.s = (q & 2) ? -a : a;
  o.c = ((q + 1) & 2) ? -b : b;
  return o;
}

}  // namespace smilehip
