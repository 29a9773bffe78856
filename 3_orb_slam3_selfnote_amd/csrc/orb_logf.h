// orb_logf.h -- bit-exact replica of the libm logf that MapPoint::PredictScale calls
// (`ceil(log(ratio)/mfLogScaleFactor)` on a float ratio, MapPoint.cc:587-602: log(float) -> glibc logf), so that the level
// prediction of the local-map search (Frame::isInFrustum, Frame.cc:572-661) can run on the device and still pick the
// reference's pyramid level at every boundary ratio = scaleFactor^k.
//
// glibc >= 2.28 implements logf after ARM "optimized-routines" (sysdeps/ieee754/flt-32/e_logf.c, e_logf_data.c):
// x = 2^k z with z in [OFF, 2 OFF) (OFF = 0x3f330000) split into 16 subintervals, r = z invc - 1 and
// log(x) = log1p(r) + logc + k ln2, log1p(r) by a degree-4 polynomial evaluated in double, rounded once to float.
// Every step is an IEEE-754 double mul / fma / add or a float <-> double conversion, so host and gfx950 give the same
// bits; the multiply-adds are written as explicit fma (the FMA ifunc variant libm selects on x86-64 hosts; the plain
// variant rounds to the same floats on every input).  tests/test_logf_replica.py checks the replica against the host
// libm (every non-negative float with ORB_EXHAUSTIVE=1, a strided sample and the PredictScale boundaries otherwise).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define ORBLG_HD __host__ __device__ inline
#else
#define ORBLG_HD inline
#endif

namespace orblg {

ORBLG_HD uint32_t fbits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(f);
#else
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
#endif
}

ORBLG_HD float bitsf(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(u);
#else
  float f;
  memcpy(&f, &u, 4);
  return f;
#endif
}

ORBLG_HD double madd(double a, double b, double c) { return __builtin_fma(a, b, c); }

// e_logf_data.c: (invc, logc) of subinterval i, ln2, poly A[0..2]
ORBLG_HD void table(int i, double &invc, double &logc) {
  switch (i) {
    case 0: invc = 0x1.661ec79f8f3bep+0; logc = -0x1.57bf7808caadep-2; break;
    case 1: invc = 0x1.571ed4aaf883dp+0; logc = -0x1.2bef0a7c06ddbp-2; break;
    case 2: invc = 0x1.49539f0f010bp+0; logc = -0x1.01eae7f513a67p-2; break;
    case 3: invc = 0x1.3c995b0b80385p+0; logc = -0x1.b31d8a68224e9p-3; break;
    case 4: invc = 0x1.30d190c8864a5p+0; logc = -0x1.6574f0ac07758p-3; break;
    case 5: invc = 0x1.25e227b0b8eap+0; logc = -0x1.1aa2bc79c81p-3; break;
    case 6: invc = 0x1.1bb4a4a1a343fp+0; logc = -0x1.a4e76ce8c0e5ep-4; break;
    case 7: invc = 0x1.12358f08ae5bap+0; logc = -0x1.1973c5a611cccp-4; break;
    case 8: invc = 0x1.0953f419900a7p+0; logc = -0x1.252f438e10c1ep-5; break;
    case 9: invc = 0x1p+0; logc = 0x0p+0; break;
    case 10: invc = 0x1.e608cfd9a47acp-1; logc = 0x1.aa5aa5df25984p-5; break;
    case 11: invc = 0x1.ca4b31f026aap-1; logc = 0x1.c5e53aa362eb4p-4; break;
    case 12: invc = 0x1.b2036576afce6p-1; logc = 0x1.526e57720db08p-3; break;
    case 13: invc = 0x1.9c2d163a1aa2dp-1; logc = 0x1.bc2860d22477p-3; break;
    case 14: invc = 0x1.886e6037841edp-1; logc = 0x1.1058bc8a07ee1p-2; break;
    default: invc = 0x1.767dcf5534862p-1; logc = 0x1.4043057b6ee09p-2; break;
  }
}

// e_logf.c:__logf
ORBLG_HD float ref_logf(float x) {
  const double Ln2 = 0x1.62e42fefa39efp-1;
  const double A0 = -0x1.00ea348b88334p-2, A1 = 0x1.5575b0be00b6ap-2, A2 = -0x1.ffffef20a4123p-2;
  const uint32_t OFF = 0x3f330000;
  uint32_t ix = fbits(x);
  if (ix == 0x3f800000u) return 0.0f;                        // log(1) = +0 in every rounding mode
  if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {       // subnormal, zero, negative, inf or nan
    if (ix * 2 == 0) return -__builtin_inff();                // __math_divzerof(1): -inf
    if (ix == 0x7f800000u) return x;                          // log(inf) = inf
    if ((ix & 0x80000000u) || ix * 2 >= 0xff000000u) return (x - x) / (x - x);   // __math_invalidf: nan (input nan quieted)
    ix = fbits(x * 0x1p23f);                                  // subnormal: normalise
    ix -= 23u << 23;
  }
  const uint32_t tmp = ix - OFF;
  const int i = (int)((tmp >> (23 - 4)) % 16);
  const int k = (int32_t)tmp >> 23;                           // arithmetic shift
  const uint32_t iz = ix - (tmp & (0x1ffu << 23));
  double invc, logc;
  table(i, invc, logc);
  const double z = (double)bitsf(iz);
  const double r = madd(z, invc, -1.0);
  const double y0 = madd((double)k, Ln2, logc);
  const double r2 = r * r;
  double y = madd(A1, r, A2);
  y = madd(A0, r2, y);
  y = madd(y, r2, y0 + r);
  return (float)y;
}

}  // namespace orblg
