// orb_tanf.h -- bit-exact replica of the libm tanf that KannalaBrandt8::unproject calls (`std::tan(theta)` on a float,
// KannalaBrandt8.cpp:135: std::tan(float) -> tanf), so that Frame::ComputeStereoFishEyeMatches' triangulation can run on the
// device and give the reference's bits.
//
// glibc 2.28 - 2.40 implements tanf as fdlibm's single-precision kernel (sysdeps/ieee754/flt-32/k_tanf.c) behind the double
// argument reduction it shares with sinf / cosf (s_tanf.c:rem_pio2f -> sincosf.h:reduce_fast): |x| <= pi/4 goes to the kernel
// directly; otherwise x = n pi/2 + dx in double, dx is split into two floats and the kernel returns tan or -1/tan of their sum.
// Every step is an IEEE-754 single or double add / mul / div or a conversion, in source order (x86-64 evaluates float expressions
// in float, and libm has no FMA variant of tanf), so host and gfx950 give the same bits under -ffp-contract=off with the correctly
// rounded fp32 divide.
//
// DOMAIN: every float.  |x| < 120 is reduce_fast's; beyond it the argument goes through sincosf.h's reduce_large (x times 2/pi in
// 64-bit integer arithmetic).  The unprojection's theta starts in [0, pi/2] and moves by Newton steps: with a distortion polynomial
// that turns back below pi/2 the steps diverge, the reference takes tanf of whatever the tenth one left, and so must this
// (tests/test_ref_cameras.py::test_unproject[distorted]).  inf and NaN give NaN as in libm.  glibc 2.41 replaced tanf by a correctly
// rounded one, and glibc before 2.28 reduced in float: against such a host the replica differs in the last bits for some arguments
// and the test fails there.  The reference's libm is not pinned.
#pragma once
#include <stdint.h>
#include "orb_logf.h"   // orblg::fbits / bitsf

#if defined(__HIPCC__)
#define ORBTN_HD __host__ __device__ inline
#else
#define ORBTN_HD inline
#endif

namespace orbtn {

// k_tanf.c:__kernel_tanf, iy = 1: tan(x + y), iy = -1: -1 / tan(x + y); |x + y| <= pi/4
ORBTN_HD float kernel_tanf(float x, float y, int iy) {
  const float pio4 = 7.8539812565e-01f, pio4lo = 3.7748947079e-08f;   // 0x3f490fda, 0x33222168
  const float T0 = 3.3333334327e-01f, T1 = 1.3333334029e-01f, T2 = 5.3968254477e-02f, T3 = 2.1869488060e-02f, T4 = 8.8632395491e-03f,
              T5 = 3.5920790397e-03f, T6 = 1.4562094584e-03f, T7 = 5.8804126456e-04f, T8 = 2.4646313977e-04f, T9 = 7.8179444245e-05f,
              T10 = 7.1407252108e-05f, T11 = -1.8558637748e-05f, T12 = 2.5907305826e-05f;
  const int32_t hx = (int32_t)orblg::fbits(x);
  const int32_t ix = hx & 0x7fffffff;
  if (ix < 0x39000000) {   // |x| < 2**-13
    if ((int)x == 0) {
      if ((ix | (iy + 1)) == 0) return 1.0f / __builtin_fabsf(x);
      else if (iy == 1) return x;
      else return -1.0f / x;
    }
  }
  if (ix >= 0x3f2ca140) {   // |x| >= 0.6744
    if (hx < 0) { x = -x; y = -y; }
    const float z0 = pio4 - x, w0 = pio4lo - y;
    x = z0 + w0;
    y = 0.0f;
    if (__builtin_fabsf(x) < 0x1p-13f) return (float)((1 - ((hx >> 30) & 2)) * iy) * (1.0f - (float)(2 * iy) * x);
  }
  float z = x * x;
  float w = z * z;
  float r = T1 + w * (T3 + w * (T5 + w * (T7 + w * (T9 + w * T11))));
  float v = z * (T2 + w * (T4 + w * (T6 + w * (T8 + w * (T10 + w * T12)))));
  float s = z * x;
  r = y + z * (s * (r + v) + y);
  r += T0 * s;
  w = x + r;
  if (ix >= 0x3f2ca140) {
    v = (float)iy;
    return (float)(1 - ((hx >> 30) & 2)) * (v - 2.0f * (x - (w * w / (w + v) - r)));
  }
  if (iy == 1) return w;
  // -1 / (x + r), accurately
  z = orblg::bitsf(orblg::fbits(w) & 0xfffff000u);
  v = r - (z - x);   // z + v = r + x
  const float a = -1.0f / w;
  const float t = orblg::bitsf(orblg::fbits(a) & 0xfffff000u);
  s = 1.0f + t * z;
  return t + a * (s + t * v);
}

// sincosf.h:reduce_large for |x| >= 120: the 24 significand bits of x, shifted by the exponent's low three bits, times three
// consecutive 32-bit words of 2/pi picked by the exponent's next four bits (sincosf_data.c:__inv_pio4 holds the windows of
// 0xA2F9836E4E441529FC2757D1F534DDC0DB6295993C439041 a byte apart; entry k ends at byte k + 1), keeping the 64 bits below the
// quadrant count.  Returns the remainder in [-pi/4, pi/4] for |x|, *np = the quadrant.
ORBTN_HD uint32_t inv_pio4_word(int k) {
  // bits [s, s + 32) from the left of 0 : H0 : H1 : H2 (64 bits each), s = 8 * (k + 1) + 32
  const uint64_t H0 = 0xA2F9836E4E441529ull, H1 = 0xFC2757D1F534DDC0ull, H2 = 0xDB6295993C439041ull;
  const int s = 8 * (k + 1) + 32, i = s >> 6, off = s & 63;
  const uint64_t hi = i == 0 ? 0ull : i == 1 ? H0 : i == 2 ? H1 : H2;
  const uint64_t lo = i == 0 ? H0 : i == 1 ? H1 : i == 2 ? H2 : 0ull;
  const uint64_t v = off ? (hi << off) | (lo >> (64 - off)) : hi;
  return (uint32_t)(v >> 32);
}
ORBTN_HD double reduce_large(uint32_t xi, int32_t *np) {
  const double pi63 = 0x1.921FB54442D18p-62;   // 2 pi * 2^-64
  const int k = (int)((xi >> 26) & 15u);
  const int shift = (int)((xi >> 23) & 7u);
  xi = (xi & 0xffffffu) | 0x800000u;
  xi <<= shift;
  uint64_t res0 = (uint64_t)(uint32_t)(xi * inv_pio4_word(k));
  const uint64_t res1 = (uint64_t)xi * inv_pio4_word(k + 4);
  const uint64_t res2 = (uint64_t)xi * inv_pio4_word(k + 8);
  res0 = (res2 >> 32) | (res0 << 32);
  res0 += res1;
  const uint64_t n = (res0 + (1ull << 61)) >> 62;
  res0 -= n << 62;
  *np = (int32_t)n;
  return (double)(int64_t)res0 * pi63;
}

// s_tanf.c:__tanf; its rem_pio2f is sincosf.h's reduce_fast in double (|x| < 120): n = round(x * 2/pi), dx = x - n * pi/2 by a
// separate multiply and subtract (tanf has no FMA variant), y0 = (float)dx, y1 = (float)(dx - y0)
ORBTN_HD float ref_tanf(float x) {
  const double HPI_INV = 0x1.45f306dc9c883p+23;   // 2/pi * 2^24
  const double HPI = 0x1.921fb54442d18p+0;        // pi/2
  const uint32_t ix = orblg::fbits(x) & 0x7fffffffu;
  if (ix <= 0x3f490fdau) return kernel_tanf(x, 0.0f, 1);   // |x| ~< pi/4
  if (ix >= 0x7f800000u) return x - x;                     // inf, nan
  if (((ix >> 20) & 0x7ffu) >= 0x42fu) {   // |x| >= 120: rem_pio2f's other branch, the sign applied to the remainder
    int32_t n;
    double dl = reduce_large(orblg::fbits(x), &n);
    if (orblg::fbits(x) >> 31) dl = -dl;
    const float l0 = (float)dl;
    const float l1 = (float)(dl - (double)l0);
    return kernel_tanf(l0, l1, 1 - ((n & 1) << 1));
  }
  double dx = (double)x;
  const double r = dx * HPI_INV;
  const int32_t n = ((int32_t)r + 0x800000) >> 24;
  const double nh = (double)n * HPI;
  dx = dx - nh;
  const float y0 = (float)dx;
  const float y1 = (float)(dx - (double)y0);
  return kernel_tanf(y0, y1, 1 - ((n & 1) << 1));
}

}  // namespace orbtn
