// orb_fast_score.h -- the threshold-free FAST-9/16 score of one pixel, stated once for the device (k_fast) and the host
// (tests/test_fast_score_network.py compiles this header into a stand-alone program).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "orb_common.h"

typedef short pk16 __attribute__((ext_vector_type(2)));  // two signed 16-bit lanes in one VGPR (v_pk_*_i16)

// The three-input minimum / maximum of the score network, per 16-bit half.  Every value the network handles is an integer in
// [FAST_BIAS - 255, FAST_BIAS + 255] = [1793, 2303] (see fast_score_S): as f16 bit patterns 0x0701..0x08ff these are positive
// normal numbers, and for positive floats the order of the numbers is the order of the bit patterns, so gfx950's packed f16
// v_pk_minimum3_f16 / v_pk_maximum3_f16 select exactly what the integer minimum / maximum selects (no NaN, denormal or signed
// zero is in the range; a min/max returns one of its operands' bit patterns unchanged).  The host takes plain integers.
constexpr int FAST_BIAS = 2048;
__host__ __device__ __forceinline__ pk16 fast_min3(pk16 a, pk16 b, pk16 c) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef _Float16 pkh __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(pk16, __builtin_elementwise_minimum(__builtin_elementwise_minimum(__builtin_bit_cast(pkh, a), __builtin_bit_cast(pkh, b)),
                                                                __builtin_bit_cast(pkh, c)));
#else
  return __builtin_elementwise_min(__builtin_elementwise_min(a, b), c);
#endif
}
__host__ __device__ __forceinline__ pk16 fast_max3(pk16 a, pk16 b, pk16 c) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef _Float16 pkh __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(pk16, __builtin_elementwise_maximum(__builtin_elementwise_maximum(__builtin_bit_cast(pkh, a), __builtin_bit_cast(pkh, b)),
                                                                __builtin_bit_cast(pkh, c)));
#else
  return __builtin_elementwise_max(__builtin_elementwise_max(a, b), c);
#endif
}

// S = max( max_arcs min_k (v - c_k), max_arcs min_k (c_k - v) ) over the 16 arcs of 9 contiguous circle pixels, clamped to
// [0, 255]; c = the centre pixel inside a plane of row pitch FAST_TILE_PITCH.
//
// The 16 arcs come in 8 pairs: arcs k and k+1 (k even) share the 8-pixel run d[k+1..k+8].  With r = min d[k+1..k+8]
//   max(min(d[k], r), min(r, d[k+9])) = min(r, max(d[k], d[k+9]))
// Proof: if r <= max(d[k], d[k+9]) one of the two inner minima is r and neither exceeds r, so both sides are r; otherwise both
// inner minima are d[k] and d[k+9] themselves and both sides are max(d[k], d[k+9]).  So
//   S = max over even k of  min( m8[k+1], max(d[k], d[k+9]) ),   m8[j] = min d[j..j+7]
// and m8 is needed at the 8 odd positions only, built by doubling on odd indices (mod 16): m2[j] = min(d[j], d[j+1]),
// m4[j] = min(m2[j], m2[j+2]), m8[j] = min(m4[j], m4[j+4]).  m8 is never formed on its own: min(m8[j], e) = min3(m4[j], m4[j+4], e)
// is ONE three-input minimum, and the eight pair values fold into their maximum with three three-input maxima and one two-input
// one.  8 + 8 minima, 8 maxima, 8 min3, 3 max3 + 1 maximum: 36 packed operations (47 with two-input operations only, 80 for
// taking every arc's minimum on its own).  An identity on the integers, per 16-bit half.
//
// All of it runs on d + FAST_BIAS (the bias rides in V2, so it costs nothing): a constant added to every value commutes with
// minimum and maximum, and it puts the values where fast_min3 / fast_max3 may take them as f16.  It comes off once at the end.
__host__ __device__ __forceinline__ int fast_score_S(const uint8_t *c /* tile centre, pitch FAST_TILE_PITCH */) {
  constexpr int Pt = FAST_TILE_PITCH;
  const int v = c[0];
  // d[k] = (v - c_k, c_k - v) + FAST_BIAS as two 16-bit halves: ONE packed min/max network yields the bright-centre margin
  // (low half) and the dark-centre margin (high half).
  const pk16 V2 = {(short)(FAST_BIAS + v), (short)(FAST_BIAS - v)};
  const pk16 K = {(short)-1, (short)1};
  pk16 d[16];
#define ORB_RING(k, off) { const short cc = (short)c[off]; const pk16 C = {cc, cc}; d[k] = C * K + V2; }
  ORB_RING(0, 3 * Pt + 0)   ORB_RING(1, 3 * Pt + 1)   ORB_RING(2, 2 * Pt + 2)    ORB_RING(3, 1 * Pt + 3)
  ORB_RING(4, 3)            ORB_RING(5, -1 * Pt + 3)  ORB_RING(6, -2 * Pt + 2)   ORB_RING(7, -3 * Pt + 1)
  ORB_RING(8, -3 * Pt)      ORB_RING(9, -3 * Pt - 1)  ORB_RING(10, -2 * Pt - 2)  ORB_RING(11, -1 * Pt - 3)
  ORB_RING(12, -3)          ORB_RING(13, 1 * Pt - 3)  ORB_RING(14, 2 * Pt - 2)   ORB_RING(15, 3 * Pt - 1)
#undef ORB_RING
  pk16 m2[8], m4[8], p[8];   // index i stands for the odd position j = 2 i + 1
#pragma unroll
  for (int i = 0; i < 8; i++) m2[i] = __builtin_elementwise_min(d[2 * i + 1], d[(2 * i + 2) & 15]);
#pragma unroll
  for (int i = 0; i < 8; i++) m4[i] = __builtin_elementwise_min(m2[i], m2[(i + 1) & 7]);
#pragma unroll
  for (int i = 0; i < 8; i++) {   // the arc pair k = 2 i, k + 1: shared run m8[k+1] = min(m4[i], m4[i+2]), end pixels d[k] and d[k+9]
    const pk16 e = __builtin_elementwise_max(d[2 * i], d[(2 * i + 9) & 15]);
    p[i] = fast_min3(m4[i], m4[(i + 2) & 7], e);
  }
  const pk16 A = __builtin_elementwise_max(fast_max3(p[0], p[1], p[2]), fast_max3(fast_max3(p[3], p[4], p[5]), p[6], p[7]));
  const int a = A.x - FAST_BIAS, b = A.y - FAST_BIAS;   // all of some arc darker by a, or brighter by b
  const int S = a > b ? a : b;
  return S < 0 ? 0 : (S > 255 ? 255 : S);
}
