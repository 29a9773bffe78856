// orb_ref_geometry.h -- the reference's projection expressions, each stated once for the host loops of orbhip.hip and the kernels
// of orb_project_kernels.h.  Every operation is the IEEE-754 single / double operation of the reference's expression in source
// order; both halves of the translation unit are compiled without contraction and with correctly rounded fp32 divide / sqrt
// (build.py), and the libm calls go through the bit-exact glibc replicas, so a function gives the same bits on either side.
// New projection code calls these and does not restate them ("Bit-exactness").
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/orbhip.h"
#include "orb_atan2f.h"
#include "orb_sincos.h"

#define ORB_REF __host__ __device__ __forceinline__

// cv::Mat `A*B + C` for a 3x3 * 3x1 product (ORBmatcher.cc:2047, :2072, Frame.cc:586): one cv::gemm whose
// small-matrix float path forms a0*b0 + a1*b1 + a2*b2 in float, then adds C.  [OPENCV-UNVERIFIED], identical in the test oracle.
ORB_REF void mat3_mul_add(const float *R, const float *x, const float *t, float *out) {  // R: row-major, row stride 4
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float t0 = R[i * 4 + 0] * x[0] + R[i * 4 + 1] * x[1] + R[i * 4 + 2] * x[2];
    out[i] = (float)((double)t0 + (double)t[i]);
  }
}

// Camera centre of a row-major 4x4 [Rcw | tcw]: Ow = -Rcw.t()*tcw (ORBmatcher.cc:2041, :2297, Frame::UpdatePoseMatrices
// Frame.cc:538), the generic cv::gemm path: accumulated in double, scaled by alpha = -1 there, rounded once.  -acc and
// acc * -1.0 are the same IEEE operation (a sign flip, exact).
ORB_REF void camera_centre(const float *T, float *Ow) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    double acc = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) acc += (double)T[4 * k + i] * (double)T[4 * k + 3];
    Ow[i] = (float)(-acc);
  }
}

// The right camera of a fisheye-stereo rig in Frame::isInFrustumChecks (Frame.cc:1276-1280), from Tcw = [mRcw | mtcw] and
// Trl = mTrl (both row-major, row stride 4) and tlr = mTlr.col(3).  [OPENCV-UNVERIFIED] like mat3_mul_add / camera_centre:
//   mR = Rrl * mRcw (:1278): a 3x3 * 3x3 cv::gemm, per entry a0*b0 + a1*b1 + a2*b2 in float (the small-matrix path);
//   mt = Rrl * mtcw + trl (:1279): mat3_mul_add;
// written as Tr = [mR | mt], 12 floats with row stride 4, so that mat3_mul_add applies to it (:1289).
ORB_REF void rig_right_pose(const float *Tcw, const float *Trl, float *Tr) {
  const float tcw[3] = {Tcw[3], Tcw[7], Tcw[11]}, trl[3] = {Trl[3], Trl[7], Trl[11]};
  float t[3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) Tr[4 * i + j] = Trl[4 * i + 0] * Tcw[j] + Trl[4 * i + 1] * Tcw[4 + j] + Trl[4 * i + 2] * Tcw[8 + j];
  mat3_mul_add(Trl, tcw, trl, t);
  Tr[3] = t[0]; Tr[7] = t[1]; Tr[11] = t[2];
}

//   twc = mRwc * tlr + mOw (:1280) with mRwc = mRcw.t() (Frame.cc:536) and mOw = camera_centre(Tcw): one `A*B + C` gemm over the
//   stored transpose, the form of mat3_mul_add.
ORB_REF void rig_right_centre(const float *Tcw, const float *tlr, const float *Ow, float *twc) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float t0 = Tcw[i] * tlr[0] + Tcw[4 + i] * tlr[1] + Tcw[8 + i] * tlr[2];
    twc[i] = (float)((double)t0 + (double)Ow[i]);
  }
}

// Mat::dot of two 3-vectors of floats: products and sum in double
ORB_REF double dot3_double(const float *a, const float *b) {
  double d = 0;
#pragma unroll
  for (int k = 0; k < 3; k++) d += (double)a[k] * (double)b[k];
  return d;
}

// cv::norm of a 3-vector of floats (NORM_L2): the squares are accumulated in double, the root is rounded to float
ORB_REF float norm3(const float *p) { return (float)sqrt(dot3_double(p, p)); }

// GeometricCamera::project(cv::Point3f): 0 Pinhole (Pinhole.cpp:46-49), 1 KannalaBrandt8 (KannalaBrandt8.cpp:29-45)
ORB_REF void project(int cam_type, const float *p, float X, float Y, float Z, float &u, float &v) {
  if (cam_type == 0) {
    u = p[0] * X / Z + p[2];
    v = p[1] * Y / Z + p[3];
  } else {
    const float x2_plus_y2 = X * X + Y * Y;
    const float theta = orbat::ref_atan2f(sqrtf(x2_plus_y2), Z);
    const float psi = orbat::ref_atan2f(Y, X);
    const float theta2 = theta * theta, theta3 = theta * theta2, theta5 = theta3 * theta2, theta7 = theta5 * theta2, theta9 = theta7 * theta2;
    const float r = theta + p[4] * theta3 + p[5] * theta5 + p[6] * theta7 + p[7] * theta9;
    // cos / sin on a float resolve to the float overloads (cosf / sinf) once <math.h> is in the translation unit, which
    // opencv2/opencv.hpp brings (libm choices) - the same assumption MapPoint::PredictScale's log(float) rests on;
    // evaluated through the bit-exact glibc replicas on both sides (tests/test_libm_replicas.py: equal to the host libm)
#ifdef ORB_KB8_DOUBLE_TRIG   // build switch for reference builds in which cos(psi) / sin(psi) bind ::cos(double) (GCC 5, or no <math.h> wrapper).
                             // The device's fp64 cos / sin are ROCm's, within 1 ulp of glibc's but NOT verified equal: with this switch the
                             // windows of config 5 are no longer covered by the bit-exact replicas (parity unpinned)
    u = (float)((double)(p[0] * r) * ::cos((double)psi) + (double)p[2]);
    v = (float)((double)(p[1] * r) * ::sin((double)psi) + (double)p[3]);
#else
    u = p[0] * r * orbsc::ref_cosf(psi) + p[2];
    v = p[1] * r * orbsc::ref_sinf(psi) + p[3];
#endif
  }
}

// The image-bounds test of the Frame searches (ORBmatcher.cc:2094-2097, :2321-2324, Frame.cc:599-602) as the reference writes it:
// two rejections, so a NaN projection passes
ORB_REF bool inside_bounds(float u, float v, float min_x, float max_x, float min_y, float max_y) {
  return !(u < min_x || u > max_x) && !(v < min_y || v > max_y);
}

// KeyFrame::IsInImage (KeyFrame.cc:844-847): closed below, open above, and a NaN projection fails
ORB_REF bool is_in_image(float u, float v, float min_x, float max_x, float min_y, float max_y) {
  return u >= min_x && u < max_x && v >= min_y && v < max_y;
}

// The scale-invariance gate of the projection searches for map point i: true when `dist` lies outside
// [0.8 * min_dist[i], 1.2 * max_dist[i]] (MapPoint::GetMinDistanceInvariance / GetMaxDistanceInvariance, MapPoint.cc:552-565).
// The signature serves a register count, not the expression: with the arrays, max_dist[i] is read only behind the first
// comparison; with both distances passed by value k_local_map_project needs one vector register more (41 against the 40 it had
// before the expressions were shared).  It may go back to by-value once that count no longer depends on it.
ORB_REF bool outside_scale_range(float dist, const float *min_dist, const float *max_dist, size_t i) {
  return dist < 0.8f * min_dist[i] || dist > 1.2f * max_dist[i];
}

// (int) of a float as the reference build converts it (x86 cvttss2si): NaN and values outside the int range give INT_MIN, where
// the C++ conversion is undefined and gfx950's v_cvt_i32_f32 would saturate
ORB_REF int x86_cvtt_f32_i32(float x) {
  return (x != x || x >= 2147483648.0f || x < -2147483648.0f) ? (int)0x80000000u : (int)x;
}

// MapPoint::PredictScale (MapPoint.cc:570-602) behind its logarithm: ceil(log(max_dist / dist) / log(scale factor)) clamped to the
// pyramid.  log_ratio is libm's logf on the host and orblg::ref_logf (orb_logf.h) on the device.
ORB_REF int level_from_log(float log_ratio, float log_sf, int nlevels) {
  int lvl = x86_cvtt_f32_i32(ceilf(log_ratio / log_sf));
  if (lvl < 0) lvl = 0;
  else if (lvl >= nlevels) lvl = nlevels - 1;
  return lvl;
}

// ORBmatcher::RadiusByViewingCos, ORBmatcher.cc:216-222
ORB_REF float radius_by_viewing_cos(float view_cos) { return ((double)view_cos > 0.998) ? 2.5f : 4.0f; }

// The level window of SearchByProjection(CurrentFrame, LastFrame) around the last keypoint's octave (ORBmatcher.cc:2113-2118,
// :2201-2206); max_level = -1: no upper limit
ORB_REF void lastframe_level_window(bool bForward, bool bBackward, int oct, int &minl, int &maxl) {
  if (bForward) { minl = oct; maxl = -1; }
  else if (bBackward) { minl = 0; maxl = oct; }
  else { minl = oct - 1; maxl = oct + 1; }
}

// flags byte of a query that takes part: bit 0, and bit 1 = pMP->Observations() > 0 (obs == NULL: all 1)
ORB_REF uint8_t query_flags(const uint8_t *obs, size_t i) { return (uint8_t)(1u | ((obs ? (obs[i] & 1u) : 1u) << 1)); }

// Bin of the rotation histogram for the angle difference `rot` of a match (ORBmatcher.cc:2177-2185); the caller keeps the match
// out of the histogram unless 0 <= bin < ORBM_HISTO_LENGTH
ORB_REF int rot_bin(float rot) {
  const float factor = 1.0f / ORBM_HISTO_LENGTH;
  if ((double)rot < 0.0) rot += 360.0f;
  int bin = (int)roundf(rot * factor);
  if (bin == ORBM_HISTO_LENGTH) bin = 0;
  return bin;
}

// ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:2416-2458) on the bin sizes.  The indices are locals until the end: updated
// through the references, the device compiler keeps them in scratch memory.
ORB_REF void three_maxima(const int *sizes, int L, int &ind1, int &ind2, int &ind3) {
  int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
  for (int i = 0; i < L; i++) {
    const int s = sizes[i];
    if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
    else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
    else if (s > max3) { max3 = s; i3 = i; }
  }
  if ((float)max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
  else if ((float)max3 < 0.1f * (float)max1) { i3 = -1; }
  ind1 = i1; ind2 = i2; ind3 = i3;
}

// cv::undistortPoints with R = I, P = K (Frame.cc:856, :883) restated: five fixed-point iterations in double
ORB_REF void undistort_point(double u, double v, const float *K, const float *D, int nD, float *ou, float *ov) {
  const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
  const double k1 = D[0], k2 = D[1], p1 = D[2], p2 = D[3], k3 = nD > 4 ? D[4] : 0.0;
  double x = (u - cx) * (1. / fx), y = (v - cy) * (1. / fy);
  const double x0 = x, y0 = y;
  for (int it = 0; it < 5; it++) {
    const double r2 = x * x + y * y;
    const double icdist = 1. / (1 + ((k3 * r2 + k2) * r2 + k1) * r2);
    const double dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x);
    const double dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
    x = (x0 - dx) * icdist;
    y = (y0 - dy) * icdist;
  }
  *ou = (float)(x * fx + cx);
  *ov = (float)(y * fy + cy);
}

#undef ORB_REF
