// orb_ref_newpoints.h -- the body of LocalMapping::CreateNewMapPoints' inner loop (LocalMapping.cc:605-880) for ONE matched pair
// (idx1 of the new keyframe, idx2 of a neighbour), with KeyFrame::UnprojectStereo (KeyFrame.cc:850-869) and the camera models'
// unprojectMat (Pinhole.cpp:78-87; KannalaBrandt8.cpp:99-139), stated once for the host entry points of orbhip.hip and
// k_new_points_geometry, under the contract of orb_ref_geometry.h: IEEE-754 single / double operations in the reference's order, no
// contraction, correctly rounded divide and sqrt, libm through the glibc replicas.
//   * cv::Mat products and sums are the forms of orb_ref_geometry.h / orb_ref_triangulate.h ([OPENCV-UNVERIFIED] exactly as there):
//     `Rwc*xn` is mat3_mul_add over the stored transpose with a zero addend, Mat::dot and cv::norm accumulate in double, a row
//     `xn*T.row(2) - T.row(i)` rounds the product and then the difference, cv::SVD::compute is jacobi_svd4_last_row, the division of a
//     matrix by a scalar is (float)((double)v * (1.0 / (double)w)).
//   * cos(2*atan2(mb/2, mvDepth[idx])) (:736, :738) takes the float overloads, atan2f and cosf (unpinned list).
//   * mbInertial does not appear: both alternatives of :746 are the same expression.
#pragma once
#include "orb_ref_triangulate.h"

#define ORB_REF __host__ __device__ __forceinline__

// Rwc * x for Rwc = Rcw.t(), read from [Rcw | tcw] (row stride 4): the gemm of mat3_mul_add with no addend (:720-721)
ORB_REF void np_rotate_to_world(const float *Tcw, const float *x, float *out) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const float t0 = Tcw[i] * x[0] + Tcw[4 + i] * x[1] + Tcw[8 + i] * x[2];
    out[i] = (float)((double)t0 + 0.0);
  }
}

// GeometricCamera::unprojectMat: Pinhole ((x - cx) / fx, (y - cy) / fy, 1) or KannalaBrandt8::unproject
ORB_REF void np_unproject(int cam_type, const float *p, float x, float y, float *xn) {
  if (cam_type == 0) { xn[0] = (x - p[2]) / p[0]; xn[1] = (y - p[3]) / p[1]; xn[2] = 1.f; }
  else kb8_unproject(p, x, y, xn);
}

// cos(2*atan2(mb/2, depth)) of :736 / :738 in float
ORB_REF float np_cos_parallax_stereo(float mb, float depth) { return orbsc::ref_cosf(2.f * orbat::ref_atan2f(mb / 2.f, depth)); }

// KeyFrame::UnprojectStereo (KeyFrame.cc:850-869): reads mvKeys, NOT mvKeysUn; false = the empty matrix (z <= 0)
ORB_REF bool np_unproject_stereo(const orbm_new_point_camera_t &c, const orbm_new_point_obs_t &o, float *x3D) {
  const float z = o.depth;
  if (!(z > 0)) return false;
  const float x3Dc[3] = {(o.key_x - c.cx) * z * c.invfx, (o.key_y - c.cy) * z * c.invfy, z};
  const float twc[3] = {c.Twc[3], c.Twc[7], c.Twc[11]};
  mat3_mul_add(c.Twc, x3Dc, twc, x3D);
  return true;
}

// Rcw.row(i).dot(x3Dt) + tcw.at<float>(i): the dot product a double, the sum in double, rounded into the float (:791-803)
ORB_REF float np_row_dot(const float *Tcw, int i, const float *x3D) { return (float)(dot3_double(Tcw + 4 * i, x3D) + (double)Tcw[4 * i + 3]); }

// One side's reprojection test (:806-828, :836-854); mbf is ALWAYS the new keyframe's (:821, :847).  true = `continue`
ORB_REF bool np_reprojection_fails(const orbm_new_point_camera_t &c, int side, bool bStereo, float mbf1, const float *Tcw, const float *x3D, float z,
                                   const orbm_new_point_obs_t &o) {
  const float sigmaSquare = c.sigma2[o.octave & (ORBX_MAX_LEVELS - 1)];
  const float x = np_row_dot(Tcw, 0, x3D), y = np_row_dot(Tcw, 1, x3D);
  const float invz = (float)(1.0 / (double)z);
  if (!bStereo) {
    float u, v;
    project(c.cam_type, c.cam[side], x, y, z, u, v);
    const float errX = u - o.x, errY = v - o.y;
    return (double)(errX * errX + errY * errY) > 5.991 * (double)sigmaSquare;
  }
  const float u = c.fx * x * invz + c.cx;
  const float u_r = u - mbf1 * invz;
  const float v = c.fy * y * invz + c.cy;
  const float errX = u - o.x, errY = v - o.y, errX_r = u_r - o.u_right;
  return (double)(errX * errX + errY * errY + errX_r * errX_r) > 7.8 * (double)sigmaSquare;
}

// LocalMapping.cc:605-880 for one pair: an ORBM_NP_* status, x3D written on ORBM_NP_ACCEPTED only.  scale_factor1 = the new
// keyframe's mfScaleFactor (:521), far_points / th_far_points = mbFarPoints / mThFarPoints (:868).
ORB_REF int new_point_geometry(const orbm_new_point_camera_t &c1, const orbm_new_point_camera_t &c2, const orbm_new_point_obs_t &o1,
                               const orbm_new_point_obs_t &o2, float scale_factor1, int far_points, float th_far_points, float *x3D_out) {
  const bool rig1 = c1.n_left != -1, rig2 = c2.n_left != -1;
  const bool bStereo1 = !rig1 && o1.u_right >= 0, bStereo2 = !rig2 && o2.u_right >= 0;   // :618, :629
  // :635-700: pose, centre and camera by (bRight1, bRight2) when both keyframes have a second camera; the left ones otherwise
  const int s1 = (rig1 && rig2 && o1.right) ? 1 : 0, s2 = (rig1 && rig2 && o2.right) ? 1 : 0;
  const float *Tcw1 = c1.Tcw[s1], *Tcw2 = c2.Tcw[s2], *Ow1 = c1.Ow[s1], *Ow2 = c2.Ow[s2];
  float xn1[3], xn2[3], ray1[3], ray2[3];
  np_unproject(c1.cam_type, c1.cam[s1], o1.x, o1.y, xn1);   // :715-716
  np_unproject(c2.cam_type, c2.cam[s2], o2.x, o2.y, xn2);
  np_rotate_to_world(Tcw1, xn1, ray1);
  np_rotate_to_world(Tcw2, xn2, ray2);
  // ray1.dot(ray2) / (cv::norm(ray1) * cv::norm(ray2)): three doubles, rounded once into the float (:726)
  const float cosParallaxRays = (float)(dot3_double(ray1, ray2) / (__builtin_sqrt(dot3_double(ray1, ray1)) * __builtin_sqrt(dot3_double(ray2, ray2))));
  const float cosParallaxStereo0 = cosParallaxRays + 1;
  float cosParallaxStereo1 = cosParallaxStereo0, cosParallaxStereo2 = cosParallaxStereo0;
  if (bStereo1) cosParallaxStereo1 = np_cos_parallax_stereo(c1.mb, o1.depth);
  else if (bStereo2) cosParallaxStereo2 = np_cos_parallax_stereo(c2.mb, o2.depth);
  const float cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;   // std::min(1, 2)
  float x3D[3];
  if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || (double)cosParallaxRays < 0.9998)) {
    float At[4][4];   // column k of A (:751-754)
#pragma unroll
    for (int k = 0; k < 4; k++) {
      At[k][0] = xn1[0] * Tcw1[8 + k] - Tcw1[k];
      At[k][1] = xn1[1] * Tcw1[8 + k] - Tcw1[4 + k];
      At[k][2] = xn2[0] * Tcw2[8 + k] - Tcw2[k];
      At[k][3] = xn2[1] * Tcw2[8 + k] - Tcw2[4 + k];
    }
    float v[4];
    jacobi_svd4_last_row(At, v, nullptr);
    if (v[3] == 0) return ORBM_NP_ZERO_W;   // :762
    const double inv = 1.0 / (double)v[3];
#pragma unroll
    for (int k = 0; k < 3; k++) x3D[k] = (float)((double)v[k] * inv);
  } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
    if (!np_unproject_stereo(c1, o1, x3D)) return ORBM_NP_EMPTY_STEREO;   // :788
  } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
    if (!np_unproject_stereo(c2, o2, x3D)) return ORBM_NP_EMPTY_STEREO;
  } else {
    return ORBM_NP_LOW_PARALLAX;   // :782
  }
  const float z1 = np_row_dot(Tcw1, 2, x3D);
  if (z1 <= 0) return ORBM_NP_BEHIND1;
  const float z2 = np_row_dot(Tcw2, 2, x3D);
  if (z2 <= 0) return ORBM_NP_BEHIND2;
  if (np_reprojection_fails(c1, s1, bStereo1, c1.mbf, Tcw1, x3D, z1, o1)) return bStereo1 ? ORBM_NP_REPROJ1_STEREO : ORBM_NP_REPROJ1;
  if (np_reprojection_fails(c2, s2, bStereo2, c1.mbf, Tcw2, x3D, z2, o2)) return bStereo2 ? ORBM_NP_REPROJ2_STEREO : ORBM_NP_REPROJ2;
  const float normal1[3] = {x3D[0] - Ow1[0], x3D[1] - Ow1[1], x3D[2] - Ow1[2]};
  const float normal2[3] = {x3D[0] - Ow2[0], x3D[1] - Ow2[1], x3D[2] - Ow2[2]};
  const float dist1 = norm3(normal1), dist2 = norm3(normal2);
  if (dist1 == 0 || dist2 == 0) return ORBM_NP_ZERO_DIST;
  if (far_points && (dist1 >= th_far_points || dist2 >= th_far_points)) return ORBM_NP_FAR;
  const float ratioFactor = 1.5f * scale_factor1;   // :521
  const float ratioDist = dist2 / dist1;
  const float ratioOctave = c1.sf[o1.octave & (ORBX_MAX_LEVELS - 1)] / c2.sf[o2.octave & (ORBX_MAX_LEVELS - 1)];
  if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return ORBM_NP_SCALE;
  x3D_out[0] = x3D[0]; x3D_out[1] = x3D[1]; x3D_out[2] = x3D[2];
  return ORBM_NP_ACCEPTED;
}

#undef ORB_REF
