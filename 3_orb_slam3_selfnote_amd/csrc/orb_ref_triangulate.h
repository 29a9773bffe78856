// orb_ref_triangulate.h -- the reference's fisheye-stereo triangulation (Frame::ComputeStereoFishEyeMatches, Frame.cc:1252-1266;
// KannalaBrandt8::unproject / Triangulate / TriangulateMatches, KannalaBrandt8.cpp:112-139, :343-444), each expression stated once
// for the host entry points of orbhip.hip and the kernels of orb_rig_stereo_kernels.h, under the contract of orb_ref_geometry.h: IEEE-754
// single / double operations in the reference's order, no contraction, correctly rounded fp32 divide / sqrt, libm through the
// glibc replicas.  The double divides and square roots are the `/` operator and __builtin_sqrt: without fast-math the device compiler
// expands both to its correctly rounded sequences (v_div_scale / v_div_fmas / v_div_fixup, and the v_rsq_f64 iteration with its two
// residual corrections), never to the approximate forms; tests/test_gpu_rig_stereo.py compares the device with the host bit for bit.
#pragma once
#include <float.h>
#include "orb_ref_geometry.h"
#include "orb_tanf.h"

#define ORB_REF __host__ __device__ __forceinline__

// KannalaBrandt8::unproject (KannalaBrandt8.cpp:112-139): p = {fx, fy, cx, cy, k0..k3}; ray[2] = 1
ORB_REF void kb8_unproject(const float *p, float px, float py, float *ray) {
  const float pwx = (px - p[2]) / p[0], pwy = (py - p[3]) / p[1];
  float scale = 1.f;
  float theta_d = sqrtf(pwx * pwx + pwy * pwy);
  // fminf(fmaxf(-CV_PI / 2.f, theta_d), CV_PI / 2.f): the double constants are converted to float by the calls
  theta_d = __builtin_fminf(__builtin_fmaxf((float)(-3.1415926535897932384626433832795 / 2.), theta_d), (float)(3.1415926535897932384626433832795 / 2.));
  if ((double)theta_d > 1e-8) {
    float theta = theta_d;
    for (int j = 0; j < 10; j++) {
      const float theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2, theta8 = theta4 * theta4;
      const float k0_theta2 = p[4] * theta2, k1_theta4 = p[5] * theta4;
      const float k2_theta6 = p[6] * theta6, k3_theta8 = p[7] * theta8;
      const float theta_fix = (theta * (1.f + k0_theta2 + k1_theta4 + k2_theta6 + k3_theta8) - theta_d) /
                              (1.f + 3.f * k0_theta2 + 5.f * k1_theta4 + 7.f * k2_theta6 + 9.f * k3_theta8);
      theta = theta - theta_fix;
      if (__builtin_fabsf(theta_fix) < 1e-6f) break;   // KannalaBrandt8::precision
    }
    scale = orbtn::ref_tanf(theta) / theta_d;   // std::tan(float) -> tanf, :135
  }
  ray[0] = pwx * scale; ray[1] = pwy * scale; ray[2] = 1.f;
}

// OpenCV's hypot helper of lapack.cpp: the larger magnitude times sqrt(1 + ratio^2)
ORB_REF double cv_hypot(double a, double b) {
  a = __builtin_fabs(a); b = __builtin_fabs(b);
  if (a > b) { b /= a; return a * __builtin_sqrt(1 + b * b); }
  if (b > 0) { a /= b; return b * __builtin_sqrt(1 + a * a); }
  return 0;
}

// Sum of squares / product of two rows of four floats, accumulated in double
ORB_REF double row4_dot(const float *a, const float *b) {
  double d = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) d += (double)a[k] * (double)b[k];
  return d;
}

// [OPENCV-UNVERIFIED] cv::SVD::compute of a 4x4 CV_32F matrix as OpenCV's OWN one-sided Jacobi does it (JacobiSVDImpl_<float>,
// modules/core/src/lapack.cpp; an OpenCV built with LAPACK calls sgesdd instead and gives other low bits, so the reference itself is
// unpinned here): the method works on At = A^T (rows = columns of A) and V = I.  Returns row 3 of vt, the right singular vector of
// the smallest singular value, in v; *sweeps = sweeps that rotated (the iteration cap is max(m, 30) = 30).
// Departure in form, not in value: the final selection sort moves an index in place of the rows of At and V.
ORB_REF void jacobi_svd4_last_row(float At[4][4], float *v, int *sweeps) {
  float V[4][4];
  double W[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    W[i] = row4_dot(At[i], At[i]);
#pragma unroll
    for (int k = 0; k < 4; k++) V[i][k] = i == k ? 1.f : 0.f;
  }
  const float eps = FLT_EPSILON * 2;
  int nsweeps = 0;
  for (int iter = 0; iter < 30; iter++) {
    bool changed = false;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = i + 1; j < 4; j++) {
        double a = W[i], b = W[j];
        double p = row4_dot(At[i], At[j]);
        if (__builtin_fabs(p) <= (double)eps * __builtin_sqrt(a * b)) continue;
        p *= 2;
        const double beta = a - b, gamma = cv_hypot(p, beta);
        float c, s;
        if (beta < 0) {
          const double delta = (gamma - beta) * 0.5;
          s = (float)__builtin_sqrt(delta / gamma);
          c = (float)(p / (gamma * (double)s * 2));
        } else {
          c = (float)__builtin_sqrt((gamma + beta) / (gamma * 2));
          s = (float)(p / (gamma * (double)c * 2));
        }
        a = b = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const float t0 = c * At[i][k] + s * At[j][k];
          const float t1 = -s * At[i][k] + c * At[j][k];
          At[i][k] = t0; At[j][k] = t1;
          a += (double)t0 * (double)t0; b += (double)t1 * (double)t1;
        }
        W[i] = a; W[j] = b;
        changed = true;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const float t0 = c * V[i][k] + s * V[j][k];
          const float t1 = -s * V[i][k] + c * V[j][k];
          V[i][k] = t0; V[j][k] = t1;
        }
      }
    if (!changed) break;
    nsweeps++;
  }
#pragma unroll
  for (int i = 0; i < 4; i++) W[i] = __builtin_sqrt(row4_dot(At[i], At[i]));
  // selection sort, descending, first maximum on ties: which original row ends up last
  int perm[4] = {0, 1, 2, 3};
#pragma unroll
  for (int i = 0; i < 3; i++) {
    int j = i;
    double wj = W[i];
    int pj = perm[i];
#pragma unroll
    for (int k = i + 1; k < 4; k++)
      if (wj < W[k]) { j = k; wj = W[k]; pj = perm[k]; }
#pragma unroll
    for (int k = i + 1; k < 4; k++)
      if (j == k) { W[k] = W[i]; perm[k] = perm[i]; }
    W[i] = wj; perm[i] = pj;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) v[k] = perm[3] == 0 ? V[0][k] : perm[3] == 1 ? V[1][k] : perm[3] == 2 ? V[2][k] : V[3][k];
  if (sweeps) *sweeps = nsweeps;
}

// KannalaBrandt8::Triangulate (KannalaBrandt8.cpp:431-444) for Tcw1 = [I | 0] and Tcw2 (3x4, row stride 4).  [OPENCV-UNVERIFIED]:
// a row `p * T.row(2) - T.row(i)` is one scaled addition in float, product rounded, then the difference; x3D = vt.row(3)[0..2] /
// vt.row(3)[3] is OpenCV's matrix-by-scalar division, each entry (float)((double)v * (1.0 / (double)w)).
ORB_REF void kb8_triangulate(float p1x, float p1y, float p2x, float p2y, const float *Tcw2, float *x3D, int *sweeps) {
  const float Tcw1[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
  float At[4][4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    At[k][0] = p1x * Tcw1[8 + k] - Tcw1[k];
    At[k][1] = p1y * Tcw1[8 + k] - Tcw1[4 + k];
    At[k][2] = p2x * Tcw2[8 + k] - Tcw2[k];
    At[k][3] = p2y * Tcw2[8 + k] - Tcw2[4 + k];
  }
  float v[4];
  jacobi_svd4_last_row(At, v, sweeps);
  const double inv = 1.0 / (double)v[3];
#pragma unroll
  for (int k = 0; k < 3; k++) x3D[k] = (float)((double)v[k] * inv);
}

// The rig's constant part of TriangulateMatches (:372-374) from Tlr = [R12 | t12] (3x4, row stride 4): Tcw2 = [R21 | t21] with
// R21 = R12.t() and t21 = -R21 * t12, a cv::gemm with alpha = -1 on the small-matrix float path (the sum of mat3_mul_add, negated)
ORB_REF void rig_Tcw2(const float *Tlr, float *Tcw2) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) Tcw2[4 * i + j] = Tlr[4 * j + i];
    const float t0 = Tlr[i] * Tlr[3] + Tlr[4 + i] * Tlr[7] + Tlr[8 + i] * Tlr[11];
    Tcw2[4 * i + 3] = (float)((double)t0 * -1.0 + 0.0);   // t0 * alpha + c * beta with no C: a zero sum stays +0
  }
}

// KannalaBrandt8::TriangulateMatches (:343-412): the depth z1 in the left camera or -1; p3D is written only with a depth.
ORB_REF float kb8_triangulate_matches(const float *cam1, const float *cam2, float k1x, float k1y, float k2x, float k2y, const float *Tlr,
                                      const float *Tcw2, float sigmaLevel, float unc, float *p3D) {
  float r1[3], r2[3], r21[3];
  kb8_unproject(cam1, k1x, k1y, r1);
  kb8_unproject(cam2, k2x, k2y, r2);
  const float zero3[3] = {0.f, 0.f, 0.f};
  mat3_mul_add(Tlr, r2, zero3, r21);   // R12 * r2 (:348)
  // r1.dot(r21) / (cv::norm(r1) * cv::norm(r21)): three doubles, rounded once into the float (:350)
  const float cosParallaxRays = (float)(dot3_double(r1, r21) / (__builtin_sqrt(dot3_double(r1, r1)) * __builtin_sqrt(dot3_double(r21, r21))));
  if ((double)cosParallaxRays > 0.9998) return -1.f;
  float x3D[3];
  kb8_triangulate(r1[0], r1[1], r2[0], r2[1], Tcw2, x3D, nullptr);
  const float z1 = x3D[2];
  if (z1 <= 0) return -1.f;
  const float R21row2[3] = {Tcw2[8], Tcw2[9], Tcw2[10]};
  const float z2 = (float)(dot3_double(R21row2, x3D) + (double)Tcw2[11]);   // :384
  if (z2 <= 0) return -1.f;
  float u, v;
  project(1, cam1, x3D[0], x3D[1], x3D[2], u, v);
  const float errX1 = u - k1x, errY1 = v - k1y;
  if ((double)(errX1 * errX1 + errY1 * errY1) > 5.991 * (double)sigmaLevel) return -1.f;
  float x3D2[3];
  const float t21[3] = {Tcw2[3], Tcw2[7], Tcw2[11]};
  mat3_mul_add(Tcw2, x3D, t21, x3D2);   // R21 * x3D + t21 (:399)
  project(1, cam2, x3D2[0], x3D2[1], x3D2[2], u, v);
  const float errX2 = u - k2x, errY2 = v - k2y;
  if ((double)(errX2 * errX2 + errY2 * errY2) > 5.991 * (double)unc) return -1.f;
  p3D[0] = x3D[0]; p3D[1] = x3D[1]; p3D[2] = x3D[2];
  return z1;
}

// Lowe's ratio test of Frame.cc:1253 on two Hamming distances: DMatch::distance is a float, the product with 0.7 a double
ORB_REF bool fisheye_ratio_test(int d0, int d1) { return (double)(float)d0 < (double)(float)d1 * 0.7; }

#undef ORB_REF
