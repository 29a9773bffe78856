// orb_ref_sim3.h -- Sim3Solver (Sim3Solver.cc:35-530): the constructor's camera coordinates, projections and thresholds, ComputeCentroid,
// ComputeSim3 (Horn's closed form), Project, CheckInliers, SetRansacParameters and the running best of iterate, each expression stated
// once for the host entry points of orbhip.hip and the kernels of orb_sim3_kernels.h, under the contract of orb_ref_geometry.h: IEEE-754
// single / double operations in the reference's order, no contraction, correctly rounded fp32 divide and sqrt.
//   * The double libm calls of ComputeSim3 (atan2 :392, and the sin / cos inside cv::Rodrigues :398) and of SetRansacParameters (pow, log
//     :169) have no device replica pinned against glibc: sim3_tail and sim3_ransac_iterations are host-only, and the device stage ends at
//     the quaternion (sim3_quaternion).
//   * cv::Mat expressions are folded as DESIGN.md section 2 folds them, every form [OPENCV-UNVERIFIED]:
//       cv::reduce(P,C,1,SUM)   3 float columns: (c0 + c2) + c1 in float (two accumulators, the second added last)    sim3_centroid
//       C/P.cols                (float)((double)v * (1.0 / 3))
//       Pr2*Pr1.t()             a transposition flag: the generic path, the sum in double, rounded once               tv_mul33_Bt
//       cv::eigen               OpenCV's own two-sided Jacobi for float on the symmetric 4 x 4                        sim3_eigen4
//       cv::norm(vec)           the double root of the double sum of squares, ascending
//       2*ang*vec/norm(vec)     one scale alpha = (2*ang) * (1.0 / norm): (float)((double)v * alpha)
//       cv::Rodrigues           double throughout, c*I + c1*r*rT + s*[r]x per entry, narrowed at the end              sim3_rodrigues
//       mR12i*Pr2               no transposed operand: the small-matrix path, the sum in float                        tv_mul33
//       Pr1.dot(P3)             nine products and their sum in double, row-major
//       cv::pow(P3,2)           p*p in float
//       O1 - ms12i*mR12i*O2     one gemm, alpha = -(double)ms12i, beta = 1: (float)((double)sum*alpha + (double)O1)
//       ms12i*mR12i             (float)((double)v * (double)ms12i)
//       (1.0/ms12i)*mR12i.t()   (float)((double)v * (1.0 / (double)ms12i)) of the transposed entry
//       -sRinv*mt12i            the small-matrix path with alpha = -1
//       dist.dot(dist)          two products and their sum in double, narrowed to float
#pragma once
#include <float.h>
#include "orb_ref_twoview.h"

#define ORB_REF __host__ __device__ __forceinline__

// ---- the constructor, :35-148 ----------------------------------------------------------------------------------------------------------
// mvnMaxError1/2 are std::vector<size_t> (Sim3Solver.h:78-79): 9.210*sigmaSquare is a double product truncated to an integer, and
// err < mvnMaxError[i] compares a float with that integer converted to float (:470).  sigma2 finite, >= 0 and below 2^53 (the entries refuse
// the rest: the conversion is undefined there).
ORB_REF float sim3_max_error(float sigma2) { return (float)(uint64_t)(9.210 * (double)sigma2); }
ORB_REF bool sim3_sigma2_ok(float sigma2) { return sigma2 >= 0.f && sigma2 < 9.0e15f; }

// mvX3Dc.push_back(Rcw*X3Dw+tcw) (:129, :132) and the same form in Project (:506): T row-major with row stride 4, [R | t]
ORB_REF void sim3_transform(const float *T, const float *X, float *out) {
  const float t[3] = {T[3], T[7], T[11]};
  mat3_mul_add(T, X, t, out);
}
// FromCameraToImage (:516-530) and the tail of Project (:507-512): projectMat(cv::Point3f(x, y, z)), both camera models
ORB_REF void sim3_project(int cam_type, const float *cam, const float *Xc, float *uv) { project(cam_type, cam, Xc[0], Xc[1], Xc[2], uv[0], uv[1]); }

// ---- ComputeCentroid, :329-338 ---------------------------------------------------------------------------------------------------------
// P: the three points as COLUMNS (P[3*r + c] = coordinate r of point c), as P3Dc1i / P3Dc2i hold them (:208-209)
ORB_REF void sim3_centroid(const float *P, float *Pr, float *C) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
    float a0 = P[3 * r], a1 = P[3 * r + 1];
    a0 = a0 + P[3 * r + 2];
    a0 = a0 + a1;                                      // cv::reduce(P,C,1,CV_REDUCE_SUM) :331
    C[r] = (float)((double)a0 * (1.0 / 3.0));          // C = C/P.cols :332
  }
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) Pr[3 * r + c] = P[3 * r + c] - C[r];   // :336
}

// ---- cv::eigen of the symmetric 4 x 4 float matrix, :386 -------------------------------------------------------------------------------
// [OPENCV-UNVERIFIED] JacobiImpl_<float> with n = 4: the pivot is the off-diagonal entry of the upper triangle of greatest magnitude, found
// through the per-row (indR) and per-column (indC) maxima, the first of equal magnitudes staying; the loop ends at |p| <= FLT_EPSILON or
// after n*n*30 = 480 rotations; then a descending selection sort.  Eigenvectors are the ROWS of V with the signs the rotations leave.
ORB_REF float sim3_hypot(float a, float b) {
  a = fabsf(a); b = fabsf(b);
  if (a > b) { b /= a; return a * sqrtf(1 + b * b); }
  if (b > 0) { a /= b; return b * sqrtf(1 + a * a); }
  return 0;
}
ORB_REF int sim3_row_max(const float *A, int k) {      // argmax |A[k][i]|, i > k  (k < 3)
  int m = k + 1;
  float mv = fabsf(A[4 * k + m]);
  for (int i = k + 2; i < 4; i++) { const float val = fabsf(A[4 * k + i]); if (mv < val) { mv = val; m = i; } }
  return m;
}
ORB_REF int sim3_col_max(const float *A, int k) {      // argmax |A[i][k]|, i < k  (k > 0)
  int m = 0;
  float mv = fabsf(A[k]);
  for (int i = 1; i < k; i++) { const float val = fabsf(A[4 * i + k]); if (mv < val) { mv = val; m = i; } }
  return m;
}
#define SIM3_ROTATE(v0, v1) { const float a0 = v0, b0 = v1; v0 = a0 * c - b0 * s; v1 = a0 * s + b0 * c; }
// Workspace of one call: SIM3_WS_FLOATS floats (A, V, W) and SIM3_WS_INTS ints (indR, indC).  The pivot's indices are data, so every
// access is at a computed address: the kernel keeps the workspace in LDS (in registers each access is a chain of selects).
#define SIM3_WS_FLOATS 36
#define SIM3_WS_INTS 8
ORB_REF void sim3_eigen4(float *A, float *W, float *V, int *indR) {   // A [16] is destroyed; W [4] descending; V [16] rows = eigenvectors
  const float eps = FLT_EPSILON;
  int *indC = indR + 4;
  for (int i = 0; i < 16; i++) V[i] = 0.f;
  for (int i = 0; i < 4; i++) V[5 * i] = 1.f;
  for (int k = 0; k < 4; k++) {
    W[k] = A[5 * k];
    indR[k] = indC[k] = 0;
    if (k < 3) indR[k] = sim3_row_max(A, k);
    if (k > 0) indC[k] = sim3_col_max(A, k);
  }
  for (int iters = 0; iters < 4 * 4 * 30; iters++) {
    int k = 0;
    float mv = fabsf(A[indR[0]]);
    for (int i = 1; i < 3; i++) { const float val = fabsf(A[4 * i + indR[i]]); if (mv < val) { mv = val; k = i; } }
    int l = indR[k];
    for (int i = 1; i < 4; i++) { const float val = fabsf(A[4 * indC[i] + i]); if (mv < val) { mv = val; k = indC[i]; l = i; } }
    const float p = A[4 * k + l];
    if (fabsf(p) <= eps) break;
    const float y = (float)((double)(W[l] - W[k]) * 0.5);
    float t = fabsf(y) + sim3_hypot(p, y);
    float s = sim3_hypot(p, t);
    const float c = t / s;
    s = p / s; t = (p / t) * p;
    if (y < 0) { s = -s; t = -t; }
    A[4 * k + l] = 0;
    W[k] -= t;
    W[l] += t;
    for (int i = 0; i < k; i++) SIM3_ROTATE(A[4 * i + k], A[4 * i + l]);
    for (int i = k + 1; i < l; i++) SIM3_ROTATE(A[4 * k + i], A[4 * i + l]);
    for (int i = l + 1; i < 4; i++) SIM3_ROTATE(A[4 * k + i], A[4 * l + i]);
    for (int i = 0; i < 4; i++) SIM3_ROTATE(V[4 * k + i], V[4 * l + i]);
    for (int j = 0; j < 2; j++) {
      const int idx = j == 0 ? k : l;
      if (idx < 3) indR[idx] = sim3_row_max(A, idx);
      if (idx > 0) indC[idx] = sim3_col_max(A, idx);
    }
  }
  for (int k = 0; k < 3; k++) {
    int m = k;
    for (int i = k + 1; i < 4; i++)
      if (W[m] < W[i]) m = i;
    if (k != m) {
      const float w = W[m]; W[m] = W[k]; W[k] = w;
      for (int i = 0; i < 4; i++) { const float v = V[4 * m + i]; V[4 * m + i] = V[4 * k + i]; V[4 * k + i] = v; }
    }
  }
}
#undef SIM3_ROTATE

// ---- ComputeSim3 up to the quaternion, :345-386 ----------------------------------------------------------------------------------------
// What the tail needs of one set besides the quaternion: Pr1, Pr2 and both centroids
struct Sim3Set { float Pr1[9], Pr2[9], O1[3], O2[3]; };
ORB_REF void sim3_quaternion(const float *P1, const float *P2, Sim3Set &S, float *q, float *ws, int *iw) {
  sim3_centroid(P1, S.Pr1, S.O1);                      // :352
  sim3_centroid(P2, S.Pr2, S.O2);                      // :353
  float M[9];
  tv_mul33_Bt(S.Pr2, S.Pr1, M);                        // M = Pr2*Pr1.t() :357
  // :365-374: float expressions left to right, assigned to double, narrowed into the Mat_<float> (:376): the float value itself
  const float N11 = M[0] + M[4] + M[8], N12 = M[5] - M[7], N13 = M[6] - M[2], N14 = M[1] - M[3];
  const float N22 = M[0] - M[4] - M[8], N23 = M[1] + M[3], N24 = M[6] + M[2];
  const float N33 = -M[0] + M[4] - M[8], N34 = M[5] + M[7], N44 = -M[0] - M[4] + M[8];
  float *N = ws, *V = ws + 16, *W = ws + 32;
  N[0] = N11; N[1] = N12; N[2] = N13; N[3] = N14; N[4] = N12; N[5] = N22; N[6] = N23; N[7] = N24;
  N[8] = N13; N[9] = N23; N[10] = N33; N[11] = N34; N[12] = N14; N[13] = N24; N[14] = N34; N[15] = N44;
  sim3_eigen4(N, W, V, iw);                            // :386
#pragma unroll
  for (int k = 0; k < 4; k++) q[k] = V[k];             // evec.row(0)
}

// ---- Project and CheckInliers for one pair, :454-514 -----------------------------------------------------------------------------------
// err = dist.dot(dist) narrowed to float (:467-468)
ORB_REF float sim3_err(const float *a, const float *b) {
  const float dx = a[0] - b[0], dy = a[1] - b[1];
  double d = 0;
  d += (double)dx * (double)dx;
  d += (double)dy * (double)dy;
  return (float)d;
}
// X1 / X2: mvX3Dc1[i] / mvX3Dc2[i]; im1 / im2: mvP1im1[i] / mvP2im2[i]; th1 / th2: sim3_max_error of the pair.  A non-finite error
// compares false: no inlier (:470)
ORB_REF bool sim3_inlier(const float *T12, const float *T21, int cam1, const float *p1, int cam2, const float *p2, const float *X1,
                         const float *X2, const float *im1, const float *im2, float th1, float th2) {
  float Xc[3], uv21[2], uv12[2];
  sim3_transform(T12, X2, Xc);                         // Project(mvX3Dc2,vP2im1,mT12i,pCamera1) :457
  sim3_project(cam1, p1, Xc, uv21);
  sim3_transform(T21, X1, Xc);                         // Project(mvX3Dc1,vP1im2,mT21i,pCamera2) :458
  sim3_project(cam2, p2, Xc, uv12);
  const float err1 = sim3_err(im1, uv21);              // dist1 = mvP1im1[i]-vP2im1[i] :464
  const float err2 = sim3_err(uv12, im2);              // dist2 = vP1im2[i]-mvP2im2[i] :465
  return err1 < th1 && err2 < th2;
}

// ---- the running best of iterate, :194-237 / :267-315 (include/orbhip.h, SIM3 RULE) -----------------------------------------------------
// One ordered pass over the independent counts.  done / max_its: mnIterations at entry and mRansacMaxIts.
struct Sim3Pass { int converged, it_stop, best_it, best_inliers, improved, no_more; };
// how many iterations the loop can run at the most: `mnIterations<mRansacMaxIts && nCurrentIterations<nIterations` (:194, :267)
ORB_REF int sim3_pass_limit(int iterations, int done, int max_its) {
  const int left = max_its > done ? max_its - done : 0;
  return iterations < left ? iterations : left;
}
ORB_REF Sim3Pass sim3_pass_begin(int best_in) { return Sim3Pass{0, 0, -1, best_in, 0, 0}; }
// one iteration with count c; false where the loop ends
ORB_REF bool sim3_pass_take(Sim3Pass &R, int c, int min_inliers) {
  R.it_stop++;
  if (c >= R.best_inliers) {                           // :219, :292: of equal counts the later iteration wins
    R.best_inliers = c; R.best_it = R.it_stop - 1; R.improved = 1;
    if (c > min_inliers) { R.converged = 1; return false; }   // :228, :301: strictly
  }
  return true;
}
ORB_REF void sim3_pass_end(Sim3Pass &R, int done, int max_its) {
  if (!R.converged && done + R.it_stop >= max_its) R.no_more = 1;   // :239, :317
}
ORB_REF Sim3Pass sim3_ordered_pass(const int32_t *counts, int iterations, int best_in, int min_inliers, int done, int max_its) {
  Sim3Pass R = sim3_pass_begin(best_in);
  const int limit = sim3_pass_limit(iterations, done, max_its);
  for (int k = 0; k < limit; k++)
    if (!sim3_pass_take(R, counts[k], min_inliers)) break;
  sim3_pass_end(R, done, max_its);
  return R;
}

// ---- host only: the double-libm tail of ComputeSim3, :388-450 ---------------------------------------------------------------------------
// cv::Rodrigues (:398) for a CV_32F 3-vector: [OPENCV-UNVERIFIED] the vector widened to double, theta = sqrt(x*x + y*y + z*z); below
// DBL_EPSILON the identity; else c*I + (1 - c)*r*rT + s*[r]x with r = v * (1/theta), per entry (c*I + c1*rrt) + s*rx, narrowed to float.
// The member feeds it a finite vector of norm <= 2 pi, or a NaN vector (norm(vec) == 0: an exact identity rotation, or a coincident set):
// NaN is not below DBL_EPSILON, so every entry is NaN.
static inline void sim3_rodrigues(const float *v, float *R) {
  double rx = v[0], ry = v[1], rz = v[2];
  const double theta = sqrt(rx * rx + ry * ry + rz * rz);
  if (theta < DBL_EPSILON) {
    for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? 1.f : 0.f;
    return;
  }
  const double c = cos(theta), s = sin(theta), c1 = 1. - c, itheta = theta ? 1. / theta : 0.;
  rx *= itheta; ry *= itheta; rz *= itheta;
  const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
  const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
  const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int k = 0; k < 9; k++) R[k] = (float)(c * I[k] + c1 * rrt[k] + s * r_x[k]);
}
// One hypothesis behind its quaternion.  R12 [9], t12 [3], s12, T12 [16], T21 [16]
struct Sim3Hyp { float R[9], t[3], s, T12[16], T21[16]; };
static inline void sim3_tail(const Sim3Set &S, const float *q, bool fix_scale, Sim3Hyp &H) {
  const float vec[3] = {q[1], q[2], q[3]};             // :389
  const double nrm = sqrt(dot3_double(vec, vec));
  const double ang = atan2(nrm, (double)q[0]);         // :392
  const double alpha = (2 * ang) * (1.0 / nrm);        // vec = 2*ang*vec/norm(vec) :394
  float aa[3];
  for (int k = 0; k < 3; k++) aa[k] = (float)((double)vec[k] * alpha);
  sim3_rodrigues(aa, H.R);                             // :398
  float P3[9];
  tv_mul33(H.R, S.Pr2, 1.0, P3);                       // P3 = mR12i*Pr2 :402
  if (!fix_scale) {
    double nom = 0, den = 0;
    for (int k = 0; k < 9; k++) nom += (double)S.Pr1[k] * (double)P3[k];   // Pr1.dot(P3) :408
    for (int k = 0; k < 9; k++) den += (double)(P3[k] * P3[k]);            // cv::pow(P3,2,aux_P3), the row-major sum :411-420
    H.s = (float)(nom / den);                          // :422
  } else {
    H.s = 1.0f;
  }
  for (int i = 0; i < 3; i++) {                        // mt12i = O1 - ms12i*mR12i*O2 :430
    float t0 = H.R[3 * i] * S.O2[0];
    t0 = t0 + H.R[3 * i + 1] * S.O2[1];
    t0 = t0 + H.R[3 * i + 2] * S.O2[2];
    H.t[i] = (float)((double)t0 * (-(double)H.s) + (double)S.O1[i] * 1.0);
  }
  for (int k = 0; k < 16; k++) H.T12[k] = H.T21[k] = (k % 5 == 0) ? 1.f : 0.f;   // :435, :444
  float sRinv[9];
  const double inv = 1.0 / (double)H.s;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      H.T12[4 * i + j] = (float)((double)H.R[3 * i + j] * (double)H.s);           // sR :437
      sRinv[3 * i + j] = (float)((double)H.R[3 * j + i] * inv);                   // sRinv :446
      H.T21[4 * i + j] = sRinv[3 * i + j];
    }
  for (int i = 0; i < 3; i++) {
    H.T12[4 * i + 3] = H.t[i];                         // :440
    float t0 = sRinv[3 * i] * H.t[0];
    t0 = t0 + sRinv[3 * i + 1] * H.t[1];
    t0 = t0 + sRinv[3 * i + 2] * H.t[2];
    H.T21[4 * i + 3] = (float)((double)t0 * -1.0 + 0.0);                          // tinv = -sRinv*mt12i :449
  }
}

// (int) of a double as the reference build converts it (x86 cvttsd2si): NaN and values outside the int range give INT_MIN
static inline int sim3_cvtt_f64_i32(double x) { return (x != x || x >= 2147483648.0 || x < -2147483648.0) ? (int)0x80000000u : (int)x; }
// SetRansacParameters (:150-174): the value mRansacMaxIts is left with
static inline int sim3_ransac_iterations(double probability, int min_inliers, int max_its, int N) {
  const float epsilon = (float)min_inliers / N;        // :161
  int nIterations;
  if (min_inliers == N) nIterations = 1;               // :166
  else nIterations = sim3_cvtt_f64_i32(ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3.0))));   // :169
  const int lo = nIterations < max_its ? nIterations : max_its;
  return lo > 1 ? lo : 1;                              // :171
}

#undef ORB_REF
