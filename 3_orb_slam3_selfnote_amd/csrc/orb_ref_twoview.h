// orb_ref_twoview.h -- TwoViewReconstruction::Reconstruct (TwoViewReconstruction.cc:39-127) and every member it calls (:129-933), each
// expression stated once for the host entry points of orbhip.hip and the kernels of orb_twoview_kernels.h, under the contract of
// orb_ref_geometry.h: IEEE-754 single / double operations in the reference's order, no contraction, correctly rounded fp32 divide and
// sqrt.  No libm replica is needed: sqrt on floats is sqrtf (the overload the file gets through <cmath>), and the one
// acos (:905) is evaluated on the host from one value per hypothesis.
//   * cv::Mat expressions are folded as DESIGN.md section 2 folds them, every form [OPENCV-UNVERIFIED]:
//       A*B, s*A*B         3 x 3 (or 3 x 4 / 3 x 1 right operand), no transposed operand: the small-matrix path, the sum of products in
//                          float, then (float)((double)sum*alpha + 0.0)                                              tv_mul33
//       A.t()*B, A*B.t()   a gemm with a transposition flag: the generic path, the sum in double, rounded once        tv_mul33_tA / _Bt
//       A.inv()            3 x 3: cofactors and determinant in double, each entry rounded once, det == 0: zeros      tv_inv33
//       cv::determinant    3 x 3 CV_32F: the cofactor expansion along the first row in double                        tv_det33
//       Mat::diag(w)       the 3 x 3 matrix with w on its diagonal, then an ordinary operand
//       t/cv::norm(t)      (float)((double)v * (1.0 / norm)), norm the double root of the double sum of squares
//       tp *= d            (float)((double)v * (double)d)
//       cv::SVD::compute   OpenCV's own one-sided Jacobi for float, for any small m x n                               tv_jacobi_svd
//   * vn (the plane normals of ReconstructH, :643-651, :681-689) is not formed: nothing reads it.
#pragma once
#include <float.h>
#include "orb_ref_triangulate.h"

#define ORB_REF __host__ __device__ __forceinline__

// One code per `continue` of CheckRT's loop (:834-898); include/orbhip.h has the same values as ORBM_TV_*
enum { TV_NOT_INLIER = 0, TV_GOOD = 1, TV_LOW_PARALLAX = 2, TV_NONFINITE = 3, TV_BEHIND1 = 4, TV_BEHIND2 = 5, TV_REPROJ1 = 6, TV_REPROJ2 = 7 };

// Floats of workspace one SVD of ComputeH21 / ComputeF21 needs: At (9 rows of 16), Vt (9 x 9), w (9); and 9 doubles of W
#define TV_WS_FLOATS (9 * 16 + 81 + 9)
#define TV_WS_DOUBLES 9

// ---- the small-matrix forms (3 x 3, row-major, row stride 3) ----------------------------------------------------------------------
// D = alpha*A*B on the small-matrix path of cv::gemm; D must not alias A or B
ORB_REF void tv_mul33(const float *A, const float *B, double alpha, float *D) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      float s = A[3 * i] * B[j];
      s = s + A[3 * i + 1] * B[3 + j];
      s = s + A[3 * i + 2] * B[6 + j];
      D[3 * i + j] = (float)((double)s * alpha + 0.0);
    }
}
// d = A*b, b a 3 x 1 column: the same path
ORB_REF void tv_mul31(const float *A, const float *b, float *d) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    float s = A[3 * i] * b[0];
    s = s + A[3 * i + 1] * b[1];
    s = s + A[3 * i + 2] * b[2];
    d[i] = (float)((double)s * 1.0 + 0.0);
  }
}
// D = alpha*A.t()*B, B with `cols` columns (row stride cols): the generic path (K.t()*F21 :484, -R.t()*t :830)
ORB_REF void tv_mul33_tA(const float *A, const float *B, int cols, double alpha, float *D) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < cols; j++) {
      double acc = 0;
      for (int k = 0; k < 3; k++) acc += (double)A[3 * k + i] * (double)B[cols * k + j];
      D[cols * i + j] = (float)(alpha * acc);
    }
}
// D = A*B.t(): the generic path (u*W.t() :930)
ORB_REF void tv_mul33_Bt(const float *A, const float *B, float *D) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double acc = 0;
#pragma unroll
      for (int k = 0; k < 3; k++) acc += (double)A[3 * i + k] * (double)B[3 * j + k];
      D[3 * i + j] = (float)acc;
    }
}
// cv::determinant of a 3 x 3 CV_32F matrix
ORB_REF double tv_det33(const float *A) {
  const double a = A[0], b = A[1], c = A[2], d = A[3], e = A[4], f = A[5], g = A[6], h = A[7], i = A[8];
  return a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
}
// cv::invert(DECOMP_LU) of a 3 x 3 CV_32F matrix (T2.inv() :139, H21i.inv() :166, K.inv() :588)
ORB_REF void tv_inv33(const float *A, float *D) {
  double s[3][3], cof[3][3];
#pragma unroll
  for (int y = 0; y < 3; y++)
#pragma unroll
    for (int x = 0; x < 3; x++) s[y][x] = (double)A[3 * y + x];
#pragma unroll
  for (int y = 0; y < 3; y++)
#pragma unroll
    for (int x = 0; x < 3; x++) {
      const int r0 = (x + 1) % 3, r1 = (x + 2) % 3, c0 = (y + 1) % 3, c1 = (y + 2) % 3;
      cof[y][x] = s[r0][c0] * s[r1][c1] - s[r0][c1] * s[r1][c0];
    }
  double d = s[0][0] * (s[1][1] * s[2][2] - s[1][2] * s[2][1]) - s[0][1] * (s[1][0] * s[2][2] - s[1][2] * s[2][0]) +
             s[0][2] * (s[1][0] * s[2][1] - s[1][1] * s[2][0]);
  if (d == 0.) {
#pragma unroll
    for (int k = 0; k < 9; k++) D[k] = 0.f;
    return;
  }
  d = 1. / d;
#pragma unroll
  for (int y = 0; y < 3; y++)
#pragma unroll
    for (int x = 0; x < 3; x++) D[3 * y + x] = (float)(cof[y][x] * d);
}
// v / cv::norm(v) for a 3-vector (:641, :679, :919)
ORB_REF void tv_unit3(const float *v, float *out) {
  const double inv = 1.0 / __builtin_sqrt(dot3_double(v, v));
#pragma unroll
  for (int k = 0; k < 3; k++) out[k] = (float)((double)v[k] * inv);
}

// ---- cv::SVD::compute for any small m x n ------------------------------------------------------------------------------------------
// [OPENCV-UNVERIFIED] OpenCV's own one-sided Jacobi for float (JacobiSVDImpl_<float>), the general form of jacobi_svd4_last_row: the n
// rows (length m, row stride m) of At are rotated against each other, the rotations gathered in the n x n Vt; sums of products in double
// in ascending index, c / s rounded to float, max(m, 30) sweeps, a descending selection sort in which the first of equal values stays.
// Then rows 0 .. n1-1 of At leave as unit vectors: a row over its length, and for a length <= FLT_MIN or a row beyond n a pseudo-random
// vector (multiply-with-carry, seeded 0x12345678 once per call) made orthogonal to the rows in front of it in two passes.  n1 = 0
// leaves At unscaled: the caller reads Vt and w only.  W: n doubles of workspace; w: the n singular values.
// For an m x n matrix A with m >= n: At = A.t(), n1 = m (FULL_UV), u = At.t(), vt = Vt.  With m < n: At = A with the roles swapped.
//
// `lanes` says who runs the function.  TvSolo: one thread.  A group of lanes that share At, W, Vt and w (orb_twoview_kernels.h): every lane
// runs everything and stores the same values, except the element updates of a rotation, of which a lane takes the elements first(),
// first() + step(), ...; sync() stands between those stores and the sums that read them.  The sums of products stay whole and in
// ascending index in every lane: they are ordered double sums and cannot be split.
struct TvSolo {
  ORB_REF int first() const { return 0; }
  ORB_REF int step() const { return 1; }
  ORB_REF void sync() const {}
};
template <class Lanes>
ORB_REF void tv_jacobi_svd(float *At, double *W, float *Vt, float *w, int m, int n, int n1, const Lanes &lanes) {
  const double minval = FLT_MIN, eps = (double)FLT_EPSILON * 2;
  for (int i = 0; i < n; i++) {
    double sd = 0;
    for (int k = 0; k < m; k++) { const float t = At[i * m + k]; sd += (double)t * (double)t; }
    W[i] = sd;
    for (int k = 0; k < n; k++) Vt[i * n + k] = i == k ? 1.f : 0.f;
  }
  const int max_iter = m > 30 ? m : 30;
  for (int iter = 0; iter < max_iter; iter++) {
    bool changed = false;
    for (int i = 0; i < n - 1; i++)
      for (int j = i + 1; j < n; j++) {
        float *Ai = At + i * m, *Aj = At + j * m;
        double a = W[i], p = 0, b = W[j];
        for (int k = 0; k < m; k++) p += (double)Ai[k] * (double)Aj[k];
        if (__builtin_fabs(p) <= eps * __builtin_sqrt(a * b)) continue;
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
        for (int k = lanes.first(); k < m; k += lanes.step()) {
          const float t0 = c * Ai[k] + s * Aj[k];
          const float t1 = -s * Ai[k] + c * Aj[k];
          Ai[k] = t0; Aj[k] = t1;
        }
        lanes.sync();
        a = b = 0;
        for (int k = 0; k < m; k++) { a += (double)Ai[k] * (double)Ai[k]; b += (double)Aj[k] * (double)Aj[k]; }   // of the new t0, t1
        W[i] = a; W[j] = b;
        changed = true;
        float *Vi = Vt + i * n, *Vj = Vt + j * n;
        for (int k = lanes.first(); k < n; k += lanes.step()) {
          const float t0 = c * Vi[k] + s * Vj[k];
          const float t1 = -s * Vi[k] + c * Vj[k];
          Vi[k] = t0; Vj[k] = t1;
        }
      }
    if (!changed) break;
  }
  lanes.sync();
  for (int i = 0; i < n; i++) {
    double sd = 0;
    for (int k = 0; k < m; k++) { const float t = At[i * m + k]; sd += (double)t * (double)t; }
    W[i] = __builtin_sqrt(sd);
  }
  for (int i = 0; i < n - 1; i++) {
    int j = i;
    for (int k = i + 1; k < n; k++)
      if (W[j] < W[k]) j = k;
    if (i != j) {
      const double tw = W[i]; W[i] = W[j]; W[j] = tw;
      for (int k = 0; k < m; k++) { const float t = At[i * m + k]; At[i * m + k] = At[j * m + k]; At[j * m + k] = t; }
      for (int k = 0; k < n; k++) { const float t = Vt[i * n + k]; Vt[i * n + k] = Vt[j * n + k]; Vt[j * n + k] = t; }
    }
  }
  for (int i = 0; i < n; i++) w[i] = (float)W[i];
  uint64_t rng = 0x12345678;
  for (int i = 0; i < n1; i++) {
    float *Ai = At + i * m;
    double sd = i < n ? W[i] : 0;
    for (int ii = 0; ii < 100 && sd <= minval; ii++) {
      const float val0 = (float)(1. / m);
      for (int k = 0; k < m; k++) {
        rng = (uint64_t)(uint32_t)rng * 4164903690U + (uint32_t)(rng >> 32);
        Ai[k] = ((uint32_t)rng & 256) != 0 ? val0 : -val0;
      }
      for (int iter = 0; iter < 2; iter++)
        for (int j = 0; j < i; j++) {
          const float *Aj = At + j * m;
          sd = 0;
          for (int k = 0; k < m; k++) sd += (double)(Ai[k] * Aj[k]);   // a float product added to the double
          float asum = 0;
          for (int k = 0; k < m; k++) {
            const float t = (float)((double)Ai[k] - sd * (double)Aj[k]);
            Ai[k] = t;
            asum += __builtin_fabsf(t);
          }
          asum = (double)asum > eps * 100 ? 1 / asum : 0;
          for (int k = 0; k < m; k++) Ai[k] *= asum;
        }
      sd = 0;
      for (int k = 0; k < m; k++) { const float t = Ai[k]; sd += (double)t * (double)t; }
      sd = __builtin_sqrt(sd);
    }
    const float s = (float)(sd > minval ? 1 / sd : 0.);
    for (int k = 0; k < m; k++) Ai[k] *= s;
  }
}

// cv::SVD::compute of a 3 x 3 matrix in full (:303, :592, :916): u, w, vt; ws as below
template <class Lanes>
ORB_REF void tv_svd33(const float *A, float *ws, double *W, float *u, float *w3, float *vt, const Lanes &lanes) {
  float *At = ws, *Vt = ws + 9, *w = ws + 18;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) At[3 * i + k] = A[3 * k + i];
  tv_jacobi_svd(At, W, Vt, w, 3, 3, 3, lanes);
#pragma unroll
  for (int i = 0; i < 3; i++) {
    w3[i] = w[i];
#pragma unroll
    for (int k = 0; k < 3; k++) { u[3 * i + k] = At[3 * k + i]; vt[3 * i + k] = Vt[3 * i + k]; }
  }
}

// ---- Normalize (:753-799) ----------------------------------------------------------------------------------------------------------
// Over EVERY keypoint of a frame: sequential float sums in index order; pn [n][2], T [9]
ORB_REF void tv_normalize(const orbx_keypoint_t *keys, int n, float *pn, float *T) {
  float meanX = 0, meanY = 0;
  for (int i = 0; i < n; i++) { meanX += keys[i].x; meanY += keys[i].y; }
  meanX = meanX / n; meanY = meanY / n;
  float meanDevX = 0, meanDevY = 0;
  for (int i = 0; i < n; i++) {
    pn[2 * i] = keys[i].x - meanX; pn[2 * i + 1] = keys[i].y - meanY;
    meanDevX += __builtin_fabsf(pn[2 * i]); meanDevY += __builtin_fabsf(pn[2 * i + 1]);
  }
  meanDevX = meanDevX / n; meanDevY = meanDevY / n;
  const float sX = (float)(1.0 / (double)meanDevX), sY = (float)(1.0 / (double)meanDevY);
  for (int i = 0; i < n; i++) { pn[2 * i] = pn[2 * i] * sX; pn[2 * i + 1] = pn[2 * i + 1] * sY; }
  T[0] = sX; T[1] = 0.f; T[2] = -meanX * sX; T[3] = 0.f; T[4] = sY; T[5] = -meanY * sY; T[6] = 0.f; T[7] = 0.f; T[8] = 1.f;
}

// ---- ComputeH21 / ComputeF21 (:231-308) with the denormalisation of FindHomography / FindFundamental (:164-166, :215-217) -----------
// q [8][4]: the set's normalised pairs (u1, v1, u2, v2).  ws: TV_WS_FLOATS floats, W: TV_WS_DOUBLES doubles.
template <class Lanes>
ORB_REF void tv_homography(const float *q, const float *T1, const float *T2inv, float *ws, double *W, float *H21, float *H12, const Lanes &lanes) {
  float *At = ws, *Vt = ws + 144, *w = ws + 225;   // At = A.t(): 9 rows of 16
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const float u1 = q[4 * i], v1 = q[4 * i + 1], u2 = q[4 * i + 2], v2 = q[4 * i + 3];
    const float r0[9] = {0.f, 0.f, 0.f, -u1, -v1, -1.f, v2 * u1, v2 * v1, v2};
    const float r1[9] = {u1, v1, 1.f, 0.f, 0.f, 0.f, -u2 * u1, -u2 * v1, -u2};
#pragma unroll
    for (int c = 0; c < 9; c++) { At[16 * c + 2 * i] = r0[c]; At[16 * c + 2 * i + 1] = r1[c]; }
  }
  tv_jacobi_svd(At, W, Vt, w, 16, 9, 0, lanes);   // u is not read: vt.row(8) is row 8 of Vt
  float Hn[9], t[9];
#pragma unroll
  for (int k = 0; k < 9; k++) Hn[k] = Vt[72 + k];
  tv_mul33(T2inv, Hn, 1.0, t);
  tv_mul33(t, T1, 1.0, H21);
  tv_inv33(H21, H12);
}
template <class Lanes>
ORB_REF void tv_fundamental(const float *q, const float *T1, const float *T2t, float *ws, double *W, float *F21, const Lanes &lanes) {
  float *At = ws, *Vt = ws + 144, *w = ws + 225;   // 8 x 9 is wider than tall: At = A, its ninth row the completed vector = vt.row(8)
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const float u1 = q[4 * i], v1 = q[4 * i + 1], u2 = q[4 * i + 2], v2 = q[4 * i + 3];
    const float r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.f};
#pragma unroll
    for (int c = 0; c < 9; c++) At[9 * i + c] = r[c];
  }
  for (int c = 0; c < 9; c++) At[72 + c] = 0.f;
  tv_jacobi_svd(At, W, Vt, w, 9, 8, 9, lanes);
  float Fpre[9], u[9], w3[3], vt[9], t[9], Fn[9];
#pragma unroll
  for (int k = 0; k < 9; k++) Fpre[k] = At[72 + k];
  lanes.sync();   // the ninth row is read, then the workspace is built anew
  tv_svd33(Fpre, ws, W, u, w3, vt, lanes);
  const float D[9] = {w3[0], 0.f, 0.f, 0.f, w3[1], 0.f, 0.f, 0.f, 0.f};   // w.at<float>(2) = 0 (:305)
  tv_mul33(u, D, 1.0, t);
  tv_mul33(t, vt, 1.0, Fn);
  tv_mul33(T2t, Fn, 1.0, t);
  tv_mul33(t, T1, 1.0, F21);
}

// ---- CheckHomography / CheckFundamental (:310-473) for one match ---------------------------------------------------------------------
// The two terms a match adds to the score, first image then second, and whether each is added (`chiSquare > th` false, so a NaN
// chiSquare adds a NaN).  The match is an inlier when both are added.  invSigmaSquare = tv_inv_sigma_square(sigma).
struct TvTerms { float t1, t2; bool in1, in2; };
ORB_REF float tv_inv_sigma_square(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }
ORB_REF TvTerms tv_check_homography(const float *H21, const float *H12, float u1, float v1, float u2, float v2, float invSigmaSquare) {
  const float th = 5.991f;
  TvTerms r;
  const float w2in1inv = (float)(1.0 / (double)(H12[6] * u2 + H12[7] * v2 + H12[8]));
  const float u2in1 = (H12[0] * u2 + H12[1] * v2 + H12[2]) * w2in1inv;
  const float v2in1 = (H12[3] * u2 + H12[4] * v2 + H12[5]) * w2in1inv;
  const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
  const float chiSquare1 = squareDist1 * invSigmaSquare;
  r.in1 = !(chiSquare1 > th); r.t1 = th - chiSquare1;
  const float w1in2inv = (float)(1.0 / (double)(H21[6] * u1 + H21[7] * v1 + H21[8]));
  const float u1in2 = (H21[0] * u1 + H21[1] * v1 + H21[2]) * w1in2inv;
  const float v1in2 = (H21[3] * u1 + H21[4] * v1 + H21[5]) * w1in2inv;
  const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
  const float chiSquare2 = squareDist2 * invSigmaSquare;
  r.in2 = !(chiSquare2 > th); r.t2 = th - chiSquare2;
  return r;
}
ORB_REF TvTerms tv_check_fundamental(const float *F, float u1, float v1, float u2, float v2, float invSigmaSquare) {
  const float th = 3.841f, thScore = 5.991f;
  TvTerms r;
  const float a2 = F[0] * u1 + F[1] * v1 + F[2];
  const float b2 = F[3] * u1 + F[4] * v1 + F[5];
  const float c2 = F[6] * u1 + F[7] * v1 + F[8];
  const float num2 = a2 * u2 + b2 * v2 + c2;
  const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
  const float chiSquare1 = squareDist1 * invSigmaSquare;
  r.in1 = !(chiSquare1 > th); r.t1 = thScore - chiSquare1;
  const float a1 = F[0] * u2 + F[3] * v2 + F[6];
  const float b1 = F[1] * u2 + F[4] * v2 + F[7];
  const float c1 = F[2] * u2 + F[5] * v2 + F[8];
  const float num1 = a1 * u1 + b1 * v1 + c1;
  const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
  const float chiSquare2 = squareDist2 * invSigmaSquare;
  r.in2 = !(chiSquare2 > th); r.t2 = thScore - chiSquare2;
  return r;
}
ORB_REF TvTerms tv_check_model(int model, const float *M21, const float *M12, float u1, float v1, float u2, float v2, float invSigmaSquare) {
  return model == 0 ? tv_check_homography(M21, M12, u1, v1, u2, v2, invSigmaSquare) : tv_check_fundamental(M21, u1, v1, u2, v2, invSigmaSquare);
}

// ---- the motion hypotheses: DecomposeE (:913-933) behind E21 = K.t()*F21*K (:484), and ReconstructH's eight (:588-690) ---------------
// T [nhyp][12]: [R | t] with row stride 4, the P2 of CheckRT in front of its product with K.  ws / W as above.
ORB_REF void tv_store_hypothesis(const float *R, const float *t, float sign_t, float *T) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) T[4 * i + j] = R[3 * i + j];
    T[4 * i + 3] = sign_t * t[i];   // t2 = -t (:492): a sign flip
  }
}
ORB_REF int tv_hypotheses_F(const float *F21, const float *K, float *ws, double *W, float *T) {
  float KtF[9], E[9], u[9], w3[3], vt[9], t[3], tu[3], uW[9], R1[9], R2[9];
  tv_mul33_tA(K, F21, 3, 1.0, KtF);
  tv_mul33(KtF, K, 1.0, E);
  tv_svd33(E, ws, W, u, w3, vt, TvSolo());
#pragma unroll
  for (int i = 0; i < 3; i++) t[i] = u[3 * i + 2];
  tv_unit3(t, tu);
  const float Wm[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
  tv_mul33(u, Wm, 1.0, uW);
  tv_mul33(uW, vt, 1.0, R1);
  if (tv_det33(R1) < 0)
#pragma unroll
    for (int k = 0; k < 9; k++) R1[k] = -R1[k];
  tv_mul33_Bt(u, Wm, uW);
  tv_mul33(uW, vt, 1.0, R2);
  if (tv_det33(R2) < 0)
#pragma unroll
    for (int k = 0; k < 9; k++) R2[k] = -R2[k];
  tv_store_hypothesis(R1, tu, 1.f, T);        // (R1, t1) :499
  tv_store_hypothesis(R2, tu, 1.f, T + 12);   // (R2, t1)
  tv_store_hypothesis(R1, tu, -1.f, T + 24);  // (R1, t2)
  tv_store_hypothesis(R2, tu, -1.f, T + 36);  // (R2, t2)
  return 4;
}
// 0 when d1/d2 < 1.00001 || d2/d3 < 1.00001 (:601), else 8
ORB_REF int tv_hypotheses_H(const float *H21, const float *K, float *ws, double *W, float *T) {
  float invK[9], tmp[9], A[9], U[9], w3[3], Vt[9];
  tv_inv33(K, invK);
  tv_mul33(invK, H21, 1.0, tmp);
  tv_mul33(tmp, K, 1.0, A);
  tv_svd33(A, ws, W, U, w3, Vt, TvSolo());
  const float s = (float)(tv_det33(U) * tv_det33(Vt));
  const float d1 = w3[0], d2 = w3[1], d3 = w3[2];
  if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return 0;
  const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
  const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
  const float x1[4] = {aux1, aux1, -aux1, -aux1};
  const float x3[4] = {aux3, -aux3, aux3, -aux3};
  const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
  const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
  const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
  const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
  const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
  const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
  for (int h = 0; h < 8; h++) {
    const int i = h & 3;
    float Rp[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, tp[3], R[9], t[3], tu[3];
    float scale;
    if (h < 4) {   // d' = d2 (:623-652)
      Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[6] = stheta[i]; Rp[8] = ctheta;
      tp[0] = x1[i]; tp[1] = 0.f; tp[2] = -x3[i];
      scale = d1 - d3;
    } else {       // d' = -d2 (:660-690)
      Rp[0] = cphi; Rp[2] = sphi[i]; Rp[4] = -1.f; Rp[6] = sphi[i]; Rp[8] = -cphi;
      tp[0] = x1[i]; tp[1] = 0.f; tp[2] = x3[i];
      scale = d1 + d3;
    }
    tv_mul33(U, Rp, (double)s, tmp);   // s*U*Rp: one gemm with alpha = s
    tv_mul33(tmp, Vt, 1.0, R);
    for (int k = 0; k < 3; k++) tp[k] = (float)((double)tp[k] * (double)scale);   // tp *= d1 -+ d3
    tv_mul31(U, tp, t);
    tv_unit3(t, tu);
    tv_store_hypothesis(R, tu, 1.f, T + 12 * h);
  }
  return 8;
}

// ---- CheckRT (:802-911) ------------------------------------------------------------------------------------------------------------
// What the function forms once per hypothesis: P1 = K[I | 0], P2 = K*[R | t] (3 x 4, the small-matrix path), O2 = -R.t()*t
struct TvCamera { float P1[12], P2[12], T[12], O2[3], fx, fy, cx, cy, th2; };
ORB_REF void tv_camera(const float *K, const float *T, float sigma, TvCamera &C) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      C.P1[4 * i + j] = j < 3 ? K[3 * i + j] : 0.f;
      C.T[4 * i + j] = T[4 * i + j];
      float s = K[3 * i] * T[j];
      s = s + K[3 * i + 1] * T[4 + j];
      s = s + K[3 * i + 2] * T[8 + j];
      C.P2[4 * i + j] = (float)((double)s * 1.0 + 0.0);
    }
  }
  camera_centre(T, C.O2);
  C.fx = K[0]; C.fy = K[4]; C.cx = K[2]; C.cy = K[5];
  C.th2 = (float)(4.0 * (double)(sigma * sigma));   // 4.0*mSigma2 (:499), mSigma2 = sigma*sigma a float (:35)
}
// Triangulate (:738-751): rows `pt*P.row(2) - P.row(i)`, the 4 x 4 Jacobi, vt.row(3)[0..2] / vt.row(3)[3]
ORB_REF void tv_triangulate(const TvCamera &C, float u1, float v1, float u2, float v2, float *x3D) {
  float At[4][4], v[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    At[k][0] = u1 * C.P1[8 + k] - C.P1[k];
    At[k][1] = v1 * C.P1[8 + k] - C.P1[4 + k];
    At[k][2] = u2 * C.P2[8 + k] - C.P2[k];
    At[k][3] = v2 * C.P2[8 + k] - C.P2[4 + k];
  }
  jacobi_svd4_last_row(At, v, nullptr);
  const double inv = 1.0 / (double)v[3];
#pragma unroll
  for (int k = 0; k < 3; k++) x3D[k] = (float)((double)v[k] * inv);
}
// The body of the loop for one inlier match: the status, p3dC1 and cosParallax (both meaningful for TV_GOOD / TV_LOW_PARALLAX)
ORB_REF int tv_check_rt(const TvCamera &C, float u1, float v1, float u2, float v2, float *p, float *cosParallax) {
  tv_triangulate(C, u1, v1, u2, v2, p);
  if (!__builtin_isfinite(p[0]) || !__builtin_isfinite(p[1]) || !__builtin_isfinite(p[2])) return TV_NONFINITE;
  const float normal1[3] = {p[0] - 0.f, p[1] - 0.f, p[2] - 0.f};   // p3dC1 - O1, O1 = zeros
  const float dist1 = norm3(normal1);
  const float normal2[3] = {p[0] - C.O2[0], p[1] - C.O2[1], p[2] - C.O2[2]};
  const float dist2 = norm3(normal2);
  const float cp = (float)(dot3_double(normal1, normal2) / (double)(dist1 * dist2));
  *cosParallax = cp;
  if (p[2] <= 0 && (double)cp < 0.99998) return TV_BEHIND1;
  float p2[3];
  const float t[3] = {C.T[3], C.T[7], C.T[11]};
  mat3_mul_add(C.T, p, t, p2);   // R*p3dC1 + t (:865)
  if (p2[2] <= 0 && (double)cp < 0.99998) return TV_BEHIND2;
  const float invZ1 = (float)(1.0 / (double)p[2]);
  const float im1x = C.fx * p[0] * invZ1 + C.cx, im1y = C.fy * p[1] * invZ1 + C.cy;
  const float squareError1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1);
  if (squareError1 > C.th2) return TV_REPROJ1;
  const float invZ2 = (float)(1.0 / (double)p2[2]);
  const float im2x = C.fx * p2[0] * invZ2 + C.cx, im2y = C.fy * p2[1] * invZ2 + C.cy;
  const float squareError2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2);
  if (squareError2 > C.th2) return TV_REPROJ2;
  return (double)cp < 0.99998 ? TV_GOOD : TV_LOW_PARALLAX;
}
// parallax = acos(vCosParallax[idx])*180/CV_PI (:905): acos is the caller's (acosf on the host); the product a float, the quotient a double
ORB_REF float tv_parallax_degrees(float acos_value) { return (float)((double)(acos_value * 180.f) / 3.1415926535897932384626433832795); }

// ---- the decisions of Reconstruct (:111-126), ReconstructF (:504-574) and ReconstructH (:693-735) -----------------------------------
// N = the winning model's inlier count.  Returns the chosen hypothesis or -1.
ORB_REF int tv_select_F(const int *nGood, const float *parallax, int N) {
  int maxGood = nGood[0];
  for (int i = 1; i < 4; i++) maxGood = nGood[i] > maxGood ? nGood[i] : maxGood;
  const int n09 = (int)(0.9 * N);
  const int nMinGood = n09 > 50 ? n09 : 50;
  int nsimilar = 0;
  for (int i = 0; i < 4; i++)
    if ((double)nGood[i] > 0.7 * maxGood) nsimilar++;
  if (maxGood < nMinGood || nsimilar > 1) return -1;
  for (int i = 0; i < 4; i++)
    if (maxGood == nGood[i]) return parallax[i] > 1.0f ? i : -1;   // an else-if chain: the first equal count decides (:528-572)
  return -1;
}
ORB_REF int tv_select_H(const int *nGood, const float *parallax, int N) {
  int bestGood = 0, secondBestGood = 0, best = -1;
  float bestParallax = -1;
  for (int i = 0; i < 8; i++) {
    if (nGood[i] > bestGood) { secondBestGood = bestGood; bestGood = nGood[i]; best = i; bestParallax = parallax[i]; }
    else if (nGood[i] > secondBestGood) secondBestGood = nGood[i];
  }
  if ((double)secondBestGood < 0.75 * bestGood && bestParallax >= 1.0f && bestGood > 50 && (double)bestGood > 0.9 * N) return best;
  return -1;
}

#undef ORB_REF
