/*
 * Stand-in for <opencv2/core/core.hpp> (TEST INFRASTRUCTURE): what the reference's CameraModels/Pinhole.cpp, KannalaBrandt8.cpp and
 * ORBmatcher.cc, and the headers they include, use of OpenCV 3.4.x - and nothing else.  Written from scratch from OpenCV's published algorithms;
 * an independent, general (any small m x n) restatement that shares no code with the product, the oracle or the test models.
 *
 *   Mat            CV_32F for the algebra, CV_8U for descriptor rows (row, ptr<int32_t>, clone, release - no algebra); two dimensions, shared
 *                  storage; row / col / rowRange / colRange are views into it.
 *   MatExpr        the lazy expressions of the two files, folded as OpenCV's MatExpr folds them (DESIGN.md section 2 has the table):
 *                    A*B, -A*B, s*A*B, A*B + C      one gemm: D = alpha*A*B + beta*C
 *                    s*A - B                        one scaled addition in float: product rounded, then the difference
 *                    A / s                          (float)((double)v * (1.0 / (double)s))
 *                    -A.t()*B                       the transposition materialised, then one gemm with alpha = -1 (the matcher)
 *                    A - B                          one float difference per entry (the matcher)
 *                    A.t(), A.inv(), A.t().inv()    materialised when assigned or used as a gemm operand
 *                  Every other expression shape asserts.
 *   gemm           inner length 2..4 (equal to one side of the result), no transposed operand: OpenCV's small-matrix path, the sum
 *                  of products in float, then (float)((double)sum*alpha + (double)c*beta).  Anything else asserts.
 *   dot, norm      accumulated in double (CV_32F).
 *   inv            3 x 3 only: the closed cofactor form evaluated in double.
 *   SVD::compute   OpenCV's own one-sided Jacobi for float (JacobiSVDImpl_<float>), in full: u, w, all of vt, rows sorted.  An OpenCV
 *                  built with LAPACK gives other low bits.
 *   fisheye::undistortPoints  declared because KannalaBrandt8::ReconstructWithTwoViews names it; aborts.
 *   FileStorage, BFMatcher, InputArray ...  declared, without bodies, at the end: named by the SLAM headers ORBmatcher.cc includes.
 *                  (oracle/ref_voc_driver.cc gives the FileStorage family aborting bodies: DBoW2's template names them in virtual members.)
 *
 * This header does not include <math.h>: whether an unqualified cos(float) inside a namespace is the float or the double function is
 * decided by opencv2/opencv.hpp (see there).  Compile without -DNDEBUG: what is not provided asserts.
 */
#ifndef REF_CAM_SHIM_CORE_HPP
#define REF_CAM_SHIM_CORE_HPP

#include <assert.h>
#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#define CV_PI 3.1415926535897932384626433832795
#define CV_8U 0
#define CV_8UC1 0
#define CV_32F 5
#define CV_64F 6

namespace cv {

template <typename T>
struct Point_ {
  T x, y;
  Point_() : x(0), y(0) {}
  Point_(T _x, T _y) : x(_x), y(_y) {}
};
typedef Point_<float> Point2f;
typedef Point_<int> Point2i;
typedef Point_<int> Point;
typedef Point_<double> Point2d;

template <typename T>
struct Point3_ {
  T x, y, z;
  Point3_() : x(0), y(0), z(0) {}
  Point3_(T _x, T _y, T _z) : x(_x), y(_y), z(_z) {}
};
typedef Point3_<float> Point3f;
typedef Point3_<double> Point3d;
typedef unsigned char uchar;
template <typename T>
struct Size_ {
  T width, height;
  Size_() : width(0), height(0) {}
  Size_(T w, T h) : width(w), height(h) {}
};
typedef Size_<int> Size;

struct KeyPoint {
  Point2f pt;
  float size, angle, response;
  int octave, class_id;
  KeyPoint() : size(0), angle(-1), response(0), octave(0), class_id(-1) {}
};

namespace shim {
/* How often the calling text reached each primitive: lets a driver tell which way a member function left without touching its
   text.  Reset by the driver; plain counters, not thread-safe. */
struct Trace { int gemm, dot, svd, ptr; };
inline Trace &trace() { static Trace t = {0, 0, 0, 0}; return t; }
}  // namespace shim

class Mat;
template <typename T> class Mat_;
template <typename T> class MatCommaInitializer_;

/* A lazy expression.  a, b, c hold the operands (sharing their storage), alpha / beta the scalars. */
struct MatExpr {
  enum Op { T, INV, SCALE, GEMM, AXMB, DIV, SUB };
  Op op;
  std::shared_ptr<Mat> a, b, c;
  double alpha, beta;
  MatExpr(Op o, const Mat &A, double al = 1.0);
  MatExpr inv() const;
  operator Mat() const;
};

class Mat {
 public:
  int rows, cols;

  Mat() : rows(0), cols(0), type_(CV_32F), step_(0), off_(0) {}
  Mat(int r, int c, int type) : rows(0), cols(0), type_(CV_32F), step_(0), off_(0) { create(r, c, type); }
  template <typename T> Mat(const MatCommaInitializer_<T> &ci);

  void create(int r, int c, int type) {
    assert((type == CV_32F || type == CV_8U) && r >= 0 && c >= 0);
    if (rows == r && cols == c && type_ == type && (buf_ || bytes_)) return;
    rows = r; cols = c; step_ = (size_t)c; off_ = 0; type_ = type;
    buf_.reset(); bytes_.reset();
    if (type == CV_32F) buf_ = std::shared_ptr<float>(new float[(size_t)r * (size_t)c + 1](), std::default_delete<float[]>());
    /* descriptor rows are read as 32-bit words (ptr<int32_t>): new[] storage is aligned for them when every row is a multiple of 4 */
    else bytes_ = std::shared_ptr<uchar>(new uchar[(size_t)r * (size_t)c + 4](), std::default_delete<uchar[]>());
  }
  void release() { rows = 0; cols = 0; step_ = 0; off_ = 0; buf_.reset(); bytes_.reset(); }
  int type() const { return type_; }
  bool empty() const { return rows == 0 || cols == 0 || (!buf_ && !bytes_); }
  bool isContinuous() const { return rows <= 1 || step_ == (size_t)cols; }
  size_t elemSize() const { return type_ == CV_32F ? sizeof(float) : 1; }
  size_t total() const { return (size_t)rows * (size_t)cols; }
  int channels() const { return 1; }
  Size size() const { return Size(cols, rows); }

  /* ptr<float> of a CV_32F matrix; ptr<uchar> / ptr<int32_t> (a row of descriptor words) of a CV_8U one */
  template <typename T> T *ptr(int y = 0) { shim::trace().ptr++; assert(y >= 0 && y < rows); return row_((T *)0, y); }
  template <typename T> const T *ptr(int y = 0) const { shim::trace().ptr++; assert(y >= 0 && y < rows); return const_cast<Mat *>(this)->row_((T *)0, y); }
  uchar *ptr(int y = 0) { return ptr<uchar>(y); }
  const uchar *ptr(int y = 0) const { return ptr<uchar>(y); }
  template <typename T> T &at(int y, int x) { assert(y >= 0 && y < rows && x >= 0 && x < cols); return row_((T *)0, y)[x]; }
  template <typename T> const T &at(int y, int x) const { return const_cast<Mat *>(this)->at<T>(y, x); }
  /* the one-index form: a continuous matrix or a single row is indexed in storage order, a single column by rows */
  template <typename T> T &at(int i) {
    if (isContinuous() || rows == 1) { assert(i >= 0 && i < rows * cols); return at<T>(cols ? i / cols : 0, cols ? i % cols : 0); }
    assert(cols == 1);
    return at<T>(i, 0);
  }
  template <typename T> const T &at(int i) const { return const_cast<Mat *>(this)->at<T>(i); }

  Mat row(int y) const { return rowRange(y, y + 1); }
  Mat col(int x) const { return colRange(x, x + 1); }
  Mat rowRange(int y0, int y1) const {
    assert(0 <= y0 && y0 <= y1 && y1 <= rows);
    Mat m(*this);
    m.off_ = off_ + (size_t)y0 * step_;
    m.rows = y1 - y0;
    return m;
  }
  Mat colRange(int x0, int x1) const {
    assert(0 <= x0 && x0 <= x1 && x1 <= cols);
    Mat m(*this);
    m.off_ = off_ + (size_t)x0;
    m.cols = x1 - x0;
    return m;
  }
  Mat clone() const {
    if (empty()) return Mat();
    Mat m(rows, cols, type_);
    for (int y = 0; y < rows; y++)
      for (int x = 0; x < cols; x++) {
        if (type_ == CV_32F) m.at<float>(y, x) = at<float>(y, x);
        else m.at<uchar>(y, x) = at<uchar>(y, x);
      }
    return m;
  }
  static Mat zeros(int r, int c, int type) { return Mat(r, c, type); }
  static Mat zeros(Size s, int type) { return Mat(s.height, s.width, type); }
  /* written into the existing storage where the shape already fits (A.row(i) = ...), into new storage otherwise */
  Mat &operator=(const MatExpr &e);

  MatExpr t() const { return MatExpr(MatExpr::T, *this); }
  MatExpr inv() const { return MatExpr(MatExpr::INV, *this); }

  double dot(const Mat &m) const {
    assert(rows == m.rows && cols == m.cols);
    shim::trace().dot++;
    double s = 0;
    for (int y = 0; y < rows; y++)
      for (int x = 0; x < cols; x++) s += (double)at<float>(y, x) * (double)m.at<float>(y, x);
    return s;
  }
  static Mat eye(int r, int c, int type) {
    Mat m(r, c, type);
    for (int i = 0; i < std::min(r, c); i++) m.at<float>(i, i) = 1.f;
    return m;
  }

 private:
  float *row_(float *, int y) { assert(type_ == CV_32F && buf_); return buf_.get() + off_ + (size_t)y * step_; }
  uchar *row_(uchar *, int y) { assert(type_ == CV_8U && bytes_); return bytes_.get() + off_ + (size_t)y * step_; }
  int *row_(int *, int y) { assert(cols % 4 == 0 && (off_ + (size_t)y * step_) % 4 == 0); return (int *)row_((uchar *)0, y); }
  int type_;
  std::shared_ptr<float> buf_;
  std::shared_ptr<uchar> bytes_;
  size_t step_, off_; /* in elements */
};

template <typename T>
class Mat_ : public Mat {
 public:
  Mat_() {}
  Mat_(int r, int c) : Mat(r, c, CV_32F) { float *only_float = (T *)0; (void)only_float; }
};

template <typename T>
class MatCommaInitializer_ {
 public:
  MatCommaInitializer_(const Mat_<T> &m) : m_(m), n_(0) {}
  template <typename T2> MatCommaInitializer_<T> &operator,(T2 v) {
    assert(n_ < m_.rows * m_.cols);
    m_.template at<T>(n_ / m_.cols, n_ % m_.cols) = (T)v;
    n_++;
    return *this;
  }
  operator Mat_<T>() const { assert(n_ == m_.rows * m_.cols); return m_; }
  const Mat_<T> &get() const { assert(n_ == m_.rows * m_.cols); return m_; }

 private:
  Mat_<T> m_;
  int n_;
};
template <typename T, typename T2>
inline MatCommaInitializer_<T> operator<<(const Mat_<T> &m, T2 v) {
  MatCommaInitializer_<T> ci(m);
  return (ci, v);
}
template <typename T> inline Mat::Mat(const MatCommaInitializer_<T> &ci) : rows(0), cols(0), type_(CV_32F), step_(0), off_(0) { *this = ci.get(); }

/* ---- evaluation ---------------------------------------------------------------------------------------------------------------- */
namespace shim {

inline Mat transposed(const Mat &a) {
  Mat m(a.cols, a.rows, CV_32F);
  for (int y = 0; y < a.rows; y++)
    for (int x = 0; x < a.cols; x++) m.at<float>(x, y) = a.at<float>(y, x);
  return m;
}

/* cv::invert, DECOMP_LU, of a 3 x 3 CV_32F matrix: the cofactors and the determinant in double, every entry rounded once.  A zero
   determinant gives the zero matrix. */
inline Mat inverted(const Mat &a) {
  assert(a.rows == 3 && a.cols == 3);
  double s[3][3];
  for (int y = 0; y < 3; y++)
    for (int x = 0; x < 3; x++) s[y][x] = (double)a.at<float>(y, x);
  Mat m(3, 3, CV_32F);
  double cof[3][3]; /* cof[y][x]: entry (y, x) of the adjugate */
  for (int y = 0; y < 3; y++)
    for (int x = 0; x < 3; x++) {
      const int r0 = (x + 1) % 3, r1 = (x + 2) % 3, c0 = (y + 1) % 3, c1 = (y + 2) % 3;
      cof[y][x] = s[r0][c0] * s[r1][c1] - s[r0][c1] * s[r1][c0];
    }
  /* the determinant along the first row; the cyclic indices above carry every cofactor's sign in the order of its two products */
  double d = s[0][0] * (s[1][1] * s[2][2] - s[1][2] * s[2][1]) - s[0][1] * (s[1][0] * s[2][2] - s[1][2] * s[2][0]) +
             s[0][2] * (s[1][0] * s[2][1] - s[1][1] * s[2][0]);
  if (d == 0.) return m;
  d = 1. / d;
  for (int y = 0; y < 3; y++)
    for (int x = 0; x < 3; x++) m.at<float>(y, x) = (float)(cof[y][x] * d);
  return m;
}

/* D = alpha*A*B + beta*C without transposition flags: the small-matrix path of cv::gemm */
inline Mat gemm(const Mat &a, const Mat &b, double alpha, const Mat *c, double beta) {
  const int len = a.cols, dh = a.rows, dw = b.cols;
  assert(b.rows == len);
  trace().gemm++;
  assert(2 <= len && len <= 4 && (len == dw || len == dh)); /* the generic, double-accumulating path is not provided */
  if (c) assert(c->rows == dh && c->cols == dw);
  Mat d(dh, dw, CV_32F);
  for (int i = 0; i < dh; i++)
    for (int j = 0; j < dw; j++) {
      float s = a.at<float>(i, 0) * b.at<float>(0, j);
      for (int k = 1; k < len; k++) s = s + a.at<float>(i, k) * b.at<float>(k, j);
      const double cv = c ? (double)c->at<float>(i, j) : 0.0;
      d.at<float>(i, j) = (float)((double)s * alpha + cv * (c ? beta : 0.0));
    }
  return d;
}

inline Mat eval(const MatExpr &e) {
  switch (e.op) {
    case MatExpr::T: return transposed(*e.a);
    case MatExpr::INV: return inverted(*e.a);
    case MatExpr::GEMM: return gemm(*e.a, *e.b, e.alpha, e.c.get(), e.beta);
    case MatExpr::AXMB: { /* addWeighted(a, alpha, b, -1, 0) for CV_32F: the scalar as a float, the product rounded, then the sum */
      const Mat &a = *e.a, &b = *e.b;
      assert(a.rows == b.rows && a.cols == b.cols);
      const float al = (float)e.alpha;
      Mat d(a.rows, a.cols, CV_32F);
      for (int y = 0; y < a.rows; y++)
        for (int x = 0; x < a.cols; x++) {
          const float p = a.at<float>(y, x) * al;
          d.at<float>(y, x) = p - b.at<float>(y, x);
        }
      return d;
    }
    case MatExpr::SUB: { /* subtract() of two CV_32F matrices: one float difference per entry */
      const Mat &a = *e.a, &b = *e.b;
      assert(a.rows == b.rows && a.cols == b.cols);
      Mat d(a.rows, a.cols, CV_32F);
      for (int y = 0; y < a.rows; y++)
        for (int x = 0; x < a.cols; x++) d.at<float>(y, x) = a.at<float>(y, x) - b.at<float>(y, x);
      return d;
    }
    case MatExpr::DIV: { /* convertTo with the scale 1/s */
      const Mat &a = *e.a;
      const double inv = 1.0 / e.alpha;
      Mat d(a.rows, a.cols, CV_32F);
      for (int y = 0; y < a.rows; y++)
        for (int x = 0; x < a.cols; x++) d.at<float>(y, x) = (float)((double)a.at<float>(y, x) * inv);
      return d;
    }
    default: break;
  }
  assert(!"ref_cam_shim: this expression shape is not provided (a scaled matrix on its own)");
  abort();
}

/* an operand of a product: a plain matrix, or an inverse / a finished product that has to exist first */
inline Mat operand(const MatExpr &e) {
  assert(e.op == MatExpr::INV || e.op == MatExpr::GEMM);
  return eval(e);
}

}  // namespace shim

inline MatExpr::MatExpr(Op o, const Mat &A, double al) : op(o), a(new Mat(A)), alpha(al), beta(0) {}
inline MatExpr::operator Mat() const { return shim::eval(*this); }
inline MatExpr MatExpr::inv() const {
  assert(op == T); /* K1.t().inv(): the transposed matrix is formed, then inverted */
  return MatExpr(INV, shim::transposed(*a));
}
inline Mat &Mat::operator=(const MatExpr &e) {
  Mat v = shim::eval(e);
  if (buf_ && type_ == CV_32F && rows == v.rows && cols == v.cols) {
    for (int y = 0; y < rows; y++)
      for (int x = 0; x < cols; x++) at<float>(y, x) = v.at<float>(y, x);
  } else {
    *this = v;
  }
  return *this;
}

inline MatExpr make_gemm(const Mat &a, const Mat &b, double alpha) {
  MatExpr e(MatExpr::GEMM, a, alpha);
  e.b.reset(new Mat(b));
  return e;
}
inline MatExpr operator-(const Mat &a) { return MatExpr(MatExpr::SCALE, a, -1.0); }
/* -A.t(): MatOp::negate materialises the transposition and scales it by -1, still lazily, so -A.t()*B is one gemm with alpha = -1
   and no transposition flag */
inline MatExpr operator-(const MatExpr &e) {
  assert(e.op == MatExpr::T);
  return MatExpr(MatExpr::SCALE, shim::transposed(*e.a), -1.0);
}
inline MatExpr operator-(const Mat &a, const Mat &b) {
  MatExpr r(MatExpr::SUB, a);
  r.b.reset(new Mat(b));
  return r;
}
inline MatExpr operator*(double s, const Mat &a) { return MatExpr(MatExpr::SCALE, a, s); }
inline MatExpr operator*(const Mat &a, const Mat &b) { return make_gemm(a, b, 1.0); }
inline MatExpr operator*(const MatExpr &e, const Mat &b) {
  if (e.op == MatExpr::SCALE) return make_gemm(*e.a, b, e.alpha);
  return make_gemm(shim::operand(e), b, 1.0);
}
inline MatExpr operator*(const MatExpr &e1, const MatExpr &e2) { return e1 * shim::operand(e2); }
inline MatExpr operator+(const MatExpr &e, const Mat &c) {
  assert(e.op == MatExpr::GEMM && !e.c);
  MatExpr r(e);
  r.c.reset(new Mat(c));
  r.beta = 1.0;
  return r;
}
inline MatExpr operator-(const MatExpr &e, const Mat &b) {
  assert(e.op == MatExpr::SCALE);
  MatExpr r(MatExpr::AXMB, *e.a, e.alpha);
  r.b.reset(new Mat(b));
  return r;
}
inline MatExpr operator/(const Mat &a, double s) { return MatExpr(MatExpr::DIV, a, s); }
/* Shapes no pinned text forms.  Without these two a lazy right operand would convert to a Mat silently and take the small-matrix path,
   which is not what OpenCV does with a transposition flag (A*B.t()) or a nested product: they assert instead. */
inline MatExpr operator*(const Mat &, const MatExpr &) {
  assert(!"ref_cam_shim: matrix * lazy expression is not provided");
  abort();
}
inline MatExpr operator*(double, const MatExpr &) {
  assert(!"ref_cam_shim: scalar * lazy expression is not provided");
  abort();
}

/* NORM_L2 of CV_32F: the sum of squares in double */
inline double norm(const Mat &a) {
  double s = 0;
  for (int y = 0; y < a.rows; y++)
    for (int x = 0; x < a.cols; x++) s += (double)a.at<float>(y, x) * (double)a.at<float>(y, x);
  return std::sqrt(s);
}

inline void hconcat(const Mat &a, const Mat &b, Mat &dst) {
  assert(a.rows == b.rows);
  Mat d(a.rows, a.cols + b.cols, CV_32F);
  for (int y = 0; y < a.rows; y++) {
    for (int x = 0; x < a.cols; x++) d.at<float>(y, x) = a.at<float>(y, x);
    for (int x = 0; x < b.cols; x++) d.at<float>(y, a.cols + x) = b.at<float>(y, x);
  }
  dst = d;
}

inline std::ostream &operator<<(std::ostream &os, const Mat &m) {
  os << "[";
  for (int y = 0; y < m.rows; y++) {
    for (int x = 0; x < m.cols; x++) os << (x ? ", " : "") << m.at<float>(y, x);
    os << (y + 1 < m.rows ? ";\n " : "");
  }
  return os << "]";
}

/* ---- cv::SVD ------------------------------------------------------------------------------------------------------------------- */
class SVD {
 public:
  enum { MODIFY_A = 1, NO_UV = 2, FULL_UV = 4 };

  /* w: min(m, n) x 1, descending; u: m x m; vt: n x n.  Only MODIFY_A | FULL_UV is provided. */
  static void compute(const Mat &src, Mat &w, Mat &u, Mat &vt, int flags) {
    assert(flags == (MODIFY_A | FULL_UV));
    shim::trace().svd++;
    int m = src.rows, n = src.cols;
    assert(m >= 1 && n >= 1);
    const bool at = m < n; /* the wider case works on the matrix itself instead of its transposition */
    if (at) std::swap(m, n);
    const int urows = m;
    std::vector<float> A((size_t)urows * m, 0.f), V((size_t)n * n, 0.f), W((size_t)n, 0.f);
    for (int i = 0; i < n; i++)
      for (int k = 0; k < m; k++) A[(size_t)i * m + k] = at ? src.at<float>(i, k) : src.at<float>(k, i);
    jacobi(A.data(), W.data(), V.data(), m, n, urows);
    w = fill(W.data(), n, 1, false);
    if (!at) { u = fill(A.data(), urows, m, true); vt = fill(V.data(), n, n, false); }
    else { u = fill(V.data(), n, n, true); vt = fill(A.data(), urows, m, false); }
  }

 private:
  static Mat fill(const float *p, int r, int c, bool transpose) {
    Mat m(transpose ? c : r, transpose ? r : c, CV_32F);
    for (int y = 0; y < r; y++)
      for (int x = 0; x < c; x++) (transpose ? m.at<float>(x, y) : m.at<float>(y, x)) = p[(size_t)y * c + x];
    return m;
  }
  static double hyp(double a, double b) {
    a = std::abs(a); b = std::abs(b);
    if (a > b) { b /= a; return a * std::sqrt(1 + b * b); }
    if (b > 0) { a /= b; return b * std::sqrt(1 + a * a); }
    return 0;
  }
  /* One-sided Jacobi on the n rows (length m) of At, rotations gathered in the n x n Vt; n1 >= n rows of At leave as left vectors. */
  static void jacobi(float *At, float *Wout, float *Vt, int m, int n, int n1) {
    const double minval = FLT_MIN, eps = (double)FLT_EPSILON * 2;
    std::vector<double> W((size_t)n);
    for (int i = 0; i < n; i++) {
      double sd = 0;
      for (int k = 0; k < m; k++) { const float t = At[(size_t)i * m + k]; sd += (double)t * t; }
      W[i] = sd;
      for (int k = 0; k < n; k++) Vt[(size_t)i * n + k] = 0;
      Vt[(size_t)i * n + i] = 1;
    }
    const int max_iter = std::max(m, 30);
    for (int iter = 0; iter < max_iter; iter++) {
      bool changed = false;
      for (int i = 0; i < n - 1; i++)
        for (int j = i + 1; j < n; j++) {
          float *Ai = At + (size_t)i * m, *Aj = At + (size_t)j * m;
          double a = W[i], p = 0, b = W[j];
          for (int k = 0; k < m; k++) p += (double)Ai[k] * Aj[k];
          if (std::abs(p) <= eps * std::sqrt(a * b)) continue;
          p *= 2;
          const double beta = a - b, gamma = hyp(p, beta);
          float c, s;
          if (beta < 0) {
            const double delta = (gamma - beta) * 0.5;
            s = (float)std::sqrt(delta / gamma);
            c = (float)(p / (gamma * s * 2));
          } else {
            c = (float)std::sqrt((gamma + beta) / (gamma * 2));
            s = (float)(p / (gamma * c * 2));
          }
          a = b = 0;
          for (int k = 0; k < m; k++) {
            const float t0 = c * Ai[k] + s * Aj[k];
            const float t1 = -s * Ai[k] + c * Aj[k];
            Ai[k] = t0; Aj[k] = t1;
            a += (double)t0 * t0; b += (double)t1 * t1;
          }
          W[i] = a; W[j] = b;
          changed = true;
          float *Vi = Vt + (size_t)i * n, *Vj = Vt + (size_t)j * n;
          for (int k = 0; k < n; k++) {
            const float t0 = c * Vi[k] + s * Vj[k];
            const float t1 = -s * Vi[k] + c * Vj[k];
            Vi[k] = t0; Vj[k] = t1;
          }
        }
      if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
      double sd = 0;
      for (int k = 0; k < m; k++) { const float t = At[(size_t)i * m + k]; sd += (double)t * t; }
      W[i] = std::sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) { /* selection sort, descending: the first of equal values stays */
      int j = i;
      for (int k = i + 1; k < n; k++)
        if (W[j] < W[k]) j = k;
      if (i != j) {
        std::swap(W[i], W[j]);
        for (int k = 0; k < m; k++) std::swap(At[(size_t)i * m + k], At[(size_t)j * m + k]);
        for (int k = 0; k < n; k++) std::swap(Vt[(size_t)i * n + k], Vt[(size_t)j * n + k]);
      }
    }
    for (int i = 0; i < n; i++) Wout[i] = (float)W[i];
    /* left vectors: the rows of At over their lengths; for a zero length (and the rows beyond n) a pseudo-random vector made
       orthogonal to the rows before it, as OpenCV does with its multiply-with-carry generator seeded 0x12345678 */
    uint64_t rng = 0x12345678;
    for (int i = 0; i < n1; i++) {
      double sd = i < n ? W[i] : 0;
      for (int ii = 0; ii < 100 && sd <= minval; ii++) {
        const float val0 = (float)(1. / m);
        for (int k = 0; k < m; k++) {
          rng = (uint64_t)(unsigned)rng * 4164903690U + (unsigned)(rng >> 32);
          At[(size_t)i * m + k] = ((unsigned)rng & 256) != 0 ? val0 : -val0;
        }
        for (int iter = 0; iter < 2; iter++)
          for (int j = 0; j < i; j++) {
            sd = 0;
            for (int k = 0; k < m; k++) sd += At[(size_t)i * m + k] * At[(size_t)j * m + k];
            float asum = 0;
            for (int k = 0; k < m; k++) {
              const float t = (float)(At[(size_t)i * m + k] - sd * At[(size_t)j * m + k]);
              At[(size_t)i * m + k] = t;
              asum += std::abs(t);
            }
            asum = asum > eps * 100 ? 1 / asum : 0;
            for (int k = 0; k < m; k++) At[(size_t)i * m + k] *= asum;
          }
        sd = 0;
        for (int k = 0; k < m; k++) { const float t = At[(size_t)i * m + k]; sd += (double)t * t; }
        sd = std::sqrt(sd);
      }
      const float s = (float)(sd > minval ? 1 / sd : 0.);
      for (int k = 0; k < m; k++) At[(size_t)i * m + k] *= s;
    }
  }
};

namespace fisheye {
/* named by KannalaBrandt8::ReconstructWithTwoViews, which no test reaches */
inline void undistortPoints(const std::vector<Point2f> &, std::vector<Point2f> &, const Mat &, const Mat &, const Mat &, const Mat &) {
  fprintf(stderr, "ref_cam_shim: cv::fisheye::undistortPoints is not provided\n");
  abort();
}
}  // namespace fisheye

/* ---- named by the SLAM headers the matcher includes (Frame.h, KeyFrame.h, Map.h, the in-tree DBoW2 headers), never called ------ */
typedef std::string String;
struct Rect { int x, y, width, height; Rect(int a, int b, int c, int d) : x(a), y(b), width(c), height(d) {} };
template <typename T, int M, int N> struct Matx { T val[M * N]; };
struct _InputArray { _InputArray(const Mat &m); };
struct _OutputArray { _OutputArray(Mat &m); };
typedef const _InputArray &InputArray;
typedef const _OutputArray &OutputArray;
struct DMatch { int queryIdx, trainIdx, imgIdx; float distance; };
enum { NORM_HAMMING = 6 };
struct BFMatcher {
  BFMatcher(int normType = 4, bool crossCheck = false);
  void knnMatch(const Mat &, const Mat &, std::vector<std::vector<DMatch> > &, int) const;
};
struct FileNode;
struct FileNodeIterator { FileNodeIterator &operator++(); FileNode operator*() const; bool operator!=(const FileNodeIterator &) const; };
struct FileNode {
  enum { SEQ = 5, MAP = 6 };
  FileNode operator[](const char *) const; FileNode operator[](const std::string &) const; FileNode operator[](int) const;
  operator int() const; operator float() const; operator double() const; operator std::string() const;
  bool empty() const; size_t size() const; int type() const; bool isSeq() const;
  FileNodeIterator begin() const; FileNodeIterator end() const;
};
struct FileStorage {
  enum { READ = 0, WRITE = 1 };
  FileStorage(); FileStorage(const std::string &, int);
  bool isOpened() const; void release();
  FileNode operator[](const char *) const; FileNode operator[](const std::string &) const;
};
template <typename T> FileStorage &operator<<(FileStorage &, const T &);
template <typename T> void operator>>(const FileNode &, T &);

}  // namespace cv

#endif
