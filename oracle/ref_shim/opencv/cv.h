/*
 * Stand-in container header -- TEST INFRASTRUCTURE, not OpenCV.
 *
 * `make -C oracle ref` compiles the reference's own ORBextractor.cc, unmodified, against this header instead of OpenCV.  It
 * provides exactly what that one file names: the containers (Mat with reference-counted storage and ROI views, KeyPoint, Point_,
 * Size, Rect, the array proxies) written here from their documented behaviour, and the primitives (FAST, GaussianBlur, resize,
 * copyMakeBorder, fastAtan2, cvRound / cvFloor / cvCeil) FORWARDED to the oracle's orc_* restatements.  So a build against this
 * header pins the extractor's own text - control flow, geometry, octree, orientation, descriptor, ordering - and says nothing
 * about the primitives: those are the oracle's on both sides of every comparison.
 *
 * An argument this header does not implement (another kernel size, sigma, border type, interpolation, element type) is asserted,
 * never ignored; keep NDEBUG off.
 */
#ifndef ORB_REF_SHIM_OPENCV_CV_H
#define ORB_REF_SHIM_OPENCV_CV_H

#include <stdint.h>
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <memory>
#include <vector>

#include "orb_oracle.h"

typedef unsigned char uchar;

#define CV_8U 0
#define CV_8UC1 0
#define CV_PI 3.1415926535897932384626433832795

inline int cvRound(double v) { return orc_cvRound(v); }
inline int cvRound(float v) { return orc_cvRound((double)v); }  /* a float is exact in double: the same half-even result */
inline int cvRound(int v) { return v; }
inline int cvFloor(double v) { return (int)std::floor(v); }
inline int cvCeil(double v) { return (int)std::ceil(v); }

namespace cv {

enum { BORDER_REFLECT_101 = 4, BORDER_ISOLATED = 16 };
enum { INTER_LINEAR = 1 };

template <typename T> struct Point_ {
  T x, y;
  Point_() : x(0), y(0) {}
  Point_(T x_, T y_) : x(x_), y(y_) {}
  Point_ &operator*=(float s) { x = (T)(x * s); y = (T)(y * s); return *this; }
};
typedef Point_<int> Point2i;
typedef Point_<int> Point;
typedef Point_<float> Point2f;

struct Size {
  int width, height;
  Size() : width(0), height(0) {}
  Size(int w, int h) : width(w), height(h) {}
};

struct Rect {
  int x, y, width, height;
  Rect() : x(0), y(0), width(0), height(0) {}
  Rect(int x_, int y_, int w, int h) : x(x_), y(y_), width(w), height(h) {}
};

struct KeyPoint {
  Point2f pt;
  float size, angle, response;
  int octave, class_id;
  KeyPoint() : pt(0, 0), size(0), angle(-1), response(0), octave(0), class_id(-1) {}
  KeyPoint(float x, float y, float size_, float angle_ = -1, float response_ = 0, int octave_ = 0, int class_id_ = -1)
      : pt(x, y), size(size_), angle(angle_), response(response_), octave(octave_), class_id(class_id_) {}
};

class _OutputArray;

/* 8-bit single-channel matrix.  Copies share the buffer; row / col ranges and operator()(Rect) are views into it. */
class Mat {
 public:
  int rows, cols;
  size_t step; /* bytes per row of the underlying buffer */
  uchar *data;

  Mat() : rows(0), cols(0), step(0), data(0), sub_(false) {}
  Mat(int r, int c, int type) : rows(0), cols(0), step(0), data(0), sub_(false) { create(r, c, type); }
  Mat(Size s, int type) : rows(0), cols(0), step(0), data(0), sub_(false) { create(s.height, s.width, type); }

  void create(int r, int c, int type) {
    assert(type == CV_8UC1 && r >= 0 && c >= 0);
    if (data && r == rows && c == cols) return; /* same geometry: the buffer (or the view) stays */
    release();
    rows = r; cols = c; step = (size_t)c;
    if ((size_t)r * (size_t)c > 0) {
      buf_ = std::make_shared<std::vector<uchar> >((size_t)r * (size_t)c);
      data = buf_->data();
    }
  }
  void release() { buf_.reset(); rows = cols = 0; step = 0; data = 0; sub_ = false; }
  static Mat zeros(int r, int c, int type) { Mat m(r, c, type); if (m.data) std::memset(m.data, 0, (size_t)r * (size_t)c); return m; }

  int type() const { return CV_8UC1; }
  bool empty() const { return data == 0 || rows == 0 || cols == 0; }
  size_t step1() const { return step; }
  bool isSubmatrix() const { return sub_; }

  template <typename T> T &at(int y, int x) { check_uchar<T>(); assert_in(y, x); return data[(size_t)y * step + x]; }
  template <typename T> const T &at(int y, int x) const { check_uchar<T>(); assert_in(y, x); return data[(size_t)y * step + x]; }
  uchar *ptr(int y = 0) { assert(y >= 0 && y < rows); return data + (size_t)y * step; }
  const uchar *ptr(int y = 0) const { assert(y >= 0 && y < rows); return data + (size_t)y * step; }

  Mat operator()(const Rect &r) const {
    assert(r.x >= 0 && r.y >= 0 && r.width >= 0 && r.height >= 0 && r.x + r.width <= cols && r.y + r.height <= rows);
    Mat v(*this);
    v.data = data + (size_t)r.y * step + r.x;
    v.rows = r.height; v.cols = r.width;
    v.sub_ = sub_ || r.width != cols || r.height != rows;
    return v;
  }
  Mat rowRange(int a, int b) const { return (*this)(Rect(0, a, cols, b - a)); }
  Mat colRange(int a, int b) const { return (*this)(Rect(a, 0, b - a, rows)); }
  Mat row(int y) const { return rowRange(y, y + 1); }

  Mat clone() const {
    Mat m(rows, cols, CV_8UC1);
    for (int y = 0; y < rows; y++) std::memcpy(m.data + (size_t)y * m.step, data + (size_t)y * step, (size_t)cols);
    return m;
  }
  inline void copyTo(const _OutputArray &dst) const;

 private:
  template <typename T> static void check_uchar() { static_assert(sizeof(T) == 1, "the stand-in Mat holds CV_8UC1 only"); }
  void assert_in(int y, int x) const { assert(data && y >= 0 && y < rows && x >= 0 && x < cols); (void)y; (void)x; }
  std::shared_ptr<std::vector<uchar> > buf_;
  bool sub_;
};

/* Array proxies: a pointer to the caller's Mat.  A proxy of a temporary (a row view) lives only for the call it is passed to. */
class _InputArray {
 public:
  _InputArray(const Mat &m) : m_(const_cast<Mat *>(&m)) {}
  bool empty() const { return m_->empty(); }
  Mat getMat() const { return *m_; }
 protected:
  Mat *m_;
};
class _OutputArray : public _InputArray {
 public:
  _OutputArray(Mat &m) : _InputArray(m) {}
  _OutputArray(const Mat &m) : _InputArray(m) {}
  void create(int r, int c, int type) const { m_->create(r, c, type); }
  void create(Size s, int type) const { m_->create(s.height, s.width, type); }
  void release() const { m_->release(); }
};
typedef const _InputArray &InputArray;
typedef const _OutputArray &OutputArray;

inline void Mat::copyTo(const _OutputArray &dst) const {
  dst.create(rows, cols, CV_8UC1);
  Mat d = dst.getMat();
  for (int y = 0; y < rows; y++) std::memmove(d.data + (size_t)y * d.step, data + (size_t)y * step, (size_t)cols);
}

/* ---- the primitives, forwarded to the oracle ------------------------------------------------------------------------------ */
inline float fastAtan2(float y, float x) { return orc_fast_atan2(y, x); }

/* cv::FAST(image, keypoints, threshold, nonmaxSuppression = true), TYPE_9_16: KeyPoint(x, y, 7.f, -1, score). */
inline void FAST(InputArray image, std::vector<KeyPoint> &keypoints, int threshold, bool nonmaxSuppression = true) {
  assert(nonmaxSuppression);
  Mat img = image.getMat();
  keypoints.clear();
  if (img.empty()) return;
  const int cap = (img.rows * img.cols) / 4 + 16;
  std::vector<int> xys((size_t)cap * 3);
  const int n = orc_fast9_16(img.data, img.cols, img.rows, img.step, threshold, xys.data(), cap);
  assert(n <= cap);
  keypoints.reserve((size_t)n);
  for (int i = 0; i < n; i++) keypoints.push_back(KeyPoint((float)xys[3 * i], (float)xys[3 * i + 1], 7.f, -1, (float)xys[3 * i + 2]));
}

inline void GaussianBlur(InputArray src, OutputArray dst, Size ksize, double sigmaX, double sigmaY = 0, int borderType = BORDER_REFLECT_101) {
  assert(ksize.width == 7 && ksize.height == 7 && sigmaX == 2 && sigmaY == 2 && borderType == BORDER_REFLECT_101);
  Mat s = src.getMat().clone(); /* the reference blurs in place; the oracle's blur may not alias */
  dst.create(s.rows, s.cols, CV_8UC1);
  Mat d = dst.getMat();
  if (s.empty()) return;
  orc_gaussian_blur7(s.data, s.cols, s.rows, s.step, d.data, d.step);
}

inline void resize(InputArray src, OutputArray dst, Size dsize, double fx = 0, double fy = 0, int interpolation = INTER_LINEAR) {
  assert(fx == 0 && fy == 0 && interpolation == INTER_LINEAR && dsize.width > 0 && dsize.height > 0);
  Mat s = src.getMat();
  assert(!s.empty());
  dst.create(dsize, CV_8UC1); /* a destination of that size already - the pyramid's view - is written in place */
  Mat d = dst.getMat();
  orc_resize_linear_u8(s.data, s.cols, s.rows, s.step, d.data, d.cols, d.rows, d.step);
}

inline void copyMakeBorder(InputArray src, OutputArray dst, int top, int bottom, int left, int right, int borderType) {
  assert(top == bottom && top == left && top == right && top >= 0);
  assert((borderType & ~BORDER_ISOLATED) == BORDER_REFLECT_101);
  Mat s0 = src.getMat();
  /* without BORDER_ISOLATED OpenCV reads a view's surroundings: only whole matrices are accepted then */
  assert((borderType & BORDER_ISOLATED) || !s0.isSubmatrix());
  Mat s = s0.clone(); /* the reference passes a view of the destination itself */
  dst.create(s.rows + 2 * top, s.cols + 2 * top, CV_8UC1);
  Mat d = dst.getMat();
  if (s.empty()) return;
  orc_copy_make_border101(s.data, s.cols, s.rows, s.step, d.data, top, d.step);
}

/* Named only by ComputeKeyPointsOld, which nothing calls. */
struct KeyPointsFilter {
  static void retainBest(std::vector<KeyPoint> &, int) {
    std::fprintf(stderr, "ref_shim: KeyPointsFilter::retainBest is not implemented\n");
    std::abort();
  }
};

}  // namespace cv

#endif
