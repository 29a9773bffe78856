/*
 * ref_driver.cc -- extern "C" face of libref_extractor.so (TEST INFRASTRUCTURE).
 *
 * libref_extractor.so = the reference's own ORBextractor.cc, compiled unmodified against the stand-in containers of
 * oracle/ref_shim (primitives forwarded to liborb_oracle.so), plus this file.  The reference's text is read from $(ORB_REFERENCE)
 * at build time and is never copied into this repository.
 *
 * The pointer tie.  DistributeOctTree sorts pair<int, ExtractorNode*> (ORBextractor.cc:682), so nodes of equal size are ordered by
 * their heap addresses: with the ordinary heap the result depends on the allocator's history.  This library replaces operator
 * new by a monotone bump allocator over one reserved virtual range (delete is a no-op), restarted by every ref_* call, so that a
 * later-created node always compares greater - the creation-order definition orb_oracle.c states for the tie.  The replacement
 * is bound inside this library only (-Wl,-Bsymbolic and a version script that exports ref_* alone).  Not thread-safe.
 * -DREF_DRIVER_SYSTEM_HEAP leaves the ordinary heap in place: for a stand-alone sanitizer build of this file, and to see the
 * allocator dependence itself.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <new>
#include <vector>

#include "ORBextractor.h"
#include "orb_oracle.h"

#ifdef REF_DRIVER_SYSTEM_HEAP
static void bump_reset() {}
#else
/* ---- monotone allocator --------------------------------------------------------------------------------------------------- */
static const size_t kBumpBytes = (size_t)4 << 30; /* address space only: pages are touched as they are used */
static char *g_base = 0;
static size_t g_used = 0;

static void *bump_alloc(size_t n) {
  if (!g_base) {
    void *p = mmap(0, kBumpBytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (p == MAP_FAILED) { perror("ref_driver: mmap"); abort(); }
    g_base = (char *)p;
  }
  n = (n + 15) & ~(size_t)15;
  if (n > kBumpBytes - g_used) { fprintf(stderr, "ref_driver: the allocator's range is exhausted\n"); abort(); }
  void *r = g_base + g_used;
  g_used += n ? n : 16;
  return r;
}
static void bump_reset() {
  if (g_base && g_used) madvise(g_base, g_used, MADV_DONTNEED); /* hand the pages back; the range stays reserved */
  g_used = 0;
}

void *operator new(size_t n) { return bump_alloc(n); }
void *operator new[](size_t n) { return bump_alloc(n); }
void *operator new(size_t n, const std::nothrow_t &) noexcept { return bump_alloc(n); }
void *operator new[](size_t n, const std::nothrow_t &) noexcept { return bump_alloc(n); }
void operator delete(void *) noexcept {}
void operator delete[](void *) noexcept {}
void operator delete(void *, const std::nothrow_t &) noexcept {}
void operator delete[](void *, const std::nothrow_t &) noexcept {}
#endif

/* ---- the protected members, through a derived class ------------------------------------------------------------------------ */
namespace {

class Probe : public ORB_SLAM3::ORBextractor {
 public:
  Probe(int nfeatures, float scaleFactor, int nlevels, int iniTh, int minTh) : ORBextractor(nfeatures, scaleFactor, nlevels, iniTh, minTh) {}
  void pyramid(const cv::Mat &image) { ComputePyramid(image); }
  void level_keypoints(std::vector<std::vector<cv::KeyPoint> > &all) { ComputeKeyPointsOctTree(all); }
  std::vector<cv::KeyPoint> distribute(const std::vector<cv::KeyPoint> &keys, int minX, int maxX, int minY, int maxY, int N) {
    return DistributeOctTree(keys, minX, maxX, minY, maxY, N, 0);
  }
  int features_of_level(int l) const { return mnFeaturesPerLevel[l]; }
};

cv::Mat wrap(const uint8_t *img, int rows, int cols, size_t stride) {
  cv::Mat m(rows, cols, CV_8UC1);
  for (int y = 0; y < rows; y++) memcpy(m.ptr(y), img + (size_t)y * stride, (size_t)cols);
  return m;
}

orc_keypoint pack(const cv::KeyPoint &k) {
  orc_keypoint o;
  o.x = k.pt.x; o.y = k.pt.y; o.size = k.size; o.angle = k.angle; o.response = k.response;
  o.octave = k.octave; o.class_id = k.class_id;
  return o;
}

}  // namespace

#define REF_E_EXCEPTION (-3)

extern "C" {

/* ORBextractor::operator().  Returns monoIndex, -1 for an empty image, -2 when cap is too small (*n_out = the count), -3 when
 * the reference threw. */
int ref_extract(int nfeatures, float scaleFactor, int nlevels, int iniTh, int minTh, const uint8_t *img, int rows, int cols,
                size_t stride, int lap0, int lap1, orc_keypoint *kps, uint8_t *desc, int cap, int *n_out) {
  bump_reset();
  *n_out = 0;
  try {
    Probe ex(nfeatures, scaleFactor, nlevels, iniTh, minTh);
    cv::Mat image = (img && rows > 0 && cols > 0) ? wrap(img, rows, cols, stride) : cv::Mat();
    std::vector<cv::KeyPoint> keys;
    cv::Mat descriptors;
    std::vector<int> lap(2);
    lap[0] = lap0; lap[1] = lap1;
    const int mono = ex(image, cv::Mat(), keys, descriptors, lap);
    if (mono < 0) return mono;
    *n_out = (int)keys.size();
    if ((int)keys.size() > cap) return -2;
    for (size_t i = 0; i < keys.size(); i++) {
      kps[i] = pack(keys[i]);
      memcpy(desc + 32 * i, descriptors.ptr((int)i), 32);
    }
    return mono;
  } catch (...) {
    return REF_E_EXCEPTION;
  }
}

/* Level sizes of the public mvImagePyramid after ComputePyramid. */
int ref_pyramid_sizes(int nfeatures, float scaleFactor, int nlevels, int iniTh, int minTh, const uint8_t *img, int rows, int cols,
                      size_t stride, int *lcols, int *lrows) {
  bump_reset();
  try {
    Probe ex(nfeatures, scaleFactor, nlevels, iniTh, minTh);
    ex.pyramid(wrap(img, rows, cols, stride));
    for (int l = 0; l < nlevels; l++) { lcols[l] = ex.mvImagePyramid[l].cols; lrows[l] = ex.mvImagePyramid[l].rows; }
    return nlevels;
  } catch (...) {
    return REF_E_EXCEPTION;
  }
}

/* mvImagePyramid, each level with `border` (0 .. 19) pixels of the padded buffer around it, into levels[l] (tight rows of
 * lcols + 2 * border bytes). */
int ref_pyramid(int nfeatures, float scaleFactor, int nlevels, int iniTh, int minTh, const uint8_t *img, int rows, int cols,
                size_t stride, int border, uint8_t **levels) {
  bump_reset();
  if (border < 0 || border > 19) return -1;
  try {
    Probe ex(nfeatures, scaleFactor, nlevels, iniTh, minTh);
    ex.pyramid(wrap(img, rows, cols, stride));
    for (int l = 0; l < nlevels; l++) {
      const cv::Mat &m = ex.mvImagePyramid[l];
      const size_t w = (size_t)(m.cols + 2 * border);
      for (int y = -border; y < m.rows + border; y++)
        memcpy(levels[l] + (size_t)(y + border) * w, m.data + (ptrdiff_t)y * (ptrdiff_t)m.step - border, w);
    }
    return nlevels;
  } catch (...) {
    return REF_E_EXCEPTION;
  }
}

/* allKeypoints of ComputeKeyPointsOctTree: per level, in level coordinates (border added, before the scaling of operator()),
 * with size, octave and angle set.  kps holds the levels one after the other, counts[l] their sizes.  Returns the total
 * (-2 - total when cap is too small). */
int ref_level_keypoints(int nfeatures, float scaleFactor, int nlevels, int iniTh, int minTh, const uint8_t *img, int rows, int cols,
                        size_t stride, orc_keypoint *kps, int cap, int *counts) {
  bump_reset();
  try {
    Probe ex(nfeatures, scaleFactor, nlevels, iniTh, minTh);
    ex.pyramid(wrap(img, rows, cols, stride));
    std::vector<std::vector<cv::KeyPoint> > all;
    ex.level_keypoints(all);
    int total = 0;
    for (int l = 0; l < nlevels; l++) total += (counts[l] = (int)all[l].size());
    if (total > cap) return -2 - total;
    int n = 0;
    for (int l = 0; l < nlevels; l++)
      for (size_t i = 0; i < all[l].size(); i++) kps[n++] = pack(all[l][i]);
    return total;
  } catch (...) {
    return REF_E_EXCEPTION;
  }
}

/* DistributeOctTree on (x, y, response) triplets, as orc_distribute_octtree.  Returns the count (-3: the reference threw). */
int ref_distribute_octtree(const float *xyr, int n, int minX, int maxX, int minY, int maxY, int N, float *out, int cap) {
  bump_reset();
  try {
    Probe ex(1000, 1.2f, 8, 20, 7);
    std::vector<cv::KeyPoint> keys;
    keys.reserve((size_t)n);
    for (int i = 0; i < n; i++) keys.push_back(cv::KeyPoint(xyr[3 * i], xyr[3 * i + 1], 7.f, -1, xyr[3 * i + 2]));
    std::vector<cv::KeyPoint> r = ex.distribute(keys, minX, maxX, minY, maxY, N);
    for (size_t i = 0; i < r.size() && (int)i < cap; i++) {
      out[3 * i] = r[i].pt.x; out[3 * i + 1] = r[i].pt.y; out[3 * i + 2] = r[i].response;
    }
    return (int)r.size();
  } catch (...) {
    return REF_E_EXCEPTION;
  }
}

/* Constructor state, for comparison with orc_extractor_init. */
int ref_features_per_level(int nfeatures, float scaleFactor, int nlevels, int iniTh, int minTh, int *out) {
  bump_reset();
  try {
    Probe ex(nfeatures, scaleFactor, nlevels, iniTh, minTh);
    for (int l = 0; l < nlevels; l++) out[l] = ex.features_of_level(l);
    return nlevels;
  } catch (...) {
    return REF_E_EXCEPTION;
  }
}

}  /* extern "C" */
