/*
 * ref_cam_driver.cc -- extern "C" face of libref_cameras.so (TEST INFRASTRUCTURE).
 *
 * libref_cameras.so = the reference's own src/CameraModels/Pinhole.cpp and KannalaBrandt8.cpp, compiled unmodified against the
 * stand-in headers of oracle/ref_cam_shim, plus this file.  The reference's text is read from $(ORB_REFERENCE) at build time and is
 * never copied into this repository.  Every entry point constructs the reference's own Pinhole / KannalaBrandt8 objects from a
 * parameter vector and calls the member for each of n inputs.  cam_type: 0 = Pinhole (4 parameters), 1 = KannalaBrandt8 (8).
 *
 * The two TwoViewReconstruction members the camera files name are defined here and abort: no entry point reaches them.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <memory>
#include <vector>

#include "CameraModels/KannalaBrandt8.h"
#include "CameraModels/Pinhole.h"

namespace ORB_SLAM3 {
TwoViewReconstruction::TwoViewReconstruction(cv::Mat &, float, int) {
  fprintf(stderr, "ref_cam_driver: TwoViewReconstruction is not part of this library\n");
  abort();
}
bool TwoViewReconstruction::Reconstruct(const std::vector<cv::KeyPoint> &, const std::vector<cv::KeyPoint> &, const std::vector<int> &, cv::Mat &,
                                        cv::Mat &, std::vector<cv::Point3f> &, std::vector<bool> &) {
  fprintf(stderr, "ref_cam_driver: TwoViewReconstruction is not part of this library\n");
  abort();
}
}  // namespace ORB_SLAM3

namespace {

/* GeometricCamera's destructor is not virtual: each object is owned through its own class */
struct Camera {
  std::unique_ptr<ORB_SLAM3::Pinhole> pinhole;
  std::unique_ptr<ORB_SLAM3::KannalaBrandt8> kb8;
  Camera(int cam_type, const float *params) {
    if (cam_type == 0) pinhole.reset(new ORB_SLAM3::Pinhole(std::vector<float>(params, params + 4)));
    if (cam_type == 1) kb8.reset(new ORB_SLAM3::KannalaBrandt8(std::vector<float>(params, params + 8)));
  }
  ORB_SLAM3::GeometricCamera *get() const { return pinhole ? (ORB_SLAM3::GeometricCamera *)pinhole.get() : kb8.get(); }
};

/* R12 and t12 as Frame.cc takes them from Tlr: views into one 3 x 4 matrix */
cv::Mat mat34(const float *T) {
  cv::Mat m(3, 4, CV_32F);
  for (int i = 0; i < 12; i++) m.at<float>(i / 4, i % 4) = T[i];
  return m;
}

cv::KeyPoint keypoint(const float *xy) {
  cv::KeyPoint k;
  k.pt.x = xy[0];
  k.pt.y = xy[1];
  return k;
}

}  // namespace

extern "C" {

/* 1 in the <cmath> build (-DREF_CAM_SHIM_CMATH), 0 in the <math.h> one */
int refcam_cmath_build(void) {
#ifdef REF_CAM_SHIM_CMATH
  return 1;
#else
  return 0;
#endif
}

/* project(cv::Point3f): xyz [n][3] -> uv [n][2] */
int refcam_project(int cam_type, const float *params, int n, const float *xyz, float *uv) {
  const Camera holder(cam_type, params);
  ORB_SLAM3::GeometricCamera *cam = holder.get();
  if (!cam) return -1;
  for (int i = 0; i < n; i++) {
    const cv::Point2f p = cam->project(cv::Point3f(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
    uv[2 * i] = p.x;
    uv[2 * i + 1] = p.y;
  }
  return 0;
}

/* unproject: xy [n][2] -> rays [n][3] */
int refcam_unproject(int cam_type, const float *params, int n, const float *xy, float *rays) {
  const Camera holder(cam_type, params);
  ORB_SLAM3::GeometricCamera *cam = holder.get();
  if (!cam) return -1;
  for (int i = 0; i < n; i++) {
    const cv::Point3f r = cam->unproject(cv::Point2f(xy[2 * i], xy[2 * i + 1]));
    rays[3 * i] = r.x;
    rays[3 * i + 1] = r.y;
    rays[3 * i + 2] = r.z;
  }
  return 0;
}

/* KannalaBrandt8::TriangulateMatches of n keypoint pairs, R12 | t12 = Tlr [12].  depth [n] = the return value; p3d [n][3] is written
   where the function reaches its end (p3D assigned) and left alone elsewhere; exit_code [n] (optional): 0 parallax, 1 z1 <= 0,
   2 z2 <= 0, 3 first reprojection error, 4 second reprojection error, 5 accepted - told apart by how often the member reached the
   stand-in primitives (cv::shim::trace): no SVD; one dot product; two row pointers; two products; p3D empty; else the end. */
int refcam_kb8_triangulate_matches(const float *cam1, const float *cam2, const float *Tlr, int n, const float *kp1, const float *kp2,
                                   const float *sigma1, const float *sigma2, float *depth, float *p3d, uint8_t *exit_code) {
  ORB_SLAM3::KannalaBrandt8 c1(std::vector<float>(cam1, cam1 + 8)), c2(std::vector<float>(cam2, cam2 + 8));
  const cv::Mat T = mat34(Tlr);
  const cv::Mat R12 = T.rowRange(0, 3).colRange(0, 3), t12 = T.col(3);
  for (int i = 0; i < n; i++) {
    cv::Mat p3D;
    cv::shim::Trace &tr = cv::shim::trace();
    tr.gemm = tr.dot = tr.svd = tr.ptr = 0;
    depth[i] = c1.TriangulateMatches(&c2, keypoint(kp1 + 2 * i), keypoint(kp2 + 2 * i), R12, t12, sigma1[i], sigma2[i], p3D);
    const int code = tr.svd == 0 ? 0 : tr.dot == 1 ? 1 : tr.ptr == 2 ? 2 : tr.gemm == 2 ? 3 : p3D.empty() ? 4 : 5;
    if (exit_code) exit_code[i] = (uint8_t)code;
    if (!p3D.empty()) {
      if (p3D.rows != 3 || p3D.cols != 1) return -2;
      for (int k = 0; k < 3; k++) p3d[3 * i + k] = p3D.at<float>(k);
    }
  }
  return 0;
}

/* epipolarConstrain of n keypoint pairs with one R12 [9] / t12 [3]: verdict [n] = 0 / 1.  sigma [n] is sigmaLevel, unc [n] is unc. */
int refcam_epipolar_constrain(int cam_type, const float *cam1, const float *cam2, const float *R12, const float *t12, int n, const float *kp1,
                              const float *kp2, const float *sigma, const float *unc, uint8_t *verdict) {
  const Camera h1(cam_type, cam1), h2(cam_type, cam2);
  ORB_SLAM3::GeometricCamera *c1 = h1.get(), *c2 = h2.get();
  if (!c1 || !c2) return -1;
  cv::Mat R(3, 3, CV_32F), t(3, 1, CV_32F);
  for (int i = 0; i < 9; i++) R.at<float>(i / 3, i % 3) = R12[i];
  for (int i = 0; i < 3; i++) t.at<float>(i) = t12[i];
  for (int i = 0; i < n; i++)
    verdict[i] = c1->epipolarConstrain(c2, keypoint(kp1 + 2 * i), keypoint(kp2 + 2 * i), R, t, sigma[i], unc[i]) ? 1 : 0;
  return 0;
}

/* the stand-in's cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) itself: A [m][n] -> w [min(m, n)], u [m][m], vt [n][n] */
int refcam_svd(int m, int n, const float *A, float *w, float *u, float *vt) {
  cv::Mat a(m, n, CV_32F), W, U, Vt;
  for (int i = 0; i < m * n; i++) a.at<float>(i / n, i % n) = A[i];
  cv::SVD::compute(a, W, U, Vt, cv::SVD::MODIFY_A | cv::SVD::FULL_UV);
  if (U.rows != m || U.cols != m || Vt.rows != n || Vt.cols != n || W.rows != (m < n ? m : n)) return -2;
  for (int i = 0; i < W.rows; i++) w[i] = W.at<float>(i);
  for (int i = 0; i < m * m; i++) u[i] = U.at<float>(i / m, i % m);
  for (int i = 0; i < n * n; i++) vt[i] = Vt.at<float>(i / n, i % n);
  return 0;
}

}  // extern "C"
