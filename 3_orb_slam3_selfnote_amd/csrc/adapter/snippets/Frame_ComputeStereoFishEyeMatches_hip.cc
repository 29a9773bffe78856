// Frame_ComputeStereoFishEyeMatches_hip.cc -- drop-in body of void Frame::ComputeStereoFishEyeMatches(), replacing
// src/Frame.cc:1228-1268.
//
// Like the other member snippets: delete (or #if 0) those lines of src/Frame.cc and add this file to the library's sources
// (INTEGRATION.md section 3b).  One call, orbm_stereo_fisheye_matches, runs BFmatcher.knnMatch(k = 2) over the lapping rows on the
// matrix pipe, Lowe's ratio test and KannalaBrandt8::TriangulateMatches for every pair that passes it (one pair per lane, the
// cv::SVD restated as OpenCV's float Jacobi) and fills mvLeftToRightMatch, mvRightToLeftMatch, mvDepth and the 3-D points; the
// host only wraps the points into mvStereo3Dpoints.  A driver that keeps rig batches resident calls
// orbm_stereo_fisheye_matches_batch_device between orbm_rig_concat_batch_device and the searches instead and never comes here.
#include "Frame.h"

#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "GeometricCamera.h"
#include "orbhip.h"

namespace ORB_SLAM3 {

namespace {
orbm_t *stereo_fisheye_matcher() {   // one handle per thread, as in ORBmatcher_hip.cc
  thread_local orbm_t *m = nullptr;
  if (!m) {
    const char *e = std::getenv("ORBHIP_DEVICE");
    m = orbm_create(e ? std::atoi(e) : 0);
    if (!m) throw std::runtime_error("Frame::ComputeStereoFishEyeMatches: orbm_create failed (no usable HIP device; there is no CPU fallback)");
  }
  return m;
}
}  // namespace

void Frame::ComputeStereoFishEyeMatches() {
  mvLeftToRightMatch = std::vector<int>(Nleft, -1);   // :1236-1241
  mvRightToLeftMatch = std::vector<int>(Nright, -1);
  mvDepth = std::vector<float>(Nleft, -1.0f);
  mvuRight = std::vector<float>(Nleft, -1);
  mvStereo3Dpoints = std::vector<cv::Mat>(Nleft);
  mnCloseMPs = 0;
  if (mpCamera->GetType() != mpCamera->CAM_FISHEYE || mpCamera2->GetType() != mpCamera2->CAM_FISHEYE)
    throw std::runtime_error("Frame::ComputeStereoFishEyeMatches: both cameras must be KannalaBrandt8");   // the reference casts without asking (:1258)
  float cp[8], cp2[8], Tlr[12];
  for (int k = 0; k < 8; k++) { cp[k] = mpCamera->getParameter(k); cp2[k] = mpCamera2->getParameter(k); }
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) Tlr[4 * r + c] = mRlr.at<float>(r, c);
    Tlr[4 * r + 3] = mtlr.at<float>(r);
  }
  std::vector<float> p3d(3 * (size_t)(Nleft > 0 ? Nleft : 1), 0.f);
  orbm_t *m = stereo_fisheye_matcher();
  const int rc = orbm_stereo_fisheye_matches(m, reinterpret_cast<const orbx_keypoint_t *>(mvKeys.data()), mDescriptors.data, Nleft, monoLeft,
                                             reinterpret_cast<const orbx_keypoint_t *>(mvKeysRight.data()), mDescriptorsRight.data, Nright, monoRight,
                                             mvLevelSigma2.data(), (int)mvLevelSigma2.size(), Tlr, cp, cp2, mvLeftToRightMatch.data(),
                                             mvRightToLeftMatch.data(), mvDepth.data(), p3d.data(), NULL);
  if (rc < 0) throw std::runtime_error(std::string("Frame::ComputeStereoFishEyeMatches: ") + orbm_last_error(m));
  for (int i = 0; i < Nleft; i++) {
    if (mvLeftToRightMatch[i] < 0) continue;
    cv::Mat p3D(3, 1, CV_32F);   // :1262
    for (int r = 0; r < 3; r++) p3D.at<float>(r) = p3d[3 * (size_t)i + r];
    mvStereo3Dpoints[i] = p3D;
  }
}

}  // namespace ORB_SLAM3
