// TwoViewReconstruction_Reconstruct_hip.cc -- drop-in body of bool TwoViewReconstruction::Reconstruct(...), replacing
// src/TwoViewReconstruction.cc:39-127, against the reference's unmodified include/TwoViewReconstruction.h.
//
// Delete (or #if 0) lines 39-127 of src/TwoViewReconstruction.cc and add this file to the library's sources; the other members of the
// file may stay, nothing calls them any more.  Both camera models reach the member unchanged: Pinhole::ReconstructWithTwoViews
// (Pinhole.cpp:126-133) directly, KannalaBrandt8::ReconstructWithTwoViews behind its own undistortion (KannalaBrandt8.cpp:218-232).
//
// What stays the reference's: the filling of mvKeys1 / mvKeys2 / mvMatches12 / mvbMatched1 (:42-62) and the drawing of the minimal sets
// (:77-96) - DUtils::Random over libc rand(), seeded once per process, later calls continuing the stream; only this side of the call can
// reproduce that, and the library never calls rand().  Everything behind the draw is one call (orbm_two_view_reconstruct: the 2 x
// mMaxIterations hypotheses and scores, the motion hypotheses and CheckRT on the device; include/orbhip.h, TWO-VIEW RULE).
#include "TwoViewReconstruction.h"

#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "Thirdparty/DBoW2/DUtils/Random.h"
#include "orbhip.h"

namespace ORB_SLAM3 {

namespace {
orbm_t *two_view_matcher() {   // one handle per thread: the member runs on the tracking thread
  thread_local orbm_t *m = nullptr;
  if (!m) {
    const char *e = std::getenv("ORBHIP_DEVICE");
    m = orbm_create(e ? std::atoi(e) : 0);
    if (!m) throw std::runtime_error("TwoViewReconstruction::Reconstruct: orbm_create failed (no usable HIP device; there is no CPU fallback)");
  }
  return m;
}
}  // namespace

bool TwoViewReconstruction::Reconstruct(const std::vector<cv::KeyPoint> &vKeys1, const std::vector<cv::KeyPoint> &vKeys2,
                                        const std::vector<int> &vMatches12, cv::Mat &R21, cv::Mat &t21, std::vector<cv::Point3f> &vP3D,
                                        std::vector<bool> &vbTriangulated) {
  static_assert(sizeof(cv::KeyPoint) == sizeof(orbx_keypoint_t), "orbx_keypoint_t mirrors cv::KeyPoint");
  mvKeys1 = vKeys1;
  mvKeys2 = vKeys2;

  // the matches with the reference frame, :50-62
  mvMatches12.clear();
  mvMatches12.reserve(mvKeys2.size());
  mvbMatched1.resize(mvKeys1.size());
  for (size_t i = 0, iend = vMatches12.size(); i < iend; i++) {
    const bool matched = vMatches12[i] >= 0;
    if (matched) mvMatches12.push_back(std::make_pair((int)i, vMatches12[i]));
    mvbMatched1[i] = matched;
  }
  const int N = (int)mvMatches12.size();
  if (N < 8) return false;   // the reference's draw below runs off vAvailableIndices here; Tracking asks for 100 matches (Tracking.cc:2479)

  // the minimal sets, :66-96: the same calls of DUtils::Random in the same order
  mvSets = std::vector<std::vector<size_t> >(mMaxIterations, std::vector<size_t>(8, 0));
  DUtils::Random::SeedRandOnce(0);
  std::vector<size_t> vAllIndices((size_t)N), vAvailableIndices;
  for (int i = 0; i < N; i++) vAllIndices[i] = i;
  std::vector<int32_t> sets((size_t)mMaxIterations * 8);
  for (int it = 0; it < mMaxIterations; it++) {
    vAvailableIndices = vAllIndices;
    for (size_t j = 0; j < 8; j++) {
      const int randi = DUtils::Random::RandomInt(0, (int)vAvailableIndices.size() - 1);
      mvSets[it][j] = vAvailableIndices[randi];
      sets[(size_t)it * 8 + j] = (int32_t)vAvailableIndices[randi];
      vAvailableIndices[randi] = vAvailableIndices.back();
      vAvailableIndices.pop_back();
    }
  }

  // :98-126 in one call
  std::vector<int32_t> matches12(vMatches12.begin(), vMatches12.end());
  matches12.resize(mvKeys1.size(), -1);
  float K[9], R[9], t[3];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) K[3 * r + c] = mK.at<float>(r, c);
  const size_t n1 = mvKeys1.size();
  std::vector<float> p3d(3 * n1 + 3);
  std::vector<uint8_t> tri(n1 + 1);
  orbm_t *m = two_view_matcher();
  const int rc = orbm_two_view_reconstruct(m, reinterpret_cast<const orbx_keypoint_t *>(mvKeys1.data()), (int)n1,
                                           reinterpret_cast<const orbx_keypoint_t *>(mvKeys2.data()), (int)mvKeys2.size(), matches12.data(), K,
                                           mSigma, mMaxIterations, sets.data(), R, t, p3d.data(), tri.data(), NULL);
  if (rc < 0) throw std::runtime_error(std::string("TwoViewReconstruction::Reconstruct: ") + orbm_last_error(m));
  if (rc == 0) return false;
  R21 = cv::Mat(3, 3, CV_32F);
  t21 = cv::Mat(3, 1, CV_32F);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) R21.at<float>(r, c) = R[3 * r + c];
    t21.at<float>(r) = t[r];
  }
  vP3D.resize(n1);
  vbTriangulated.assign(n1, false);
  for (size_t i = 0; i < n1; i++) {
    vP3D[i] = cv::Point3f(p3d[3 * i], p3d[3 * i + 1], p3d[3 * i + 2]);
    vbTriangulated[i] = tri[i] != 0;
  }
  return true;
}

}  // namespace ORB_SLAM3
