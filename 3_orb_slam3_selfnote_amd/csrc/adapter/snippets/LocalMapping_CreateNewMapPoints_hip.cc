// LocalMapping_CreateNewMapPoints_hip.cc -- the neighbour loop of void LocalMapping::CreateNewMapPoints() (src/LocalMapping.cc:525-583)
// with ONE search for all neighbours in front of it instead of one ORBmatcher::SearchForTriangulation call per neighbour.
//
// The geometric body of the loop - parallax, linear triangulation, the reprojection and scale tests, the new MapPoint
// (src/LocalMapping.cc:585-900) - stays where it is, unchanged.  Add this file to the library's sources and make three edits in
// src/LocalMapping.cc:
//   1. in front of the loop (:525), once bCoarse's expression of :577-581 has been moved up there:
//        NeighbourTriangulation search(mpCurrentKeyFrame, vpNeighKFs, mbMonocular, bCoarse);
//   2. the baseline tests (:535-560) become            if (search.skipped(i)) continue;
//      (the constructor has evaluated exactly those tests, once, into the `skip` table of the call);
//   3. the search (:583) becomes                       search.matched_indices(i, vMatchedIndices);
// `if(i>0 && CheckNewKeyFrames()) return;` (:528) stays: the rows of the neighbours that are not reached are dropped.
//
// Why the K searches may be made before the loop although its body gives keypoints of mpCurrentKeyFrame map points (AddMapPoint,
// :892) - the masking rule of include/orbhip.h: the member reads of KF1 only GetMapPoint(idx1), per idx1 (ORBmatcher.cc:1049-1055),
// vbMatched2 is never set (:1027, :1083), neighbour i's own map points change only in iteration i (:893), and the matcher is built
// with checkOri = false (:500).  So the sequential result for neighbour i is row i from the state at loop entry without the idx1 that
// received a map point since: matched_indices() drops those.  bCoarse is read once at loop entry, where the reference reads the
// tracker's state again per neighbour.
//
// The entry is chosen by camera model as in ORBmatcher_hip.cc: Pinhole throughout -> orbm_search_for_triangulation_neighbours,
// KannalaBrandt8 throughout (single cameras or rigs) -> orbm_search_for_triangulation_kb8_neighbours; anything else keeps the per-pair
// member (whose generic-predicate route calls the reference's own epipolarConstrain), made when the loop reaches the neighbour.
#include <cstdlib>
#include <cstring>
#include <list>   // Map.h names std::list without including it
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "LocalMapping.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "ORBmatcher.h"
#include "orbhip.h"

namespace ORB_SLAM3 {

namespace {
orbm_t *neighbours_matcher() {   // one handle per thread, as in ORBmatcher_hip.cc
  thread_local orbm_t *m = nullptr;
  if (!m) {
    const char *e = std::getenv("ORBHIP_DEVICE");
    m = orbm_create(e ? std::atoi(e) : 0);
    if (!m) throw std::runtime_error("LocalMapping::CreateNewMapPoints: orbm_create failed (no usable HIP device; there is no CPU fallback)");
  }
  return m;
}

// The slice of a KeyFrame the search reads, flattened (the Side of ORBmatcher_hip.cc)
struct FlatKeyFrame {
  std::vector<uint32_t> id;
  std::vector<int32_t> start, idx;
  std::vector<uint8_t> has;
  std::vector<cv::KeyPoint> keys;
  std::vector<float> ur;
  orbm_keyframe_t k;
  explicit FlatKeyFrame(KeyFrame *pKF) : has(pKF->N) {
    std::memset(&k, 0, sizeof(k));
    start.push_back(0);
    for (DBoW2::FeatureVector::const_iterator it = pKF->mFeatVec.begin(); it != pKF->mFeatVec.end(); ++it) {
      id.push_back(it->first);
      for (size_t m = 0; m < it->second.size(); m++) idx.push_back((int32_t)it->second[m]);
      start.push_back((int32_t)idx.size());
    }
    for (int i = 0; i < pKF->N; i++) has[i] = pKF->GetMapPoint(i) != NULL;
    if (pKF->NLeft != -1) { keys = pKF->mvKeys; keys.insert(keys.end(), pKF->mvKeysRight.begin(), pKF->mvKeysRight.end()); }  // ORBmatcher.cc:1064-1066
    else keys = pKF->mvKeysUn;
    keys.resize(pKF->N);
    // bStereo = !mpCamera2 && mvuRight[idx] >= 0 (ORBmatcher.cc:1059, :1086): always false on a rig
    if (pKF->mpCamera2 || (int)pKF->mvuRight.size() < pKF->N) ur.assign(pKF->N, -1.0f); else ur = pKF->mvuRight;
  }
  void bind(KeyFrame *pKF) {   // after the object has reached its final address
    k.n = pKF->N;
    k.keys_un = reinterpret_cast<const orbx_keypoint_t *>(keys.data());
    k.descriptors = pKF->mDescriptors.data;
    k.u_right = ur.data();
    k.has_mappoint = has.data();
    k.n_nodes = (int32_t)id.size();
    k.node_id = id.data(); k.node_start = start.data(); k.node_idx = idx.data();
    k.scale_factors = pKF->mvScaleFactors.data(); k.level_sigma2 = pKF->mvLevelSigma2.data();
    k.nlevels = (int32_t)pKF->mvScaleFactors.size();
  }
};

void mat33_of(const cv::Mat &M, float *o) { for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) o[3 * r + c] = M.at<float>(r, c); }
void vec3_of(const cv::Mat &M, float *o) { for (int r = 0; r < 3; r++) o[r] = M.at<float>(r); }
void pose_of(const cv::Mat &R, const cv::Mat &t, float *o) {   // [R | t], row stride 4
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) o[4 * r + c] = R.at<float>(r, c);
    o[4 * r + 3] = t.at<float>(r);
  }
}
}  // namespace

struct NeighbourTriangulation {
  KeyFrame *mpCurrentKeyFrame;
  std::vector<KeyFrame *> vpNeighKFs;
  bool bCoarse, batched;
  std::vector<uint8_t> skip;
  std::vector<int32_t> matches12;   // [K][N1], batched only
  int N1;

  NeighbourTriangulation(KeyFrame *pKF1, const std::vector<KeyFrame *> &neighbours, bool bMonocular, bool coarse)
      : mpCurrentKeyFrame(pKF1), vpNeighKFs(neighbours), bCoarse(coarse), batched(false), skip(neighbours.size(), 0), N1(pKF1->N) {
    const int K = (int)vpNeighKFs.size();
    // the baseline tests, src/LocalMapping.cc:535-560
    cv::Mat Ow1 = pKF1->GetCameraCenter();
    int searched = 0;
    for (int i = 0; i < K; i++) {
      KeyFrame *pKF2 = vpNeighKFs[i];
      cv::Mat vBaseline = pKF2->GetCameraCenter() - Ow1;
      const float baseline = cv::norm(vBaseline);
      if (!bMonocular) {
        if (baseline < pKF2->mb) skip[i] = 1;
      } else {
        const float medianDepthKF2 = pKF2->ComputeSceneMedianDepth(2);
        const float ratioBaselineDepth = baseline / medianDepthKF2;
        if (ratioBaselineDepth < 0.01) skip[i] = 1;
      }
      searched += !skip[i];
    }
    if (searched == 0) return;
    // one camera model throughout?  (the routing of ORBmatcher_hip.cc)
    const bool rig = pKF1->mpCamera2 != NULL;
    bool pinhole = !rig && pKF1->mpCamera->GetType() == 0;
    bool fisheye = (pKF1->NLeft != -1) == rig && pKF1->mpCamera->GetType() == 1 && (!rig || pKF1->mpCamera2->GetType() == 1);
    for (int i = 0; i < K; i++) {
      if (skip[i]) continue;
      KeyFrame *pKF2 = vpNeighKFs[i];
      pinhole = pinhole && !pKF2->mpCamera2 && pKF2->mpCamera->GetType() == 0;
      fisheye = fisheye && (pKF2->mpCamera2 != NULL) == rig && (pKF2->NLeft != -1) == rig && pKF2->mpCamera->GetType() == 1 &&
                (!rig || pKF2->mpCamera2->GetType() == 1);
    }
    if (!pinhole && !fisheye) return;   // per pair, when the loop gets there
    // flatten KF1 once and the neighbours once
    FlatKeyFrame A(pKF1);
    A.bind(pKF1);
    std::vector<FlatKeyFrame> B;
    B.reserve(K);
    std::vector<orbm_keyframe_t> tab(K);
    std::memset(tab.data(), 0, sizeof(orbm_keyframe_t) * (size_t)K);
    for (int i = 0; i < K; i++) {
      if (skip[i]) continue;            // a skipped neighbour is neither flattened nor read
      B.push_back(FlatKeyFrame(vpNeighKFs[i]));
      B.back().bind(vpNeighKFs[i]);
      tab[i] = B.back().k;
    }
    matches12.assign((size_t)K * (size_t)(N1 > 0 ? N1 : 1), -1);
    std::vector<int32_t> nmatches(K, 0);
    cv::Mat R1w = pKF1->GetRotation(), t1w = pKF1->GetTranslation(), Cw = pKF1->GetCameraCenter();
    int rc;
    if (pinhole) {
      float fR1w[9], ft1w[3], fCw[3], cam1[4];
      mat33_of(R1w, fR1w); vec3_of(t1w, ft1w); vec3_of(Cw, fCw);
      for (int k = 0; k < 4; k++) cam1[k] = pKF1->mpCamera->getParameter(k);
      std::vector<float> R2w((size_t)K * 9, 0.f), t2w((size_t)K * 3, 0.f), cam2((size_t)K * 4, 0.f);
      for (int i = 0; i < K; i++) {
        if (skip[i]) continue;
        mat33_of(vpNeighKFs[i]->GetRotation(), &R2w[(size_t)i * 9]);
        vec3_of(vpNeighKFs[i]->GetTranslation(), &t2w[(size_t)i * 3]);
        for (int k = 0; k < 4; k++) cam2[(size_t)i * 4 + k] = vpNeighKFs[i]->mpCamera->getParameter(k);
      }
      rc = orbm_search_for_triangulation_neighbours(neighbours_matcher(), &A.k, K, tab.data(), fR1w, ft1w, fCw, cam1, R2w.data(), t2w.data(), cam2.data(),
                                                    skip.data(), 0, bCoarse ? 1 : 0, matches12.data(), nmatches.data());
    } else {
      float cams1[2][8] = {};
      for (int k = 0; k < 8; k++) {
        cams1[0][k] = pKF1->mpCamera->getParameter(k);
        if (rig) cams1[1][k] = pKF1->mpCamera2->getParameter(k);
      }
      std::vector<float> ep((size_t)K * 2, 0.f), cams2((size_t)K * 16, 0.f), T12((size_t)K * 48, 0.f);
      std::vector<int32_t> n_left2(K, -1);
      for (int i = 0; i < K; i++) {
        if (skip[i]) continue;
        KeyFrame *pKF2 = vpNeighKFs[i];
        cv::Mat R2w = pKF2->GetRotation(), t2w = pKF2->GetTranslation();
        cv::Mat C2 = R2w * Cw + t2w;                                            // ORBmatcher.cc:988-993
        const cv::Point2f e = pKF2->mpCamera->project(C2);
        ep[(size_t)i * 2] = e.x; ep[(size_t)i * 2 + 1] = e.y;
        n_left2[i] = rig ? pKF2->NLeft : -1;
        for (int k = 0; k < 8; k++) {
          cams2[(size_t)i * 16 + k] = pKF2->mpCamera->getParameter(k);
          if (rig) cams2[(size_t)i * 16 + 8 + k] = pKF2->mpCamera2->getParameter(k);
        }
        float *T = &T12[(size_t)i * 48];
        if (!rig) {                                                             // ORBmatcher.cc:1007-1008
          cv::Mat R12 = R1w * R2w.t();
          cv::Mat t12 = -R1w * R2w.t() * t2w + t1w;
          pose_of(R12, t12, T);
        } else {                                                                // ORBmatcher.cc:1011-1019: ll, lr, rl, rr
          cv::Mat Rr1 = pKF1->GetRightRotation(), tr1 = pKF1->GetRightTranslation();
          cv::Mat Rr2 = pKF2->GetRightRotation(), tr2 = pKF2->GetRightTranslation();
          cv::Mat Rll = R1w * R2w.t(), Rlr = R1w * Rr2.t(), Rrl = Rr1 * R2w.t(), Rrr = Rr1 * Rr2.t();
          cv::Mat tll = R1w * (-R2w.t() * t2w) + t1w, tlr = R1w * (-Rr2.t() * tr2) + t1w;
          cv::Mat trl = Rr1 * (-R2w.t() * t2w) + tr1, trr = Rr1 * (-Rr2.t() * tr2) + tr1;
          pose_of(Rll, tll, T); pose_of(Rlr, tlr, T + 12); pose_of(Rrl, trl, T + 24); pose_of(Rrr, trr, T + 36);
        }
      }
      rc = orbm_search_for_triangulation_kb8_neighbours(neighbours_matcher(), &A.k, rig ? pKF1->NLeft : -1, K, tab.data(), n_left2.data(), ep.data(),
                                                        &cams1[0][0], cams2.data(), T12.data(), skip.data(), 0, bCoarse ? 1 : 0, matches12.data(),
                                                        nmatches.data());
    }
    if (rc < 0) throw std::runtime_error(std::string("LocalMapping::CreateNewMapPoints (liborbhip): ") + orbm_last_error(neighbours_matcher()));
    batched = true;
  }

  // src/LocalMapping.cc:535-560
  bool skipped(size_t i) const { return skip[i] != 0; }

  // src/LocalMapping.cc:583: vMatchedIndices of neighbour i as the sequential loop would find them now
  int matched_indices(size_t i, std::vector<std::pair<size_t, size_t> > &vMatchedIndices) const {
    if (!batched) {   // another camera model: the per-pair member, from the current state
      ORBmatcher matcher(0.6f, false);
      return matcher.SearchForTriangulation(mpCurrentKeyFrame, vpNeighKFs[i], cv::Mat(), vMatchedIndices, false, bCoarse);
    }
    vMatchedIndices.clear();
    const int32_t *row = &matches12[i * (size_t)(N1 > 0 ? N1 : 1)];
    for (int idx1 = 0; idx1 < N1; idx1++) {
      if (row[idx1] < 0) continue;
      if (mpCurrentKeyFrame->GetMapPoint(idx1)) continue;   // the mask: idx1 received a map point in an earlier iteration (:892)
      vMatchedIndices.push_back(std::make_pair((size_t)idx1, (size_t)row[idx1]));
    }
    return (int)vMatchedIndices.size();
  }
};

}  // namespace ORB_SLAM3
