// LocalMapping_CreateNewMapPoints_hip.cc -- the neighbour loop of void LocalMapping::CreateNewMapPoints() (src/LocalMapping.cc:525-583)
// with ONE search for all neighbours in front of it instead of one ORBmatcher::SearchForTriangulation call per neighbour - and, on
// request, the geometric body of the loop (:585-880) in the same call.
//
// Search-only form: the geometric body of the loop - parallax, linear triangulation, the reprojection and scale tests, the new MapPoint
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
// With `geometry` set the constructor goes one step further (orbm_create_new_map_points / orbm_create_new_map_points_kb8): the body of
// the loop runs on the device too, and the loop body from :585 to :880 becomes
//        for (const orbm_new_point_t *p = search.new_points_begin(i); p != search.new_points_end(i); ++p) {
//          cv::Mat x3D = search.x3D(*p); const int idx1 = p->idx1, idx2 = p->idx2;
//          MapPoint *pMP = new MapPoint(x3D, mpCurrentKeyFrame, mpAtlas->GetCurrentMap());     // :883
//          ... :889-902 unchanged ...
//        }
// The list holds what the sequential loop creates (the SEQUENTIAL RULE of include/orbhip.h: an accepted pair whose idx1 no earlier
// neighbour had accepted), in its order; a `return` at :528 in front of neighbour i simply leaves the entries of neighbours >= i unused.
// Where the camera models are mixed (has_new_points() false) the search-only form and the reference's own body remain.
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

// What the body of the loop reads of a KeyFrame beyond FlatKeyFrame (orbm_keyframe_geometry_t)
struct FlatGeometry {
  float Tcw[12], Ow[3], TcwRight[12], OwRight[3], Twc[12];
  orbm_keyframe_geometry_t g;
  static void rows_of(const cv::Mat &T, float *o) { for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) o[4 * r + c] = T.at<float>(r, c); }
  explicit FlatGeometry(KeyFrame *pKF) {
    std::memset(&g, 0, sizeof(g));
    rows_of(pKF->GetPose(), Tcw);
    rows_of(pKF->GetPoseInverse(), Twc);
    cv::Mat O = pKF->GetCameraCenter();
    for (int r = 0; r < 3; r++) Ow[r] = O.at<float>(r);
    if (pKF->mpCamera2) {
      rows_of(pKF->GetRightPose(), TcwRight);
      cv::Mat Or = pKF->GetRightCameraCenter();
      for (int r = 0; r < 3; r++) OwRight[r] = Or.at<float>(r);
    }
    g.fx = pKF->fx; g.fy = pKF->fy; g.cx = pKF->cx; g.cy = pKF->cy; g.invfx = pKF->invfx; g.invfy = pKF->invfy; g.mb = pKF->mb; g.mbf = pKF->mbf;
  }
  void bind(KeyFrame *pKF) {   // after the object has reached its final address
    g.Tcw = Tcw; g.Ow = Ow; g.Twc = Twc;
    g.Tcw_right = pKF->mpCamera2 ? TcwRight : NULL;
    g.Ow_right = pKF->mpCamera2 ? OwRight : NULL;
    const bool arrays = !pKF->mpCamera2 && (int)pKF->mvDepth.size() >= pKF->N && (int)pKF->mvKeys.size() >= pKF->N;
    g.depth = arrays ? pKF->mvDepth.data() : NULL;
    g.keys = arrays ? reinterpret_cast<const orbx_keypoint_t *>(pKF->mvKeys.data()) : NULL;
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
  bool bCoarse, batched, listed;
  std::vector<uint8_t> skip;
  std::vector<int32_t> matches12;   // [K][N1], batched only
  std::vector<orbm_new_point_t> points;   // geometry only: the new map points in creation order
  std::vector<size_t> first_of;           // [K + 1]: the entries of neighbour i are points[first_of[i] .. first_of[i + 1])
  int N1;

  // geometry: also run the body of the loop (:605-880) on the device; bFarPoints / thFarPoints = mbFarPoints / mThFarPoints
  NeighbourTriangulation(KeyFrame *pKF1, const std::vector<KeyFrame *> &neighbours, bool bMonocular, bool coarse, bool geometry = false,
                         bool bFarPoints = false, float thFarPoints = 0.f)
      : mpCurrentKeyFrame(pKF1), vpNeighKFs(neighbours), bCoarse(coarse), batched(false), listed(false), skip(neighbours.size(), 0),
        first_of(neighbours.size() + 1, 0), N1(pKF1->N) {
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
    // ... and, for the body of the loop, their poses, intrinsics, mvDepth and mvKeys
    std::vector<FlatGeometry> GB;
    std::vector<orbm_keyframe_geometry_t> gtab(K);
    std::memset(gtab.data(), 0, sizeof(orbm_keyframe_geometry_t) * (size_t)K);
    FlatGeometry GA(pKF1);
    GA.bind(pKF1);
    if (geometry) {
      GB.reserve(K);
      for (int i = 0; i < K; i++) {
        if (skip[i]) continue;
        GB.push_back(FlatGeometry(vpNeighKFs[i]));
      }
      for (int i = 0, b = 0; i < K; i++) {
        if (skip[i]) continue;
        GB[b].bind(vpNeighKFs[i]);
        gtab[i] = GB[b++].g;
      }
      points.resize(N1 > 0 ? N1 : 1);   // an idx1 appears at most once
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
      if (geometry)
        rc = orbm_create_new_map_points(neighbours_matcher(), &A.k, &GA.g, pKF1->mfScaleFactor, K, tab.data(), gtab.data(), fR1w, ft1w, fCw, cam1, R2w.data(),
                                        t2w.data(), cam2.data(), skip.data(), bCoarse ? 1 : 0, bFarPoints ? 1 : 0, thFarPoints, points.data(), N1, NULL,
                                        matches12.data(), nmatches.data());
      else
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
      if (geometry)
        rc = orbm_create_new_map_points_kb8(neighbours_matcher(), &A.k, &GA.g, pKF1->mfScaleFactor, rig ? pKF1->NLeft : -1, K, tab.data(), gtab.data(),
                                            n_left2.data(), ep.data(), &cams1[0][0], cams2.data(), T12.data(), skip.data(), bCoarse ? 1 : 0,
                                            bFarPoints ? 1 : 0, thFarPoints, points.data(), N1, NULL, matches12.data(), nmatches.data());
      else
        rc = orbm_search_for_triangulation_kb8_neighbours(neighbours_matcher(), &A.k, rig ? pKF1->NLeft : -1, K, tab.data(), n_left2.data(), ep.data(),
                                                          &cams1[0][0], cams2.data(), T12.data(), skip.data(), 0, bCoarse ? 1 : 0, matches12.data(),
                                                          nmatches.data());
    }
    if (rc < 0) throw std::runtime_error(std::string("LocalMapping::CreateNewMapPoints (liborbhip): ") + orbm_last_error(neighbours_matcher()));
    batched = true;
    if (geometry) {   // rc = the number of new points; the list is ordered by neighbour
      points.resize((size_t)rc);
      for (size_t p = 0; p < points.size(); p++) first_of[(size_t)points[p].neighbour + 1]++;
      for (int i = 0; i < K; i++) first_of[(size_t)i + 1] += first_of[(size_t)i];
      listed = true;
    }
  }

  // geometry form: true when the list exists (one camera model throughout); otherwise use matched_indices() and the reference's own body
  bool has_new_points() const { return listed; }
  // the new map points of neighbour i, in ascending idx1: what the body of the loop (:605-880) accepts in iteration i
  const orbm_new_point_t *new_points_begin(size_t i) const { return points.data() + first_of[i]; }
  const orbm_new_point_t *new_points_end(size_t i) const { return points.data() + first_of[i + 1]; }
  static cv::Mat x3D(const orbm_new_point_t &p) {
    cv::Mat x(3, 1, CV_32F);
    for (int r = 0; r < 3; r++) x.at<float>(r) = p.x3D[r];
    return x;
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
