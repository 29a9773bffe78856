// LoopClosing_SearchAndFuse_hip.cc -- drop-in bodies of both overloads of void LoopClosing::SearchAndFuse(...), replacing
// src/LoopClosing.cc:2631-2707, with ONE search for all corrected keyframes in front of the loop (orbm_fuse_sim3_keyframes) instead of
// one ORBmatcher::Fuse(pKF, Scw, vpMapPoints, 4, vpReplacePoints) call - one upload of the same loop / merge points, one host loop over
// them, one synchronisation - per keyframe.
//
// LoopClosing.cc holds the whole LoopClosing class, so these members cannot be swapped by exchanging a translation unit: delete (or
// #if 0) lines 2631-2707 of src/LoopClosing.cc and add this file to the library's sources.  The callers - CorrectLoop
// (:1376) and the two map merges (:1995, :2506) - stay as they are.
//
// Why the searches may be made before the loop although its body changes map points between them - the SEARCH-AND-FUSE RULE of
// include/orbhip.h: the search reads of a keyframe only what the loop never writes and is claimless; of a point it reads isBad(),
// membership in pKF->GetMapPoints(), position, normal, the two distances and the descriptor.  Inside iteration t only AddObservation /
// AddMapPoint run; every Replace is deferred to after the search of t and makes the SEARCHED point the survivor, so validity only
// shrinks (and is tested live here, with the snapshot of GetMapPoints() the reference takes at entry of each Fuse call) and only
// the survivor's ComputeDistinctiveDescriptors() can change a searched quantity.  So iteration t compares every still-valid point's
// GetDescriptor() with the 32 bytes that were uploaded and repeats the search of target t, with orbm_fuse_sim3_cam, for the points that
// differ.  How many points differ on real sequences is not known; each costs one entry of a per-target call, and here every successful
// Replace can make one.
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <list>   // Map.h names std::list without including it
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "LoopClosing.h"
#include "Converter.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "orbhip.h"

namespace ORB_SLAM3 {

namespace {
orbm_t *search_and_fuse_matcher() {   // one handle per thread, as in ORBmatcher_hip.cc
  thread_local orbm_t *m = nullptr;
  if (!m) {
    const char *e = std::getenv("ORBHIP_DEVICE");
    m = orbm_create(e ? std::atoi(e) : 0);
    if (!m) throw std::runtime_error("LoopClosing::SearchAndFuse: orbm_create failed (no usable HIP device; there is no CPU fallback)");
  }
  return m;
}

// The raw mfMaxDistance / mfMinDistance of a MapPoint (MapPointRaw of ORBmatcher_hip.cc: the getters only expose them scaled)
struct LoopPointRaw : MapPoint {
  static float MapPoint::*max_distance() { return &LoopPointRaw::mfMaxDistance; }
  static float MapPoint::*min_distance() { return &LoopPointRaw::mfMinDistance; }
  static std::mutex MapPoint::*mutex_pos() { return &LoopPointRaw::mMutexPos; }
};

// One corrected keyframe, flattened as ORBmatcher::Fuse(pKF, Scw, ...) flattens it (ORBmatcher_hip.cc)
struct FlatSim3Target {
  KeyFrame *pKF;
  float S[16];
  std::vector<float> params;
  orbm_fuse_sim3_target_t g;
  FlatSim3Target(KeyFrame *kf, const cv::Mat &Scw) : pKF(kf) {
    std::memset(&g, 0, sizeof(g));
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) S[4 * r + c] = Scw.at<float>(r, c);
    g.cam_type = (int32_t)pKF->mpCamera->GetType();
    params.resize(g.cam_type == 0 ? 4 : 8);
    for (size_t k = 0; k < params.size(); k++) params[k] = pKF->mpCamera->getParameter((int)k);
  }
  void bind() {   // after the object has reached its final address
    orbm_frame_t &f = g.kf;
    f.n = (int)pKF->mvKeysUn.size();
    f.keys_un = reinterpret_cast<const orbx_keypoint_t *>(pKF->mvKeysUn.data());
    f.descriptors = pKF->mDescriptors.data;
    f.u_right = NULL;   // the Sim3 overload has no stereo term
    f.min_x = (float)pKF->mnMinX; f.max_x = (float)pKF->mnMaxX; f.min_y = (float)pKF->mnMinY; f.max_y = (float)pKF->mnMaxY;
    g.scale_factors = pKF->mvScaleFactors.data();
    g.nlevels = (int32_t)pKF->mvScaleFactors.size();
    g.log_scale_factor = pKF->mfLogScaleFactor;
    g.Scw = S; g.cam_params = params.data();
  }
};

// The loop of either overload: every search in front of it, then per keyframe the dirty test, ORBmatcher.cc:1768-1782 and the
// deferred Replace loop (LoopClosing.cc:2651-2665)
struct LoopFusion {
  std::vector<MapPoint *> &vpMapPoints;
  float th;
  std::vector<FlatSim3Target> targets;
  std::vector<uint8_t> desc;               // [nP][32]: the descriptors that were uploaded
  std::vector<float> Xw, normal, dmax, dmin;
  std::vector<int32_t> best_idx, best_dist;   // [T][nP]
  size_t nP;

  LoopFusion(std::vector<MapPoint *> &points, float th_) : vpMapPoints(points), th(th_), nP(points.size()) {}

  void add(KeyFrame *pKF, const cv::Mat &Scw) { targets.push_back(FlatSim3Target(pKF, Scw)); }

  void flatten(size_t i, MapPoint *pMP) {
    cv::Mat P = pMP->GetWorldPos(), N = pMP->GetNormal();
    for (int r = 0; r < 3; r++) { Xw[3 * i + r] = P.at<float>(r); normal[3 * i + r] = N.at<float>(r); }
    std::memcpy(&desc[32 * i], pMP->GetDescriptor().ptr<uint8_t>(), 32);
    std::unique_lock<std::mutex> lock(pMP->*LoopPointRaw::mutex_pos());
    dmax[i] = pMP->*LoopPointRaw::max_distance();
    dmin[i] = pMP->*LoopPointRaw::min_distance();
  }

  void search() {   // the ONE call
    const size_t T = targets.size();
    std::vector<orbm_fuse_sim3_target_t> tab(T);
    for (size_t t = 0; t < T; t++) { targets[t].bind(); tab[t] = targets[t].g; }
    const size_t n1 = nP > 0 ? nP : 1;
    desc.assign(n1 * 32, 0); Xw.assign(n1 * 3, 0.f); normal.assign(n1 * 3, 0.f); dmax.assign(n1, 0.f); dmin.assign(n1, 0.f);
    std::vector<uint8_t> live(n1, 0);
    for (size_t i = 0; i < nP; i++) {
      MapPoint *pMP = vpMapPoints[i];
      if (pMP->isBad()) continue;                                                   // ORBmatcher.cc:1692
      live[i] = 1;
      flatten(i, pMP);
    }
    std::vector<uint8_t> valid((T > 0 ? T : 1) * n1, 0);
    for (size_t t = 0; t < T; t++) {
      const std::set<MapPoint *> spAlreadyFound = targets[t].pKF->GetMapPoints();   // :1680
      for (size_t i = 0; i < nP; i++) valid[t * nP + i] = live[i] && !spAlreadyFound.count(vpMapPoints[i]);
    }
    best_idx.assign((T > 0 ? T : 1) * n1, -1);
    best_dist.assign((T > 0 ? T : 1) * n1, 256);
    std::vector<int32_t> nfused(T > 0 ? T : 1, 0);
    const int rc = orbm_fuse_sim3_keyframes(search_and_fuse_matcher(), (int)T, tab.data(), (int)nP, valid.data(), Xw.data(), normal.data(), desc.data(),
                                            dmax.data(), dmin.data(), th, best_idx.data(), best_dist.data(), nfused.data());
    if (rc < 0) throw std::runtime_error(std::string("LoopClosing::SearchAndFuse (liborbhip): ") + orbm_last_error(search_and_fuse_matcher()));
  }

  // matcher.Fuse(pKF_t, Scw_t, vpMapPoints, th, vpReplacePoints) on the live objects; returns nFused
  int fuse(size_t t, std::vector<MapPoint *> &vpReplacePoints) {
    FlatSim3Target &G = targets[t];
    KeyFrame *pKF = G.pKF;
    int32_t *row = &best_idx[t * nP];
    const std::set<MapPoint *> spAlreadyFound = pKF->GetMapPoints();                // :1680
    std::vector<uint8_t> valid(nP > 0 ? nP : 1, 0), dirty(nP > 0 ? nP : 1, 0), now;
    bool any = false;
    for (size_t j = 0; j < nP; j++) {
      MapPoint *pMP = vpMapPoints[j];
      if (pMP->isBad() || spAlreadyFound.count(pMP)) continue;                      // :1692
      valid[j] = 1;
      // the SEARCH-AND-FUSE RULE's exception: still valid for this target, and the descriptor is no longer the uploaded one
      cv::Mat d = pMP->GetDescriptor();
      if (std::memcmp(d.ptr<uint8_t>(), &desc[32 * j], 32) == 0) continue;
      if (!any) { now = desc; any = true; }
      std::memcpy(&now[32 * j], d.ptr<uint8_t>(), 32);
      dirty[j] = 1;
    }
    if (any) {
      std::vector<int32_t> bi(nP, -1), bd(nP, 256);
      const int rc = orbm_fuse_sim3_cam(search_and_fuse_matcher(), &G.g.kf, G.g.scale_factors, G.g.nlevels, G.g.log_scale_factor, (int)nP, dirty.data(),
                                        Xw.data(), normal.data(), now.data(), dmax.data(), dmin.data(), G.S, G.g.cam_type, G.params.data(), th, bi.data(),
                                        bd.data());
      if (rc < 0) throw std::runtime_error(std::string("LoopClosing::SearchAndFuse (liborbhip): ") + orbm_last_error(search_and_fuse_matcher()));
      for (size_t j = 0; j < nP; j++)
        if (dirty[j]) row[j] = bi[j];
    }
    int nFused = 0;
    for (size_t j = 0; j < nP; j++) {                                               // :1768-1782, on the live objects, in order
      if (!valid[j] || row[j] < 0) continue;
      MapPoint *pMP = vpMapPoints[j];
      MapPoint *pMPinKF = pKF->GetMapPoint(row[j]);
      if (pMPinKF) {
        if (!pMPinKF->isBad()) vpReplacePoints[j] = pMPinKF;
      } else {
        pMP->AddObservation(pKF, row[j]);
        pKF->AddMapPoint(pMP, row[j]);
      }
      nFused++;
    }
    return nFused;
  }

  // LoopClosing.cc:2648-2665 / :2688-2702 for target t; returns num_replaces
  int fuse_and_replace(size_t t) {
    KeyFrame *pKF = targets[t].pKF;
    Map *pMap = pKF->GetMap();
    std::vector<MapPoint *> vpReplacePoints(vpMapPoints.size(), static_cast<MapPoint *>(NULL));
    fuse(t, vpReplacePoints);
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);   // Get Map Mutex
    int num_replaces = 0;
    const int nLP = (int)vpMapPoints.size();
    for (int i = 0; i < nLP; i++) {
      MapPoint *pRep = vpReplacePoints[i];
      if (pRep) {
        num_replaces += 1;
        pRep->Replace(vpMapPoints[i]);
      }
    }
    return num_replaces;
  }
};
}  // namespace

void LoopClosing::SearchAndFuse(const KeyFrameAndPose &CorrectedPosesMap, vector<MapPoint *> &vpMapPoints) {
  int total_replaces = 0;
  cout << "FUSE: Initially there are " << vpMapPoints.size() << " MPs" << endl;
  cout << "FUSE: Intially there are " << CorrectedPosesMap.size() << " KFs" << endl;
  LoopFusion fusion(vpMapPoints, 4);
  for (KeyFrameAndPose::const_iterator mit = CorrectedPosesMap.begin(), mend = CorrectedPosesMap.end(); mit != mend; mit++) {
    g2o::Sim3 g2oScw = mit->second;
    fusion.add(mit->first, Converter::toCvMat(g2oScw));                             // :2642-2646, the std::map's order
  }
  fusion.search();
  for (size_t t = 0; t < fusion.targets.size(); t++) total_replaces += fusion.fuse_and_replace(t);
  cout << "FUSE: " << total_replaces << " MPs had been fused" << endl;
}

void LoopClosing::SearchAndFuse(const vector<KeyFrame *> &vConectedKFs, vector<MapPoint *> &vpMapPoints) {
  int total_replaces = 0;
  cout << "FUSE-POSE: Initially there are " << vpMapPoints.size() << " MPs" << endl;
  cout << "FUSE-POSE: Intially there are " << vConectedKFs.size() << " KFs" << endl;
  LoopFusion fusion(vpMapPoints, 4);
  for (auto mit = vConectedKFs.begin(), mend = vConectedKFs.end(); mit != mend; mit++) fusion.add(*mit, (*mit)->GetPose());   // :2684-2686
  fusion.search();
  for (size_t t = 0; t < fusion.targets.size(); t++) {
    const int num_replaces = fusion.fuse_and_replace(t);
    cout << "FUSE-POSE: KF " << fusion.targets[t].pKF->mnId << " ->" << num_replaces << " MPs fused" << endl;
    total_replaces += num_replaces;
  }
  cout << "FUSE-POSE: " << total_replaces << " MPs had been fused" << endl;
}

}  // namespace ORB_SLAM3
