// SearchByBoW_candidates_hip.h -- what Tracking_Relocalization_hip.cc and LoopClosing_DetectCommonRegionsFromBoW_hip.cc share: a
// keyframe or frame flattened for the one-call SearchByBoW entries of include/orbhip.h, as ORBmatcher::SearchByBoW flattens one pair
// (ORBmatcher_hip.cc), and the handle.
#pragma once
#include <cstdlib>
#include <cstring>
#include <list>   // Map.h names std::list without including it
#include <stdexcept>
#include <string>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "orbhip.h"

namespace ORB_SLAM3 {
namespace bow_candidates {

inline orbm_t *matcher() {   // one handle per thread, as in ORBmatcher_hip.cc
  thread_local orbm_t *m = nullptr;
  if (!m) {
    const char *e = std::getenv("ORBHIP_DEVICE");
    m = orbm_create(e ? std::atoi(e) : 0);
    if (!m) throw std::runtime_error("SearchByBoW: orbm_create failed (no usable HIP device; there is no CPU fallback)");
  }
  return m;
}

inline int checked(int rc, const char *who) {
  if (rc < 0) throw std::runtime_error(std::string(who) + " (liborbhip): " + orbm_last_error(matcher()));
  return rc;
}

// One operand: DBoW2::FeatureVector in key order, the keypoints whose angle the member reads, the map-point flags
struct Flat {
  std::vector<uint32_t> id;
  std::vector<int32_t> start, idx;
  std::vector<uint8_t> has;
  std::vector<cv::KeyPoint> keys;
  orbm_keyframe_t k;
  Flat() { std::memset(&k, 0, sizeof(k)); }

  void nodes(const DBoW2::FeatureVector &fv) {
    start.push_back(0);
    for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) {
      id.push_back(it->first);
      for (size_t j = 0; j < it->second.size(); j++) idx.push_back((int32_t)it->second[j]);
      start.push_back((int32_t)idx.size());
    }
  }
  void bind(int n, const unsigned char *descriptors) {   // after the object has reached its final address
    k.n = n;
    k.keys_un = reinterpret_cast<const orbx_keypoint_t *>(keys.data());
    k.descriptors = descriptors;
    k.has_mappoint = has.data();
    k.n_nodes = (int32_t)id.size();
    k.node_id = id.data(); k.node_start = start.data(); k.node_idx = idx.data();
  }

  // pKF as the FIRST operand of SearchByBoW(pKF, F) (ORBmatcher.cc:273-469): rigs concatenate mvKeys and mvKeysRight (:383-395)
  void keyframe_against_frame(KeyFrame *pKF, const std::vector<MapPoint *> &mps) {
    nodes(pKF->mFeatVec);
    has.resize(pKF->N);
    for (int i = 0; i < pKF->N; i++) has[i] = mps[i] && !mps[i]->isBad();            // :307-313
    if (pKF->mpCamera2) { keys = pKF->mvKeys; keys.insert(keys.end(), pKF->mvKeysRight.begin(), pKF->mvKeysRight.end()); }
    else keys = pKF->mvKeysUn;
    bind(pKF->N, pKF->mDescriptors.data);
  }
  // F as the SECOND operand of SearchByBoW(pKF, F): its map points are not read
  void frame(Frame &F) {
    nodes(F.mFeatVec);
    has.assign(F.N, 0);
    keys = F.mvKeys;                                                                  // the angle of F.mvKeys, :395
    if (F.Nleft != -1) keys.insert(keys.end(), F.mvKeysRight.begin(), F.mvKeysRight.end());
    bind(F.N, F.mDescriptors.data);
  }
  // either operand of SearchByBoW(pKF1, pKF2) (:839-979): the right image's keypoints of a rig never take part (:874-876, :894-896)
  void keyframe_against_keyframe(KeyFrame *pKF, const std::vector<MapPoint *> &mps) {
    nodes(pKF->mFeatVec);
    has.resize(pKF->N);
    const int nUn = (int)pKF->mvKeysUn.size();
    for (int i = 0; i < pKF->N; i++) has[i] = (pKF->NLeft == -1 || i < nUn) && mps[i] && !mps[i]->isBad();
    keys = pKF->mvKeysUn;
    keys.resize(pKF->N);   // rigs: N counts both images, the padding is never read (has_mappoint = 0 there)
    bind(pKF->N, pKF->mDescriptors.data);
  }
};

}  // namespace bow_candidates
}  // namespace ORB_SLAM3
