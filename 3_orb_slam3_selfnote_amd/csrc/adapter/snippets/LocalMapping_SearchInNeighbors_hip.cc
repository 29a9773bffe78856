// LocalMapping_SearchInNeighbors_hip.cc -- the two Fuse steps of void LocalMapping::SearchInNeighbors() (src/LocalMapping.cc:983-1035)
// with ONE search for all target keyframes in front of the loop (orbm_fuse_keyframes) instead of one ORBmatcher::Fuse call - one
// upload of the same points, one host loop, one synchronisation - per target and camera.
//
// A helper class, not a member of ORBmatcher.  Add this file to the library's sources and make two edits in src/LocalMapping.cc
// (INTEGRATION.md):
//   1. the forward loop (:989-1000) becomes
//        NeighbourFusion fusion(vpTargetKFs, vpMapPointMatches);
//        for (size_t i = 0; i < vpTargetKFs.size(); i++) fusion.fuse(i);
//   2. the reverse step (:1033-1035) becomes
//        NeighbourFusion back(std::vector<KeyFrame *>(1, mpCurrentKeyFrame), vpFuseCandidates);
//        back.fuse(0);
// fuse(i) does for target keyframe i - both cameras of a rig, left then right - what ORBmatcher::Fuse (ORBmatcher_hip.cc) does on the
// live objects: the reference's own test `!isBad() && !IsInKeyFrame(pKF)` in front of every entry, then :1625-1645.
//
// Why the searches may be made before the loop although its body (Replace / AddObservation) changes map points between them - the
// FUSE RULE of include/orbhip.h: the search reads of a keyframe only what the loop never writes and is claimless; of a point it reads
// isBad(), IsInKeyFrame(pKF), position, normal, the two distances and the descriptor.  The body leaves position, normal and distances
// alone, validity only shrinks (and is tested live here), and only MapPoint::Replace's ComputeDistinctiveDescriptors() can change a
// descriptor - the survivor's, which may be the searched point or the keyframe's own point, and that one may sit anywhere in the list.
// So fuse(i) compares every still-valid point's GetDescriptor() with the 32 bytes that were uploaded (by content, not by index) and
// repeats the search of target i, with orbm_fuse, for the points that differ - before its first entry, which is early enough: a point
// that iteration i changes is in pKF_i afterwards.  The two targets of a rig keyframe are consecutive and the test runs for each.
// How many points differ on real sequences is not known; each costs one entry of a per-target call.
#include <cstdlib>
#include <cstring>
#include <list>   // Map.h names std::list without including it
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "LocalMapping.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "ORBmatcher.h"
#include "orbhip.h"

namespace ORB_SLAM3 {

namespace {
orbm_t *fusion_matcher() {   // one handle per thread, as in ORBmatcher_hip.cc
  thread_local orbm_t *m = nullptr;
  if (!m) {
    const char *e = std::getenv("ORBHIP_DEVICE");
    m = orbm_create(e ? std::atoi(e) : 0);
    if (!m) throw std::runtime_error("LocalMapping::SearchInNeighbors: orbm_create failed (no usable HIP device; there is no CPU fallback)");
  }
  return m;
}

// The raw mfMaxDistance / mfMinDistance of a MapPoint (MapPointRaw of ORBmatcher_hip.cc: the getters only expose them scaled)
struct FusionPointRaw : MapPoint {
  static float MapPoint::*max_distance() { return &FusionPointRaw::mfMaxDistance; }
  static float MapPoint::*min_distance() { return &FusionPointRaw::mfMinDistance; }
  static std::mutex MapPoint::*mutex_pos() { return &FusionPointRaw::mMutexPos; }
};

// One target of the call: one camera of one keyframe, flattened as ORBmatcher::Fuse flattens it (ORBmatcher_hip.cc)
struct FlatFuseTarget {
  KeyFrame *pKF;
  bool bRight;
  int shift;            // NLeft for the right camera: added to the matched index (ORBmatcher.cc:1608)
  float T[16], Ow[3];
  std::vector<float> params;
  orbm_fuse_target_t g;
  FlatFuseTarget(KeyFrame *kf, bool right) : pKF(kf), bRight(right), shift(right ? kf->NLeft : 0) {
    std::memset(&g, 0, sizeof(g));
    cv::Mat Rcw = bRight ? pKF->GetRightRotation() : pKF->GetRotation();            // :1431-1444
    cv::Mat tcw = bRight ? pKF->GetRightTranslation() : pKF->GetTranslation();
    cv::Mat O = bRight ? pKF->GetRightCameraCenter() : pKF->GetCameraCenter();
    std::memset(T, 0, sizeof(T));
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) T[4 * r + c] = Rcw.at<float>(r, c); T[4 * r + 3] = tcw.at<float>(r); Ow[r] = O.at<float>(r); }
    T[15] = 1.f;
    GeometricCamera *pCamera = bRight ? pKF->mpCamera2 : pKF->mpCamera;
    g.cam_type = (int32_t)pCamera->GetType();
    params.resize(g.cam_type == 0 ? 4 : 8);
    for (size_t k = 0; k < params.size(); k++) params[k] = pCamera->getParameter((int)k);
  }
  void bind() {   // after the object has reached its final address
    orbm_frame_t &f = g.kf;
    f.n = (int)pKF->mvKeysUn.size();
    f.keys_un = reinterpret_cast<const orbx_keypoint_t *>(pKF->mvKeysUn.data());
    f.descriptors = pKF->mDescriptors.data;
    f.u_right = pKF->mvuRight.empty() ? NULL : pKF->mvuRight.data();
    f.min_x = (float)pKF->mnMinX; f.max_x = (float)pKF->mnMaxX; f.min_y = (float)pKF->mnMinY; f.max_y = (float)pKF->mnMaxY;
    if (pKF->NLeft != -1) {   // rigs: the raw keypoints of the chosen image, the descriptor rows behind NLeft (:1569-1571, :1608)
      const std::vector<cv::KeyPoint> &keys = bRight ? pKF->mvKeysRight : pKF->mvKeys;
      f.n = (int)keys.size();
      f.keys_un = reinterpret_cast<const orbx_keypoint_t *>(keys.data());
      f.descriptors = pKF->mDescriptors.data + (size_t)shift * 32;
    }
    g.scale_factors = pKF->mvScaleFactors.data();
    g.inv_level_sigma2 = pKF->mvInvLevelSigma2.data();
    g.nlevels = (int32_t)pKF->mvScaleFactors.size();
    g.log_scale_factor = pKF->mfLogScaleFactor;
    g.Tcw = T; g.Ow = Ow; g.cam_params = params.data();
    g.bf = pKF->mbf;
  }
};
}  // namespace

struct NeighbourFusion {
  std::vector<KeyFrame *> vpTargetKFs;
  std::vector<MapPoint *> vpMapPoints;
  float th;
  std::vector<FlatFuseTarget> targets;     // one per camera: a rig keyframe contributes (left, right), consecutive
  std::vector<size_t> first_of;            // [K + 1]: the targets of keyframe i are targets[first_of[i] .. first_of[i + 1])
  std::vector<uint8_t> desc;               // [nP][32]: the descriptors that were uploaded
  std::vector<float> Xw, normal, dmax, dmin;
  std::vector<int32_t> best_idx, best_dist;   // [T][nP]
  size_t nP;

  NeighbourFusion(const std::vector<KeyFrame *> &vpKFs, const std::vector<MapPoint *> &points, float th_ = 3.0f)
      : vpTargetKFs(vpKFs), vpMapPoints(points), th(th_), first_of(vpKFs.size() + 1, 0), nP(points.size()) {
    for (size_t i = 0; i < vpTargetKFs.size(); i++) {
      first_of[i] = targets.size();
      targets.push_back(FlatFuseTarget(vpTargetKFs[i], false));
      if (vpTargetKFs[i]->NLeft != -1) targets.push_back(FlatFuseTarget(vpTargetKFs[i], true));
    }
    first_of[vpTargetKFs.size()] = targets.size();
    const size_t T = targets.size();
    std::vector<orbm_fuse_target_t> tab(T);
    for (size_t t = 0; t < T; t++) { targets[t].bind(); tab[t] = targets[t].g; }
    const size_t n1 = nP > 0 ? nP : 1;
    desc.assign(n1 * 32, 0); Xw.assign(n1 * 3, 0.f); normal.assign(n1 * 3, 0.f); dmax.assign(n1, 0.f); dmin.assign(n1, 0.f);
    std::vector<uint8_t> live(n1, 0);
    for (size_t i = 0; i < nP; i++) {
      MapPoint *pMP = vpMapPoints[i];
      if (!pMP || pMP->isBad()) continue;                                           // :1464-1477
      live[i] = 1;
      flatten(i, pMP);
    }
    std::vector<uint8_t> valid((T > 0 ? T : 1) * n1, 0);
    for (size_t t = 0; t < T; t++)
      for (size_t i = 0; i < nP; i++) valid[t * nP + i] = live[i] && !vpMapPoints[i]->IsInKeyFrame(targets[t].pKF);   // :1479
    best_idx.assign((T > 0 ? T : 1) * n1, -1);
    best_dist.assign((T > 0 ? T : 1) * n1, 256);
    std::vector<int32_t> nfused(T > 0 ? T : 1, 0);
    const int rc = orbm_fuse_keyframes(fusion_matcher(), (int)T, tab.data(), (int)nP, valid.data(), Xw.data(), normal.data(), desc.data(), dmax.data(),
                                       dmin.data(), th, best_idx.data(), best_dist.data(), nfused.data());
    if (rc < 0) throw std::runtime_error(std::string("LocalMapping::SearchInNeighbors (liborbhip): ") + orbm_last_error(fusion_matcher()));
  }

  void flatten(size_t i, MapPoint *pMP) {
    cv::Mat P = pMP->GetWorldPos(), N = pMP->GetNormal();
    for (int r = 0; r < 3; r++) { Xw[3 * i + r] = P.at<float>(r); normal[3 * i + r] = N.at<float>(r); }
    std::memcpy(&desc[32 * i], pMP->GetDescriptor().ptr<uint8_t>(), 32);
    std::unique_lock<std::mutex> lock(pMP->*FusionPointRaw::mutex_pos());
    dmax[i] = pMP->*FusionPointRaw::max_distance();
    dmin[i] = pMP->*FusionPointRaw::min_distance();
  }

  // matcher.Fuse(vpTargetKFs[i], vpMapPoints) and, for a rig, matcher.Fuse(vpTargetKFs[i], vpMapPoints, true); returns the sum of nFused
  int fuse(size_t i) {
    int nFused = 0;
    for (size_t t = first_of[i]; t < first_of[i + 1]; t++) nFused += fuse_target(t);
    return nFused;
  }

  int fuse_target(size_t t) {
    FlatFuseTarget &G = targets[t];
    KeyFrame *pKF = G.pKF;
    int32_t *row = &best_idx[t * nP];
    // the FUSE RULE's exception: points that are still valid for this target and whose descriptor is no longer the uploaded one
    std::vector<uint8_t> dirty(nP > 0 ? nP : 1, 0), now;
    bool any = false;
    for (size_t j = 0; j < nP; j++) {
      MapPoint *pMP = vpMapPoints[j];
      if (!pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
      cv::Mat d = pMP->GetDescriptor();
      if (std::memcmp(d.ptr<uint8_t>(), &desc[32 * j], 32) == 0) continue;
      if (!any) { now = desc; any = true; }
      std::memcpy(&now[32 * j], d.ptr<uint8_t>(), 32);
      dirty[j] = 1;
    }
    if (any) {
      std::vector<int32_t> bi(nP, -1), bd(nP, 256);
      const int rc = orbm_fuse(fusion_matcher(), &G.g.kf, G.g.scale_factors, G.g.inv_level_sigma2, G.g.nlevels, G.g.log_scale_factor, (int)nP, dirty.data(),
                               Xw.data(), normal.data(), now.data(), dmax.data(), dmin.data(), G.T, G.Ow, G.g.cam_type, G.params.data(), G.g.bf, th, bi.data(),
                               bd.data());
      if (rc < 0) throw std::runtime_error(std::string("LocalMapping::SearchInNeighbors (liborbhip): ") + orbm_last_error(fusion_matcher()));
      for (size_t j = 0; j < nP; j++)
        if (dirty[j]) row[j] = bi[j];
    }
    int nFused = 0;
    for (size_t j = 0; j < nP; j++) {                                               // :1625-1645, on the live objects, in order
      if (row[j] < 0) continue;
      MapPoint *pMP = vpMapPoints[j];
      if (!pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;                 // the reference's own live test (:1464-1483)
      const int bestIdx = row[j] + G.shift;
      MapPoint *pMPinKF = pKF->GetMapPoint(bestIdx);
      if (pMPinKF) {
        if (!pMPinKF->isBad()) {
          if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
          else pMPinKF->Replace(pMP);
        }
      } else {
        pMP->AddObservation(pKF, bestIdx);
        pKF->AddMapPoint(pMP, bestIdx);
      }
      nFused++;
    }
    return nFused;
  }
};

}  // namespace ORB_SLAM3
