// Tracking_UpdateLocalMap_hip.cc -- void Tracking::UpdateLocalKeyFrames() and void Tracking::UpdateLocalPoints()
// (src/Tracking.cc:3590-3762, :3559-3587) from the device: the vote, the first list, the expansion, the temporal tail and the local
// points are one orbm_update_local_map call.  The two bodies below replace the reference's; UpdateLocalMap() (:3542-3553) stays as it
// is and calls them one after the other.  Add this file to the library's sources and remove the two bodies from src/Tracking.cc
// (INTEGRATION.md).
//
// What is flattened per frame is what the call can read, not the map: the frame's map points with their observations; the keyframes
// that observe them (the voted ones) with their ten best covisibles, children and parent; the chain of mPrevKF from mpLastKeyFrame; and
// of every one of these keyframes its rows (mvpMapPoints) with isBad() of the points.  Observations of points that are not in the frame
// are never read by either member and are passed as empty lists.  kf_rank is the order of the keyframes' addresses (RANK RULE,
// include/orbhip.h); the stamps are written back on the live objects (STAMP NOTE).  A system that keeps the tables resident on the device
// calls orbm_update_local_map_device and orbm_gather_local_map_device instead and uploads only what local mapping changed.
//
// THE SNAPSHOT.  isBad(), the observations, the covisibility lists, children, parents and rows are read once, while flattening; the
// reference reads them as its loops reach them.  Local mapping can add a keyframe, erase an observation or set a point bad meanwhile: a
// difference in time, as for the other batch snippets.  UpdateLocalPoints tests isBad() of every point again when it writes the list,
// so a point that turned bad after the snapshot is not handed on; a keyframe that turned bad after the snapshot stays in
// mvpLocalKeyFrames for this frame, as it would have had the reference passed it a moment earlier.
#include <algorithm>
#include <cstdlib>
#include <list>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "Tracking.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "orbhip.h"

namespace ORB_SLAM3 {

namespace {
orbm_t *local_map_matcher() {   // one handle per thread, as in ORBmatcher_hip.cc
  thread_local orbm_t *m = nullptr;
  if (!m) {
    const char *e = std::getenv("ORBHIP_DEVICE");
    m = orbm_create(e ? std::atoi(e) : 0);
    if (!m) throw std::runtime_error("Tracking::UpdateLocalMap: orbm_create failed (no usable HIP device; there is no CPU fallback)");
  }
  return m;
}

// what UpdateLocalKeyFrames leaves for UpdateLocalPoints, which UpdateLocalMap calls next on the same thread
thread_local std::vector<MapPoint *> tLocalPoints;

struct LocalMapTables {
  std::vector<KeyFrame *> kfs;
  std::vector<MapPoint *> pts;
  std::map<KeyFrame *, int> kfIndex;
  std::map<MapPoint *, int> ptIndex;
  std::vector<std::vector<int32_t> > obs;   // per point; filled for the frame's points only
  int kf(KeyFrame *pKF) {
    const std::map<KeyFrame *, int>::iterator it = kfIndex.find(pKF);
    if (it != kfIndex.end()) return it->second;
    kfIndex[pKF] = (int)kfs.size();
    kfs.push_back(pKF);
    return (int)kfs.size() - 1;
  }
  int pt(MapPoint *pMP) {
    const std::map<MapPoint *, int>::iterator it = ptIndex.find(pMP);
    if (it != ptIndex.end()) return it->second;
    ptIndex[pMP] = (int)pts.size();
    pts.push_back(pMP);
    obs.push_back(std::vector<int32_t>());
    return (int)pts.size() - 1;
  }
};
}  // namespace

void Tracking::UpdateLocalKeyFrames() {
  // the frame that votes (:3596-3646)
  const bool bCurrent = !mpAtlas->isImuInitialized() || (mCurrentFrame.mnId < mnLastRelocFrameId + 2);
  Frame &F = bCurrent ? mCurrentFrame : mLastFrame;
  const bool bInertial = mSensor == System::IMU_MONOCULAR || mSensor == System::IMU_STEREO;   // :3737
  LocalMapTables T;
  std::vector<int32_t> framePoint(F.N > 0 ? F.N : 1, -1);
  std::vector<uint8_t> ptBad;
  for (int i = 0; i < F.N; i++) {
    MapPoint *pMP = F.mvpMapPoints[i];
    if (!pMP) continue;
    const bool known = T.ptIndex.count(pMP) != 0;
    const int p = T.pt(pMP);
    framePoint[i] = p;
    if (known) continue;
    ptBad.push_back(pMP->isBad() ? 1 : 0);
    if (ptBad.back()) continue;
    const std::map<KeyFrame *, std::tuple<int, int> > observations = pMP->GetObservations();
    for (std::map<KeyFrame *, std::tuple<int, int> >::const_iterator it = observations.begin(), itend = observations.end(); it != itend; it++)
      T.obs[p].push_back(T.kf(it->first));
  }
  // the surroundings of the voted keyframes, and the temporal chain
  const size_t nVoted = T.kfs.size();
  std::vector<int32_t> best(nVoted * ORBM_MAP_BEST, -1), childStart(1, 0), child, parent;
  for (size_t g = 0; g < nVoted; g++) {
    KeyFrame *pKF = T.kfs[g];
    const std::vector<KeyFrame *> vNeighs = pKF->GetBestCovisibilityKeyFrames(10);
    for (size_t j = 0; j < vNeighs.size() && j < ORBM_MAP_BEST; j++) best[g * ORBM_MAP_BEST + j] = T.kf(vNeighs[j]);
    const std::set<KeyFrame *> spChilds = pKF->GetChilds();   // std::set iterates in address order: ascending rank
    for (std::set<KeyFrame *>::const_iterator sit = spChilds.begin(), send = spChilds.end(); sit != send; sit++) child.push_back(T.kf(*sit));
    childStart.push_back((int32_t)child.size());
    KeyFrame *pParent = pKF->GetParent();
    parent.push_back(pParent ? T.kf(pParent) : -1);
  }
  int lastKF = -1;
  if (bInertial) {
    KeyFrame *temp = mCurrentFrame.mpLastKeyFrame;
    if (temp) lastKF = T.kf(temp);
    for (int i = 0; i < 20 && temp; i++) { temp = temp->mPrevKF; if (temp) T.kf(temp); }
  }
  const int G = (int)T.kfs.size();
  best.resize((size_t)G * ORBM_MAP_BEST, -1);
  childStart.resize((size_t)G + 1, (int32_t)child.size());
  parent.resize((size_t)G, -1);
  std::vector<int32_t> rank(G), map(G, 0), prev(G, -1), rowStart(1, 0), rowPoint;
  std::vector<uint8_t> kfBad(G);
  std::vector<KeyFrame *> byAddress(T.kfs);
  std::sort(byAddress.begin(), byAddress.end(), std::less<KeyFrame *>());
  for (int r = 0; r < G; r++) rank[T.kfIndex[byAddress[r]]] = r;
  for (int g = 0; g < G; g++) {
    KeyFrame *pKF = T.kfs[g];
    kfBad[g] = pKF->isBad() ? 1 : 0;
    if (pKF->mPrevKF) { const std::map<KeyFrame *, int>::const_iterator it = T.kfIndex.find(pKF->mPrevKF); if (it != T.kfIndex.end()) prev[g] = it->second; }
    const std::vector<MapPoint *> vpMPs = pKF->GetMapPointMatches();
    for (size_t i = 0; i < vpMPs.size(); i++) {
      MapPoint *pMP = vpMPs[i];
      if (!pMP) { rowPoint.push_back(-1); continue; }
      const bool known = T.ptIndex.count(pMP) != 0;
      rowPoint.push_back(T.pt(pMP));
      if (!known) ptBad.push_back(pMP->isBad() ? 1 : 0);
    }
    rowStart.push_back((int32_t)rowPoint.size());
  }
  const int P = (int)T.pts.size();
  std::vector<int32_t> obsStart(1, 0), obsKF;
  for (int p = 0; p < P; p++) { obsKF.insert(obsKF.end(), T.obs[p].begin(), T.obs[p].end()); obsStart.push_back((int32_t)obsKF.size()); }
  orbm_map_graph_t graph;
  graph.G = G; graph.kf_rank = rank.data(); graph.kf_bad = kfBad.data(); graph.kf_map = map.data();
  graph.kf_row_start = rowStart.data(); graph.row_point = rowPoint.data(); graph.kf_best = best.data();
  graph.kf_child_start = childStart.data(); graph.kf_child = child.data(); graph.kf_parent = parent.data(); graph.kf_prev = prev.data();
  graph.P = P; graph.pt_bad = ptBad.data(); graph.obs_start = obsStart.data(); graph.obs_kf = obsKF.data();

  std::vector<int32_t> localKF(G + 24), localPoint(P > 0 ? P : 1);
  std::vector<uint8_t> slotBad(F.N > 0 ? F.N : 1, 0);
  int32_t nLocalKF = 0, nLocalPoint = 0, kfMax = -1, maxVotes = 0;
  if (orbm_update_local_map(local_map_matcher(), &graph, F.N, framePoint.data(), bInertial ? 1 : 0, lastKF, G + 24, P, localKF.data(), &nLocalKF, &kfMax,
                            &maxVotes, slotBad.data(), localPoint.data(), &nLocalPoint) < 0)
    throw std::runtime_error(std::string("Tracking::UpdateLocalMap: ") + orbm_last_error(local_map_matcher()));

  for (int i = 0; i < F.N; i++)
    if (slotBad[i]) F.mvpMapPoints[i] = NULL;                       // :3616, :3642
  mvpLocalKeyFrames.clear();
  mvpLocalKeyFrames.reserve(nLocalKF);
  for (int j = 0; j < nLocalKF; j++) {
    KeyFrame *pKF = T.kfs[localKF[j]];
    mvpLocalKeyFrames.push_back(pKF);
    pKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;             // :3674, :3701, :3716, :3729, :3750
  }
  if (kfMax >= 0) {                                                 // :3757-3761
    mpReferenceKF = T.kfs[kfMax];
    mCurrentFrame.mpReferenceKF = mpReferenceKF;
  }
  tLocalPoints.clear();
  for (int j = 0; j < nLocalPoint; j++) tLocalPoints.push_back(T.pts[localPoint[j]]);
}

void Tracking::UpdateLocalPoints() {
  mvpLocalMapPoints.clear();
  for (size_t j = 0; j < tLocalPoints.size(); j++) {
    MapPoint *pMP = tLocalPoints[j];
    if (pMP->isBad()) continue;                                     // turned bad after the snapshot
    mvpLocalMapPoints.push_back(pMP);
    pMP->mnTrackReferenceForFrame = mCurrentFrame.mnId;             // :3583
  }
  tLocalPoints.clear();
}

}  // namespace ORB_SLAM3
