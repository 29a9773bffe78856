// KeyFrame_UpdateConnections_hip.cc -- void KeyFrame::UpdateConnections(bool) (src/KeyFrame.cc:407-530) for the keyframes of a loop, the
// counting of all of them in one device call (orbm_update_connections).
//
// A helper class, KeyFrameConnections, not a member swap: KeyFrame::UpdateConnections stays in src/KeyFrame.cc for its single calls
// (LocalMapping.cc:400, :1057).  Where the reference calls it in a loop over keyframes whose map state no longer changes inside the loop
// (LoopClosing.cc:1343, :1384-1390, :2007-2020, :2518-2531; Optimizer.cc:2283), make two edits:
//   1. in front of the loop, with the keyframes the loop will visit:
//        KeyFrameConnections conn(vpKeyFrames);
//   2. inside, `pKFi->UpdateConnections();` becomes
//        conn.apply(pKFi);
//
// Why all targets may be counted at loop entry - the CONNECTIONS RULE of include/orbhip.h: KFcounter reads mvpMapPoints, the
// observations, isBad() and GetMap(), and UpdateConnections writes none of them.  What the member WRITES is replayed by apply(pKF) on
// the live objects, in the caller's order: AddConnection on every keyframe at or above the threshold in address order (or on pKFmax
// alone), with the UpdateBestCovisibles re-sort it triggers; the keyframe's own three tables; mpParent / AddChild at the first
// connection.  kf_rank is the order of the keyframes' addresses (RANK RULE).
//
// THE SNAPSHOT.  The rows, observations, isBad() and GetMap() are read once, in the constructor.  A loop that changes map points
// between two of its UpdateConnections calls (LoopClosing.cc:1270-1343 replaces points inside the same iteration) must construct the
// helper after those changes.  apply() of a keyframe that was not given to the constructor throws.
//
// The three tables and mbFirstConnection are protected members of KeyFrame.  The helper reaches them through pointers to members
// formed in a class derived from KeyFrame, which the language allows; no edit of KeyFrame.h is needed.
#include <algorithm>
#include <cstdlib>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "Map.h"
#include "orbhip.h"

namespace ORB_SLAM3 {

namespace {
orbm_t *connections_matcher() {   // one handle per thread, as in ORBmatcher_hip.cc
  thread_local orbm_t *m = nullptr;
  if (!m) {
    const char *e = std::getenv("ORBHIP_DEVICE");
    m = orbm_create(e ? std::atoi(e) : 0);
    if (!m) throw std::runtime_error("KeyFrame::UpdateConnections: orbm_create failed (no usable HIP device; there is no CPU fallback)");
  }
  return m;
}

struct KeyFrameTables : public KeyFrame {   // never constructed: a place to name KeyFrame's protected members
  static std::map<KeyFrame *, int> &weights(KeyFrame *p) { return p->*(&KeyFrameTables::mConnectedKeyFrameWeights); }
  static std::vector<KeyFrame *> &ordered(KeyFrame *p) { return p->*(&KeyFrameTables::mvpOrderedConnectedKeyFrames); }
  static std::vector<int> &orderedWeights(KeyFrame *p) { return p->*(&KeyFrameTables::mvOrderedWeights); }
  static bool &firstConnection(KeyFrame *p) { return p->*(&KeyFrameTables::mbFirstConnection); }
  static KeyFrame *&parent(KeyFrame *p) { return p->*(&KeyFrameTables::mpParent); }
  static std::mutex &mutex(KeyFrame *p) { return p->*(&KeyFrameTables::mMutexConnections); }
};
}  // namespace

class KeyFrameConnections {
 public:
  explicit KeyFrameConnections(const std::vector<KeyFrame *> &vpKeyFrames, int th = 15);
  void apply(KeyFrame *pKF);   // what pKF->UpdateConnections() writes (KeyFrame.cc:442-529)

 private:
  int kf(KeyFrame *pKF);
  std::vector<KeyFrame *> mKFs;
  std::map<KeyFrame *, int> mIndex, mTarget;
  std::vector<int32_t> mConnStart, mConnKF, mConnW, mOrdStart, mOrdKF, mOrdW, mKFmax, mNmax;
  int mTh;
};

int KeyFrameConnections::kf(KeyFrame *pKF) {
  const std::map<KeyFrame *, int>::iterator it = mIndex.find(pKF);
  if (it != mIndex.end()) return it->second;
  mIndex[pKF] = (int)mKFs.size();
  mKFs.push_back(pKF);
  return (int)mKFs.size() - 1;
}

KeyFrameConnections::KeyFrameConnections(const std::vector<KeyFrame *> &vpKeyFrames, int th) : mTh(th) {
  std::vector<int32_t> targets;
  for (size_t t = 0; t < vpKeyFrames.size(); t++)
    if (!mTarget.count(vpKeyFrames[t])) { mTarget[vpKeyFrames[t]] = (int)targets.size(); targets.push_back(kf(vpKeyFrames[t])); }
  const int T = (int)targets.size();
  // the rows of the targets, their points, and the observers of those points (every observer is a keyframe of the table; only the
  // targets have rows)
  std::map<MapPoint *, int> ptIndex;
  std::vector<uint8_t> ptBad;
  std::vector<int32_t> rowStart(1, 0), rowPoint, obsStart(1, 0), obsKF;
  for (int t = 0; t < T; t++) {
    const std::vector<MapPoint *> vpMP = mKFs[t]->GetMapPointMatches();   // targets are slots 0 .. T-1
    for (size_t i = 0; i < vpMP.size(); i++) {
      MapPoint *pMP = vpMP[i];
      if (!pMP) { rowPoint.push_back(-1); continue; }
      std::map<MapPoint *, int>::iterator it = ptIndex.find(pMP);
      if (it == ptIndex.end()) {
        it = ptIndex.insert(std::make_pair(pMP, (int)ptBad.size())).first;
        ptBad.push_back(pMP->isBad() ? 1 : 0);
        if (!ptBad.back()) {
          const std::map<KeyFrame *, std::tuple<int, int> > observations = pMP->GetObservations();
          for (std::map<KeyFrame *, std::tuple<int, int> >::const_iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++)
            obsKF.push_back(kf(mit->first));
        }
        obsStart.push_back((int32_t)obsKF.size());
      }
      rowPoint.push_back(it->second);
    }
    rowStart.push_back((int32_t)rowPoint.size());
  }
  const int G = (int)mKFs.size(), P = (int)ptBad.size();
  rowStart.resize((size_t)G + 1, (int32_t)rowPoint.size());
  std::vector<int32_t> rank(G), map(G), best((size_t)G * ORBM_MAP_BEST, -1), childStart((size_t)G + 1, 0), parent(G, -1);
  std::vector<uint8_t> kfBad(G);
  std::vector<KeyFrame *> byAddress(mKFs);
  std::sort(byAddress.begin(), byAddress.end(), std::less<KeyFrame *>());
  for (int r = 0; r < G; r++) rank[mIndex[byAddress[r]]] = r;
  std::map<Map *, int> mapIndex;
  for (int g = 0; g < G; g++) {
    kfBad[g] = mKFs[g]->isBad() ? 1 : 0;
    Map *pMap = mKFs[g]->GetMap();
    if (!mapIndex.count(pMap)) { const int n = (int)mapIndex.size(); mapIndex[pMap] = n; }
    map[g] = mapIndex[pMap];
  }
  orbm_map_graph_t graph;
  graph.G = G; graph.kf_rank = rank.data(); graph.kf_bad = kfBad.data(); graph.kf_map = map.data();
  graph.kf_row_start = rowStart.data(); graph.row_point = rowPoint.data(); graph.kf_best = best.data();
  graph.kf_child_start = childStart.data(); graph.kf_child = NULL; graph.kf_parent = parent.data(); graph.kf_prev = NULL;
  graph.P = P; graph.pt_bad = ptBad.data(); graph.obs_start = obsStart.data(); graph.obs_kf = obsKF.data();
  const size_t cap = (size_t)T * (size_t)G;
  mConnStart.assign(T + 1, 0); mOrdStart.assign(T + 1, 0); mKFmax.assign(T > 0 ? T : 1, -1); mNmax.assign(T > 0 ? T : 1, 0);
  mConnKF.assign(cap > 0 ? cap : 1, 0); mConnW = mConnKF; mOrdKF = mConnKF; mOrdW = mConnKF;
  if (orbm_update_connections(connections_matcher(), &graph, T, targets.data(), mTh, (int)cap, mConnStart.data(), mConnKF.data(), mConnW.data(),
                              mOrdStart.data(), mOrdKF.data(), mOrdW.data(), mKFmax.data(), mNmax.data()) < 0)
    throw std::runtime_error(std::string("KeyFrame::UpdateConnections: ") + orbm_last_error(connections_matcher()));
}

void KeyFrameConnections::apply(KeyFrame *pKF) {
  const std::map<KeyFrame *, int>::const_iterator tit = mTarget.find(pKF);
  if (tit == mTarget.end()) throw std::runtime_error("KeyFrame::UpdateConnections: a keyframe that was not given to the constructor");
  const int t = tit->second, c0 = mConnStart[t], c1 = mConnStart[t + 1], o0 = mOrdStart[t], o1 = mOrdStart[t + 1];
  if (c0 == c1) return;                                             // KFcounter.empty() (:442)
  bool anyPair = false;
  for (int i = c0; i < c1; i++)                                     // address order, as the loop of :455-469
    if (mConnW[i] >= mTh) { mKFs[mConnKF[i]]->AddConnection(pKF, mConnW[i]); anyPair = true; }
  if (!anyPair) mKFs[mKFmax[t]]->AddConnection(pKF, mNmax[t]);      // :471-475
  std::unique_lock<std::mutex> lockCon(KeyFrameTables::mutex(pKF));   // :486-528
  std::map<KeyFrame *, int> &weights = KeyFrameTables::weights(pKF);
  weights.clear();
  for (int i = c0; i < c1; i++) weights[mKFs[mConnKF[i]]] = mConnW[i];
  std::vector<KeyFrame *> &ordered = KeyFrameTables::ordered(pKF);
  std::vector<int> &orderedWeights = KeyFrameTables::orderedWeights(pKF);
  ordered.clear(); orderedWeights.clear();
  for (int i = o0; i < o1; i++) { ordered.push_back(mKFs[mOrdKF[i]]); orderedWeights.push_back(mOrdW[i]); }
  if (KeyFrameTables::firstConnection(pKF) && pKF->mnId != pKF->GetMap()->GetInitKFid()) {
    KeyFrameTables::parent(pKF) = ordered.front();
    ordered.front()->AddChild(pKF);
    KeyFrameTables::firstConnection(pKF) = false;
  }
}

}  // namespace ORB_SLAM3
