// LocalMapping_KeyFrameCulling_hip.cc -- the redundancy counts of void LocalMapping::KeyFrameCulling() (src/LocalMapping.cc:1158-1310)
// from the device: the per-keyframe walk over every map point's observations (:1202-1264) becomes one upload in front of the loop
// (orbm_keyframe_culling_open) and one orbm_keyframe_culling_step per keyframe that passes the test.
//
// A helper class, KeyFrameCullingCounts, not a member swap: the reference's loop, with its inertial branch (:1268-1299) and its
// mbAbortBA / count breaks (:1305), stays in src/LocalMapping.cc.  Add this file to the library's sources and make three edits there
// (INTEGRATION.md):
//   1. in front of the loop (:1195):
//        KeyFrameCullingCounts cull(vpLocalKeyFrames, mbMonocular, redundant_th);
//   2. lines :1202-1264 become
//        int nMPs, nRedundantObservations; cull.counts(pKF, nMPs, nRedundantObservations);
//   3. after each of the three `pKF->SetBadFlag();` (:1287, :1296, :1302):
//        cull.erased(pKF);
//
// Why the counts of a later keyframe may come from the device although SetBadFlag changes map points in between - the
// SEQUENTIAL CULLING RULE of include/orbhip.h: the device carries Observations(), GetObservations() and isBad() of every map point through the loop in the
// loop's order.  It stops at every keyframe that passes the test; erased(pKF) reports pKF->isBad() as `applied`, so the device erases
// exactly the keyframes that SetBadFlag erased (mbNotErase, KeyFrame.cc:650-655, leaves isBad() false).  A passing keyframe for which
// the host never calls erased() - the inertial conditions said no, or the loop broke - counts as not applied.
//
// THE SNAPSHOT.  Observations, isBad() and the keyframe list are read once, in the constructor; the reference reads them at each
// iteration.  Tracking can add observations of a newer keyframe meanwhile and loop closing can set a keyframe bad: a difference in time,
// as for the other batch snippets.  A keyframe that turned bad after the snapshot is `continue`d by the loop's own test (:1200) before
// counts() is reached; should counts() be asked for it anyway it answers with the snapshot's counts, and since erased() is not called
// its observations stay in the device's tables for the rest of this loop.  A keyframe that was bad or the map's first at the snapshot
// answers 0, 0.
// THE RIG OCTAVE.  For a rig row i >= NLeft the reference reads mvKeysRight[i].octave (:1226), not [i - NLeft].  The snippet passes the
// reference's value where i < mvKeysRight.size() and mvKeysRight[i - NLeft].octave where the reference would read past the vector.
#include <cstdlib>
#include <list>   // Map.h names std::list without including it
#include <map>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "LocalMapping.h"
#include "KeyFrame.h"
#include "MapPoint.h"
#include "orbhip.h"

namespace ORB_SLAM3 {

namespace {
orbm_t *culling_matcher() {   // one handle per thread, as in ORBmatcher_hip.cc
  thread_local orbm_t *m = nullptr;
  if (!m) {
    const char *e = std::getenv("ORBHIP_DEVICE");
    m = orbm_create(e ? std::atoi(e) : 0);
    if (!m) throw std::runtime_error("LocalMapping::KeyFrameCulling: orbm_create failed (no usable HIP device; there is no CPU fallback)");
  }
  return m;
}
}  // namespace

class KeyFrameCullingCounts {
 public:
  KeyFrameCullingCounts(const std::vector<KeyFrame *> &vpLocalKeyFrames, bool bMonocular, float redundant_th);
  // nMPs and nRedundantObservations of :1204-1264 for pKF, at this point of the loop; asks the device to walk on as far as needed
  void counts(KeyFrame *pKF, int &nMPs, int &nRedundantObservations);
  // after pKF->SetBadFlag(): whether the keyframe was erased (mbNotErase leaves it alive)
  void erased(KeyFrame *pKF);

 private:
  int point(MapPoint *pMP);
  std::map<KeyFrame *, int> mIndex;
  std::map<MapPoint *, int> mPoint;
  std::vector<uint8_t> mSkip, mBad, mObsW;
  std::vector<float> mThDepth, mRowDepth;
  std::vector<int32_t> mRowStart, mRowPoint, mRowLevel, mNObs, mObsStart, mObsKF, mObsLevel, mnMPs, mnRed;
  int mK, mWalked, mReturned, mApplied;   // keyframes [0, mWalked) have counts; the passing keyframe of the last step; what the next step applies
};

// One distinct map point: Observations(), isBad() and GetObservations() flattened, levels by :1236-1248, weights by MapPoint.cc:179-187
int KeyFrameCullingCounts::point(MapPoint *pMP) {
  const std::map<MapPoint *, int>::iterator it = mPoint.find(pMP);
  if (it != mPoint.end()) return it->second;
  const int p = (int)mBad.size();
  mPoint[pMP] = p;
  const bool bad = pMP->isBad();
  mBad.push_back(bad ? 1 : 0);
  mNObs.push_back(pMP->Observations());
  if (!bad) {   // a bad point's observations are cleared (MapPoint.cc:225)
    const std::map<KeyFrame *, std::tuple<int, int> > observations = pMP->GetObservations();
    for (std::map<KeyFrame *, std::tuple<int, int> >::const_iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
      KeyFrame *pKFi = mit->first;
      const int leftIndex = std::get<0>(mit->second), rightIndex = std::get<1>(mit->second);
      if (leftIndex == -1 && rightIndex == -1) throw std::runtime_error("LocalMapping::KeyFrameCulling: an observation without an index");
      int scaleLeveli = -1;
      if (pKFi->NLeft == -1)
        scaleLeveli = pKFi->mvKeysUn[leftIndex].octave;
      else {
        if (leftIndex != -1) scaleLeveli = pKFi->mvKeys[leftIndex].octave;
        if (rightIndex != -1) {
          const int rightLevel = pKFi->mvKeysRight[rightIndex - pKFi->NLeft].octave;
          scaleLeveli = (scaleLeveli == -1 || scaleLeveli > rightLevel) ? rightLevel : scaleLeveli;
        }
      }
      int w = 0;
      if (leftIndex != -1) w += (!pKFi->mpCamera2 && pKFi->mvuRight[leftIndex] >= 0) ? 2 : 1;
      if (rightIndex != -1) w += 1;
      const std::map<KeyFrame *, int>::const_iterator kit = mIndex.find(pKFi);
      mObsKF.push_back(kit == mIndex.end() ? -1 : kit->second);
      mObsLevel.push_back(scaleLeveli);
      mObsW.push_back((uint8_t)w);
    }
  }
  mObsStart.push_back((int32_t)mObsKF.size());
  return p;
}

KeyFrameCullingCounts::KeyFrameCullingCounts(const std::vector<KeyFrame *> &vpLocalKeyFrames, bool bMonocular, float redundant_th)
    : mK((int)vpLocalKeyFrames.size()), mWalked(0), mReturned(-1), mApplied(0) {
  for (int k = 0; k < mK; k++) mIndex[vpLocalKeyFrames[k]] = k;
  mRowStart.push_back(0);
  mObsStart.push_back(0);
  for (int k = 0; k < mK; k++) {
    KeyFrame *pKF = vpLocalKeyFrames[k];
    const bool skip = pKF->mnId == pKF->GetMap()->GetInitKFid() || pKF->isBad();   // :1200
    mSkip.push_back(skip ? 1 : 0);
    mThDepth.push_back(pKF->mThDepth);
    if (!skip) {
      const std::vector<MapPoint *> vpMapPoints = pKF->GetMapPointMatches();
      for (size_t i = 0, iend = vpMapPoints.size(); i < iend; i++) {
        MapPoint *pMP = vpMapPoints[i];
        mRowPoint.push_back(pMP ? point(pMP) : -1);
        int scaleLevel = 0;
        if (pMP) {   // :1224-1226
          if (pKF->NLeft == -1) scaleLevel = pKF->mvKeysUn[i].octave;
          else if ((int)i < pKF->NLeft) scaleLevel = pKF->mvKeys[i].octave;
          else scaleLevel = i < pKF->mvKeysRight.size() ? pKF->mvKeysRight[i].octave : pKF->mvKeysRight[i - pKF->NLeft].octave;
        }
        mRowLevel.push_back(scaleLevel);
        if (!bMonocular) mRowDepth.push_back(pKF->mvDepth[i]);
      }
    }
    mRowStart.push_back((int32_t)mRowPoint.size());
  }
  mnMPs.assign(mK > 0 ? mK : 1, 0);
  mnRed.assign(mK > 0 ? mK : 1, 0);
  orbm_culling_t c;
  c.K = mK; c.skip = mSkip.data(); c.th_depth = mThDepth.data();
  c.row_start = mRowStart.data(); c.row_point = mRowPoint.data(); c.row_level = mRowLevel.data();
  c.row_depth = bMonocular ? NULL : mRowDepth.data();
  c.P = (int32_t)mBad.size(); c.bad = mBad.data(); c.n_obs = mNObs.data();
  c.obs_start = mObsStart.data(); c.obs_kf = mObsKF.data(); c.obs_level = mObsLevel.data(); c.obs_w = mObsW.data();
  c.mono = bMonocular ? 1 : 0; c.redundant_th = redundant_th;
  if (orbm_keyframe_culling_open(culling_matcher(), &c) < 0)
    throw std::runtime_error(std::string("LocalMapping::KeyFrameCulling: ") + orbm_last_error(culling_matcher()));
}

void KeyFrameCullingCounts::counts(KeyFrame *pKF, int &nMPs, int &nRedundantObservations) {
  const std::map<KeyFrame *, int>::const_iterator kit = mIndex.find(pKF);
  if (kit == mIndex.end()) throw std::runtime_error("LocalMapping::KeyFrameCulling: a keyframe that is not in the list");
  const int k = kit->second;
  while (mWalked <= k) {   // the device stops at every passing keyframe: walk on until k has been reached
    int32_t at = mK;
    if (orbm_keyframe_culling_step(culling_matcher(), mApplied, &at, mnMPs.data(), mnRed.data()) < 0)
      throw std::runtime_error(std::string("LocalMapping::KeyFrameCulling: ") + orbm_last_error(culling_matcher()));
    mApplied = 0;
    mReturned = at < mK ? at : -1;
    mWalked = at < mK ? at + 1 : mK;
  }
  nMPs = mnMPs[k];
  nRedundantObservations = mnRed[k];
}

void KeyFrameCullingCounts::erased(KeyFrame *pKF) {
  const std::map<KeyFrame *, int>::const_iterator kit = mIndex.find(pKF);
  if (kit != mIndex.end() && kit->second == mReturned) mApplied = pKF->isBad() ? 1 : 0;
}

}  // namespace ORB_SLAM3
