// MapPoint_UpdateBatch_hip.cc -- drop-in bodies of void MapPoint::ComputeDistinctiveDescriptors() (src/MapPoint.cc:350-436) and
// void MapPoint::UpdateNormalAndDepth() (src/MapPoint.cc:467-547), and MapPointUpdateBatch, which runs both for a whole vector of map
// points with ONE device call (orbm_update_map_points) - the loop of src/LocalMapping.cc:1040-1053, and the per-point pair behind
// LocalMapping::CreateNewMapPoints (:890-897) and at initialisation (Tracking.cc:2353, :2374, :2552, :3400, :4460).
//
// Delete (or #if 0) lines 350-436 and 467-547 of src/MapPoint.cc and add this file to the library's sources; it REPLACES
// MapPoint_ComputeDistinctiveDescriptors_hip.cc where both members are wanted (the two files define the same member).  Declare the
// helper where it is used:
//     namespace ORB_SLAM3 { struct MapPointUpdateBatch { static void Run(const std::vector<MapPoint*> &vpMPs); }; }
//
// mDescriptor, mfMinDistance, mfMaxDistance and mNormalVector are protected and the reference's headers stay unmodified, so Run() does
// not write them: it hands its results to the two members through a thread-local table and then calls the members, which keep the
// reference's locks, early returns and write-back lines.  A member takes the table's result only when the table holds `this` AND what it
// copies under its own lock equals what Run() saw: the observations (and the keyframes' isBad() flags) for the descriptor; the
// observations, the reference keyframe and the position for the normal and the depth range.  Otherwise - a member called outside Run(),
// or a concurrent change between the snapshot and the write - it takes the single-point path, the same entry with nmp = 1 on the state
// of that moment.  So the writes happen in the reference's order, under its locks, with what the reference's member gives at that moment.
// The camera centres are read at the snapshot (the reference reads them, unlocked, inside the member).
// More than 1024 entries of one map point (ORBM limit, include/orbhip.h) are refused with an exception.
#include "MapPoint.h"

#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "KeyFrame.h"
#include "orbhip.h"

namespace ORB_SLAM3 {

struct MapPointUpdateBatch { static void Run(const std::vector<MapPoint *> &vpMPs); };

namespace {
typedef std::map<KeyFrame *, std::tuple<int, int> > Observations;

orbm_t *update_matcher() {   // one handle per thread: LocalMapping and Tracking both update map points
  thread_local orbm_t *m = nullptr;
  if (!m) {
    const char *e = std::getenv("ORBHIP_DEVICE");
    m = orbm_create(e ? std::atoi(e) : 0);
    if (!m) throw std::runtime_error("MapPoint update: orbm_create failed (no usable HIP device; there is no CPU fallback)");
  }
  return m;
}

// The flat entries of map points in the layout of orbm_map_point_update_t
struct Entries {
  std::vector<int32_t> start{0};
  std::vector<uint8_t> desc, in_desc;
  std::vector<float> centre, pos, ref_centre, ref_scale, ref_max_scale;

  void entry(KeyFrame *pKF, int index, const cv::Mat &Ow, bool good) {
    const uint8_t *row = pKF->mDescriptors.ptr<uint8_t>(index);
    desc.insert(desc.end(), row, row + 32);
    for (int k = 0; k < 3; k++) centre.push_back(Ow.at<float>(k));
    in_desc.push_back(good ? 1 : 0);
  }
  // One point: the walk of :371-386 / :489-511 and the reference keyframe's level by :519-531
  void point(Observations observations, KeyFrame *pRefKF, const cv::Mat &Pos) {
    for (Observations::iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
      KeyFrame *pKF = mit->first;
      const bool good = !pKF->isBad();
      const int leftIndex = std::get<0>(mit->second), rightIndex = std::get<1>(mit->second);
      if (leftIndex != -1) entry(pKF, leftIndex, pKF->GetCameraCenter(), good);
      if (rightIndex != -1) entry(pKF, rightIndex, pKF->GetRightCameraCenter(), good);
    }
    start.push_back((int32_t)in_desc.size());
    const cv::Mat Ow = pRefKF->GetCameraCenter();
    for (int k = 0; k < 3; k++) { pos.push_back(Pos.at<float>(k)); ref_centre.push_back(Ow.at<float>(k)); }
    const std::tuple<int, int> indexes = observations[pRefKF];   // :519, on the copy as there
    const int leftIndex = std::get<0>(indexes), rightIndex = std::get<1>(indexes);
    int level;
    if (pRefKF->NLeft == -1) level = pRefKF->mvKeysUn[leftIndex].octave;
    else if (leftIndex != -1) level = pRefKF->mvKeys[leftIndex].octave;
    else level = pRefKF->mvKeysRight[rightIndex - pRefKF->NLeft].octave;
    ref_scale.push_back(pRefKF->mvScaleFactors[level]);
    ref_max_scale.push_back(pRefKF->mvScaleFactors[pRefKF->mnScaleLevels - 1]);
  }
  int size() const { return (int)start.size() - 1; }
  void run(const char *who, std::vector<int32_t> &best, std::vector<float> &normal, std::vector<float> &mind, std::vector<float> &maxd) const {
    const size_t n = (size_t)size();
    best.assign(n, -1); normal.assign(3 * n, 0.f); mind.assign(n, 0.f); maxd.assign(n, 0.f);
    const orbm_map_point_update_t u = {(int32_t)n, start.data(), desc.data(), centre.data(), in_desc.data(), pos.data(), ref_centre.data(),
                                       ref_scale.data(), ref_max_scale.data()};
    if (orbm_update_map_points(update_matcher(), &u, best.data(), normal.data(), mind.data(), maxd.data()) < 0)
      throw std::runtime_error(std::string(who) + ": " + orbm_last_error(update_matcher()));
  }
};

// What Run() computed for one map point, and what it computed it from
struct Result {
  Observations observations;
  std::vector<uint8_t> in_desc;   // per entry, the keyframes' !isBad() at the snapshot
  KeyFrame *pRefKF;
  float pos[3];
  int32_t best;                   // entry index, -1: none
  uint8_t row[32];                // that entry's descriptor
  float normal[3], min_dist, max_dist;
};
thread_local std::unordered_map<MapPoint *, Result> tUpdateTable;

bool same_position(const cv::Mat &Pos, const float *p) { return std::memcmp(Pos.ptr<float>(0), p, 3 * sizeof(float)) == 0; }
}  // namespace

void MapPointUpdateBatch::Run(const std::vector<MapPoint *> &vpMPs) {
  Entries E;
  std::vector<MapPoint *> listed;
  tUpdateTable.clear();
  for (size_t i = 0; i < vpMPs.size(); i++) {
    MapPoint *pMP = vpMPs[i];
    if (!pMP || pMP->isBad() || tUpdateTable.count(pMP)) continue;   // each pointer once
    Result &R = tUpdateTable[pMP];
    R.observations = pMP->GetObservations();
    R.pRefKF = pMP->GetReferenceKeyFrame();
    const cv::Mat Pos = pMP->GetWorldPos();
    for (int k = 0; k < 3; k++) R.pos[k] = Pos.at<float>(k);
    if (R.observations.empty() || !R.pRefKF) { tUpdateTable.erase(pMP); continue; }   // the members return early, or take their own path
    const size_t first = E.in_desc.size();
    E.point(R.observations, R.pRefKF, Pos);
    R.in_desc.assign(E.in_desc.begin() + first, E.in_desc.end());
    listed.push_back(pMP);
  }
  if (!listed.empty()) {
    std::vector<int32_t> best;
    std::vector<float> normal, mind, maxd;
    E.run("MapPointUpdateBatch::Run", best, normal, mind, maxd);
    for (size_t p = 0; p < listed.size(); p++) {
      Result &R = tUpdateTable[listed[p]];
      R.best = best[p];
      if (R.best >= 0) std::memcpy(R.row, &E.desc[32 * ((size_t)E.start[p] + (size_t)R.best)], 32);
      for (int k = 0; k < 3; k++) R.normal[k] = normal[3 * p + k];
      R.min_dist = mind[p]; R.max_dist = maxd[p];
    }
  }
  try {
    for (size_t i = 0; i < vpMPs.size(); i++) {                      // the reference's loop, in the vector's order
      MapPoint *pMP = vpMPs[i];
      if (!pMP || pMP->isBad()) continue;
      pMP->ComputeDistinctiveDescriptors();
      pMP->UpdateNormalAndDepth();
    }
  } catch (...) {
    tUpdateTable.clear();
    throw;
  }
  tUpdateTable.clear();
}

void MapPoint::ComputeDistinctiveDescriptors() {
  std::map<KeyFrame *, std::tuple<int, int> > observations;
  {
    std::unique_lock<std::mutex> lock1(mMutexFeatures);   // :358-363
    if (mbBad) return;
    observations = mObservations;
  }
  if (observations.empty()) return;
  // the walk of :371-386: the flagged rows, and every keyframe's flag per entry for the comparison with the snapshot
  std::vector<cv::Mat> vDescriptors;
  std::vector<uint8_t> in_desc;
  vDescriptors.reserve(observations.size());
  for (std::map<KeyFrame *, std::tuple<int, int> >::iterator mit = observations.begin(), mend = observations.end(); mit != mend; mit++) {
    KeyFrame *pKF = mit->first;
    const bool good = !pKF->isBad();
    const int leftIndex = std::get<0>(mit->second), rightIndex = std::get<1>(mit->second);
    if (leftIndex != -1) { in_desc.push_back(good); if (good) vDescriptors.push_back(pKF->mDescriptors.row(leftIndex)); }
    if (rightIndex != -1) { in_desc.push_back(good); if (good) vDescriptors.push_back(pKF->mDescriptors.row(rightIndex)); }
  }
  if (vDescriptors.empty()) return;   // :389
  cv::Mat chosen;
  const std::unordered_map<MapPoint *, Result>::const_iterator it = tUpdateTable.find(this);
  if (it != tUpdateTable.end() && it->second.best >= 0 && it->second.observations == observations && it->second.in_desc == in_desc) {
    chosen.create(1, 32, CV_8U);
    std::memcpy(chosen.ptr<uint8_t>(0), it->second.row, 32);
  } else {                            // :392-427 for this point alone
    const int N = (int)vDescriptors.size();
    std::vector<uint8_t> desc((size_t)N * 32);
    for (int i = 0; i < N; i++) std::memcpy(&desc[(size_t)i * 32], vDescriptors[i].ptr<uint8_t>(0), 32);
    const int32_t start[2] = {0, N};
    int32_t best = 0;
    if (orbm_distinctive_descriptors(update_matcher(), 1, start, desc.data(), &best) < 0 || best < 0)
      throw std::runtime_error(std::string("MapPoint::ComputeDistinctiveDescriptors: ") + orbm_last_error(update_matcher()));
    chosen = vDescriptors[best].clone();
  }
  {
    std::unique_lock<std::mutex> lock(mMutexFeatures);   // :429-435
    mDescriptor = chosen;
  }
}

void MapPoint::UpdateNormalAndDepth() {
  std::map<KeyFrame *, std::tuple<int, int> > observations;
  KeyFrame *pRefKF;
  cv::Mat Pos;
  {
    std::unique_lock<std::mutex> lock1(mMutexFeatures);   // :473-481
    std::unique_lock<std::mutex> lock2(mMutexPos);
    if (mbBad) return;
    observations = mObservations;
    pRefKF = mpRefKF;
    Pos = mWorldPos.clone();
  }
  if (observations.empty()) return;
  float normal[3], min_dist, max_dist;
  const std::unordered_map<MapPoint *, Result>::const_iterator it = tUpdateTable.find(this);
  if (it != tUpdateTable.end() && it->second.observations == observations && it->second.pRefKF == pRefKF && same_position(Pos, it->second.pos)) {
    const Result &R = it->second;
    for (int k = 0; k < 3; k++) normal[k] = R.normal[k];
    min_dist = R.min_dist; max_dist = R.max_dist;
  } else {                            // :486-535 for this point alone
    Entries E;
    E.point(observations, pRefKF, Pos);
    std::vector<int32_t> best;
    std::vector<float> n, mind, maxd;
    E.run("MapPoint::UpdateNormalAndDepth", best, n, mind, maxd);
    for (int k = 0; k < 3; k++) normal[k] = n[k];
    min_dist = mind[0]; max_dist = maxd[0];
  }
  cv::Mat normalMat(3, 1, CV_32F);
  for (int k = 0; k < 3; k++) normalMat.at<float>(k) = normal[k];
  {
    std::unique_lock<std::mutex> lock3(mMutexPos);   // :541-546
    mfMaxDistance = max_dist;
    mfMinDistance = min_dist;
    mNormalVector = normalMat;
  }
}

}  // namespace ORB_SLAM3
