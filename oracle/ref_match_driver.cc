/*
 * ref_match_driver.cc -- extern "C" face of libref_matcher.so (TEST INFRASTRUCTURE).
 *
 * libref_matcher.so = the reference's own src/ORBmatcher.cc, src/CameraModels/Pinhole.cpp and KannalaBrandt8.cpp, compiled unmodified
 * against the stand-in headers of oracle/ref_cam_shim, plus this file.  The reference's text is read from $(ORB_REFERENCE) at build
 * time and is never copied into this repository.  This file includes nothing of the product, of orb_oracle.c or of tests/, and the
 * library links neither.
 *
 * Two things live here:
 *
 *  1. The members of Frame, KeyFrame and MapPoint that ORBmatcher.cc calls.  Their own files (Frame.cc, KeyFrame.cc, MapPoint.cc)
 *     need g2o, the vocabulary and the optimiser and cannot be compiled, so each is written out here, in a few lines, after the
 *     file:line it follows.  THESE DEFINITIONS ARE OURS AND REMAIN UNPINNED; the pin covers the text of ORBmatcher.cc and of the two
 *     camera files it calls.  A member that no pinned search reaches aborts with its name instead of carrying an untested body.
 *
 *  2. One entry point per pinned ORBmatcher member.  Each takes the flattened arrays of the matching orc_* function of
 *     orb_oracle.h, builds Frame / KeyFrame / MapPoint objects from them, calls the member and flattens the result: the return
 *     value and F.mvpMapPoints / vpMapPointMatches / vnMatches12 as indices.
 *
 * Slots.  mvpMapPoints travels as slot[i] (the tag of the map point at keypoint i, -1 = NULL) and slot_obs[i] (Observations() > 0
 * of that point, 0 where the slot is empty).  A tag >= 0 on entry becomes an occupant with that tag; the queries are tagged with
 * their own index.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <set>
#include <vector>

#include "ORBmatcher.h"
#include "CameraModels/KannalaBrandt8.h"
#include "CameraModels/Pinhole.h"

/* ================================================================================================================================ */
/* 1. driver-defined members (unpinned)                                                                                              */
/* ================================================================================================================================ */
namespace ORB_SLAM3 {

#define REFM_NOT_REACHED(name)                                                                        \
  do {                                                                                                \
    fprintf(stderr, "ref_match_driver: %s is reached by no pinned member and has no body\n", name); \
    abort();                                                                                          \
  } while (0)

TwoViewReconstruction::TwoViewReconstruction(cv::Mat &, float, int) { REFM_NOT_REACHED("TwoViewReconstruction"); }
bool TwoViewReconstruction::Reconstruct(const std::vector<cv::KeyPoint> &, const std::vector<cv::KeyPoint> &, const std::vector<int> &, cv::Mat &,
                                        cv::Mat &, std::vector<cv::Point3f> &, std::vector<bool> &) {
  REFM_NOT_REACHED("TwoViewReconstruction::Reconstruct");
}

/* ---- Frame --------------------------------------------------------------------------------------------------------------------- */
float Frame::mnMinX = 0, Frame::mnMaxX = 0, Frame::mnMinY = 0, Frame::mnMaxY = 0;
float Frame::mfGridElementWidthInv = 0, Frame::mfGridElementHeightInv = 0;
float Frame::fx = 0, Frame::fy = 0, Frame::cx = 0, Frame::cy = 0, Frame::invfx = 0, Frame::invfy = 0;

/* Frame.cc:45: an empty frame; every pointer null, no right image */
Frame::Frame()
    : mpcpi(NULL), mpORBvocabulary(NULL), mpORBextractorLeft(NULL), mpORBextractorRight(NULL), mTimeStamp(0), mbf(0), mb(0), mThDepth(0), N(0),
      mnCloseMPs(0), mpImuPreintegrated(NULL), mpLastKeyFrame(NULL), mpPrevFrame(NULL), mpImuPreintegratedFrame(NULL), mnId(0),
      mpReferenceKF(NULL), mnScaleLevels(0), mfScaleFactor(0), mfLogScaleFactor(0), mnDataset(0), mTimeStereoMatch(0), mTimeORB_Ext(0),
      mbImuPreintegrated(false), mpMutexImu(NULL), mpCamera(NULL), mpCamera2(NULL), Nleft(-1), Nright(-1), monoLeft(-1), monoRight(-1) {}

/* Frame.cc:744-813.  The cell window [floor((c - min - r) * inv), ceil((c - min + r) * inv)] clipped to the grid, on each axis; a
   window wholly outside gives nothing.  Cells are walked ix then iy and each cell in its stored order: the order the searches'
   first-minimum ties depend on.  Level filter: on when minLevel > 0 or maxLevel >= 0; the upper bound only when maxLevel >= 0. */
vector<size_t> Frame::GetFeaturesInArea(const float &x, const float &y, const float &r, const int minLevel, const int maxLevel, const bool bRight) const {
  vector<size_t> found;
  found.reserve(N);
  const int x0 = std::max(0, (int)floorf((x - mnMinX - r) * mfGridElementWidthInv));
  if (x0 >= FRAME_GRID_COLS) return found;
  const int x1 = std::min((int)FRAME_GRID_COLS - 1, (int)ceilf((x - mnMinX + r) * mfGridElementWidthInv));
  if (x1 < 0) return found;
  const int y0 = std::max(0, (int)floorf((y - mnMinY - r) * mfGridElementHeightInv));
  if (y0 >= FRAME_GRID_ROWS) return found;
  const int y1 = std::min((int)FRAME_GRID_ROWS - 1, (int)ceilf((y - mnMinY + r) * mfGridElementHeightInv));
  if (y1 < 0) return found;
  const bool levels = minLevel > 0 || maxLevel >= 0;
  const std::vector<cv::KeyPoint> &keys = Nleft == -1 ? mvKeysUn : (bRight ? mvKeysRight : mvKeys);
  for (int ix = x0; ix <= x1; ix++)
    for (int iy = y0; iy <= y1; iy++) {
      const std::vector<size_t> &cell = bRight ? mGridRight[ix][iy] : mGrid[ix][iy];
      for (size_t j = 0; j < cell.size(); j++) {
        const cv::KeyPoint &kp = keys[cell[j]];
        if (levels && (kp.octave < minLevel || (maxLevel >= 0 && kp.octave > maxLevel))) continue;
        if (fabsf(kp.pt.x - x) < r && fabsf(kp.pt.y - y) < r) found.push_back(cell[j]);
      }
    }
  return found;
}

/* ---- KeyFrame ------------------------------------------------------------------------------------------------------------------ */
/* KeyFrame.cc:48-98: a keyframe takes over the frame's keypoints, descriptors, BoW vectors, pyramid constants, map points, cameras
   and grids.  The IMU, database, vocabulary and map members are left empty; SetPose (KeyFrame.cc:112) is not called because no pinned
   member reads a keyframe pose. */
KeyFrame::KeyFrame(Frame &F, Map *pMap, KeyFrameDatabase *pKFDB)
    : bImu(false), mnId(0), mnFrameId(F.mnId), mTimeStamp(F.mTimeStamp), mnGridCols(FRAME_GRID_COLS), mnGridRows(FRAME_GRID_ROWS),
      mfGridElementWidthInv(F.mfGridElementWidthInv), mfGridElementHeightInv(F.mfGridElementHeightInv), mnTrackReferenceForFrame(0),
      mnFuseTargetForKF(0), mnBALocalForKF(0), mnBAFixedForKF(0), mnNumberOfOpt(0), mnLoopQuery(0), mnLoopWords(0), mLoopScore(0),
      mnRelocQuery(0), mnRelocWords(0), mRelocScore(0), mnMergeQuery(0), mnMergeWords(0), mMergeScore(0), mnPlaceRecognitionQuery(0),
      mnPlaceRecognitionWords(0), mPlaceRecognitionScore(0), mbCurrentPlaceRecognition(false), mnBAGlobalForKF(0), mnMergeCorrectedForKF(0),
      mnMergeForKF(0), mfScaleMerge(0), mnBALocalForMerge(0), mfScale(0), fx(F.fx), fy(F.fy), cx(F.cx), cy(F.cy), invfx(F.invfx),
      invfy(F.invfy), mbf(F.mbf), mb(F.mb), mThDepth(F.mThDepth), N(F.N), mvKeys(F.mvKeys), mvKeysUn(F.mvKeysUn), mvuRight(F.mvuRight),
      mvDepth(F.mvDepth), mDescriptors(F.mDescriptors.clone()), mBowVec(F.mBowVec), mFeatVec(F.mFeatVec), mnScaleLevels(F.mnScaleLevels),
      mfScaleFactor(F.mfScaleFactor), mfLogScaleFactor(F.mfLogScaleFactor), mvScaleFactors(F.mvScaleFactors),
      mvLevelSigma2(F.mvLevelSigma2), mvInvLevelSigma2(F.mvInvLevelSigma2), mnMinX((int)F.mnMinX), mnMinY((int)F.mnMinY),
      mnMaxX((int)F.mnMaxX), mnMaxY((int)F.mnMaxY), mPrevKF(NULL), mNextKF(NULL), mpImuPreintegrated(NULL), mnOriginMapId(0), mnDataset(0),
      mbHasHessian(false), mvpMapPoints(F.mvpMapPoints), mpKeyFrameDB(pKFDB), mpORBvocabulary(NULL), mbFirstConnection(true), mpParent(NULL),
      mbNotErase(false), mbToBeErased(false), mbBad(false), mHalfBaseline(0), mpMap(pMap), mpCamera(F.mpCamera), mpCamera2(F.mpCamera2),
      mvLeftToRightMatch(F.mvLeftToRightMatch), mvRightToLeftMatch(F.mvRightToLeftMatch), mvKeysRight(F.mvKeysRight), NLeft(F.Nleft),
      NRight(F.Nright) {
  mGrid.assign(mnGridCols, std::vector<std::vector<size_t> >(mnGridRows));
  if (F.Nleft != -1) mGridRight.assign(mnGridCols, std::vector<std::vector<size_t> >(mnGridRows));
  for (int i = 0; i < mnGridCols; i++)
    for (int j = 0; j < mnGridRows; j++) {
      mGrid[i][j] = F.mGrid[i][j];
      if (F.Nleft != -1) mGridRight[i][j] = F.mGridRight[i][j];
    }
}

/* KeyFrame.cc:384-388: the per-keypoint map points, by value */
vector<MapPoint *> KeyFrame::GetMapPointMatches() { return mvpMapPoints; }

/* reached only by the local-mapping and loop-closing searches, which are not pinned yet */
vector<size_t> KeyFrame::GetFeaturesInArea(const float &, const float &, const float &, const bool) const { REFM_NOT_REACHED("KeyFrame::GetFeaturesInArea"); }
bool KeyFrame::IsInImage(const float &, const float &) const { REFM_NOT_REACHED("KeyFrame::IsInImage"); }
std::set<MapPoint *> KeyFrame::GetMapPoints() { REFM_NOT_REACHED("KeyFrame::GetMapPoints"); }
MapPoint *KeyFrame::GetMapPoint(const size_t &) { REFM_NOT_REACHED("KeyFrame::GetMapPoint"); }
void KeyFrame::AddMapPoint(MapPoint *, const size_t &) { REFM_NOT_REACHED("KeyFrame::AddMapPoint"); }
cv::Mat KeyFrame::GetPose() { REFM_NOT_REACHED("KeyFrame::GetPose"); }
cv::Mat KeyFrame::GetRightPose() { REFM_NOT_REACHED("KeyFrame::GetRightPose"); }
cv::Mat KeyFrame::GetRotation() { REFM_NOT_REACHED("KeyFrame::GetRotation"); }
cv::Mat KeyFrame::GetTranslation() { REFM_NOT_REACHED("KeyFrame::GetTranslation"); }
cv::Mat KeyFrame::GetCameraCenter() { REFM_NOT_REACHED("KeyFrame::GetCameraCenter"); }
cv::Mat KeyFrame::GetRightRotation() { REFM_NOT_REACHED("KeyFrame::GetRightRotation"); }
cv::Mat KeyFrame::GetRightTranslation() { REFM_NOT_REACHED("KeyFrame::GetRightTranslation"); }
cv::Mat KeyFrame::GetRightCameraCenter() { REFM_NOT_REACHED("KeyFrame::GetRightCameraCenter"); }

/* ---- MapPoint ------------------------------------------------------------------------------------------------------------------ */
/* MapPoint.cc:33-37: a point nobody observes, seen by no frame */
MapPoint::MapPoint()
    : mnId(0), mnFirstKFid(0), mnFirstFrame(0), nObs(0), mTrackProjX(0), mTrackProjY(0), mTrackDepth(0), mTrackDepthR(0), mTrackProjXR(0),
      mTrackProjYR(0), mbTrackInView(false), mbTrackInViewR(false), mnTrackScaleLevel(0), mnTrackScaleLevelR(0), mTrackViewCos(0),
      mTrackViewCosR(0), mnTrackReferenceForFrame(0), mnLastFrameSeen(0), mnBALocalForKF(0), mnFuseCandidateForKF(0), mnLoopPointForKF(0),
      mnCorrectedByKF(0), mnCorrectedReference(0), mnBAGlobalForKF(0), mnBALocalForMerge(0), mInvDepth(0), mInitU(0), mInitV(0),
      mpHostKF(NULL), mnOriginMapId(0), mpRefKF(NULL), mBackupRefKFId(0), mnVisible(1), mnFound(1), mbBad(false), mpReplaced(NULL),
      mBackupReplacedId(0), mfMinDistance(0), mfMaxDistance(0), mpMap(NULL) {}

bool MapPoint::isBad() { return mbBad; }                            /* MapPoint.cc:305-310 */
int MapPoint::Observations() { return nObs; }                       /* MapPoint.cc:211-215 */
cv::Mat MapPoint::GetWorldPos() { return mWorldPos.clone(); }       /* MapPoint.cc:123-127 */
cv::Mat MapPoint::GetDescriptor() { return mDescriptor.clone(); }   /* MapPoint.cc:438-442 */
/* MapPoint.cc:555-565: the scale-invariance band is 20 % wider than the stored distances */
float MapPoint::GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
float MapPoint::GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
/* MapPoint.cc:587-602: the level whose scale is nearest above max distance / current distance, clamped to the pyramid.  The text's
   un-suffixed log and ceil of a float are the float overloads (`using namespace std` and <math.h> are both in that file). */
int MapPoint::PredictScale(const float &currentDist, Frame *pF) {
  const float ratio = mfMaxDistance / currentDist;
  const int level = (int)ceilf(logf(ratio) / pF->mfLogScaleFactor);
  return level < 0 ? 0 : (level >= pF->mnScaleLevels ? pF->mnScaleLevels - 1 : level);
}

/* reached only by the local-mapping and loop-closing searches, which are not pinned yet */
int MapPoint::PredictScale(const float &, KeyFrame *) { REFM_NOT_REACHED("MapPoint::PredictScale(KeyFrame*)"); }
cv::Mat MapPoint::GetNormal() { REFM_NOT_REACHED("MapPoint::GetNormal"); }
bool MapPoint::IsInKeyFrame(KeyFrame *) { REFM_NOT_REACHED("MapPoint::IsInKeyFrame"); }
std::tuple<int, int> MapPoint::GetIndexInKeyFrame(KeyFrame *) { REFM_NOT_REACHED("MapPoint::GetIndexInKeyFrame"); }
void MapPoint::AddObservation(KeyFrame *, int) { REFM_NOT_REACHED("MapPoint::AddObservation"); }
void MapPoint::Replace(MapPoint *) { REFM_NOT_REACHED("MapPoint::Replace"); }

}  // namespace ORB_SLAM3

/* ================================================================================================================================ */
/* 2. entry points                                                                                                                   */
/* ================================================================================================================================ */
using ORB_SLAM3::Frame;
using ORB_SLAM3::KeyFrame;
using ORB_SLAM3::MapPoint;
using ORB_SLAM3::ORBmatcher;

extern "C" {
/* what orc_frame_init takes: mvKeysUn (mono / rectified) or one image of a rig, the bounds and the pyramid's scale factors */
struct refm_frame {
  int32_t N;
  const float *kx, *ky;
  const int32_t *octave;
  const float *angle;
  const uint8_t *desc;
  const float *uRight; /* NULL: all -1 */
  float minX, maxX, minY, maxY;
  const float *scaleFactors;
  int32_t nlevels;
};
/* field for field orc_keyframe of orb_oracle.h, so that a test hands both the same record */
struct refm_keyframe {
  int N;
  const float *kx, *ky;
  const int32_t *octave;
  const float *angle;
  const uint8_t *desc;
  const float *uRight;
  const uint8_t *has_mp;
  int n_nodes;
  const uint32_t *node_id;
  const int32_t *node_start;
  const int32_t *node_idx;
  const float *scaleFactors, *levelSigma2;
};
}

namespace {

/* the protected members of ORBmatcher and MapPoint, opened by derivation */
struct Matcher : ORBmatcher {
  Matcher(float nnratio, bool checkOri) : ORBmatcher(nnratio, checkOri) {}
  using ORBmatcher::ComputeThreeMaxima;
  using ORBmatcher::RadiusByViewingCos;
};

struct Point : MapPoint {
  int tag;
  Point(int tag_, int observations) : tag(tag_) { nObs = observations; }
  void descriptor(const uint8_t *d) {
    mDescriptor.create(1, 32, CV_8U);
    memcpy(mDescriptor.ptr<uint8_t>(0), d, 32);
  }
  void position(const float *X) {
    mWorldPos.create(3, 1, CV_32F);
    for (int k = 0; k < 3; k++) mWorldPos.at<float>(k) = X[k];
  }
  void distances(float maxDist, float minDist) { mfMaxDistance = maxDist; mfMinDistance = minDist; }
  void bad(bool b) { mbBad = b; }
};

struct Points {
  std::vector<std::unique_ptr<Point> > all;
  Point *make(int tag, int observations) {
    all.emplace_back(new Point(tag, observations));
    return all.back().get();
  }
};

std::vector<cv::KeyPoint> keypoints(const refm_frame &f) {
  std::vector<cv::KeyPoint> k((size_t)f.N);
  for (int i = 0; i < f.N; i++) {
    k[i].pt.x = f.kx[i]; k[i].pt.y = f.ky[i];
    k[i].octave = f.octave[i]; k[i].angle = f.angle[i];
  }
  return k;
}

/* Frame.cc:434-465 with PosInGrid (:815-825): keypoint i goes to the cell of its rounded grid coordinate, in keypoint order; one
   outside the grid goes nowhere */
void fill_grid(std::vector<size_t> (*grid)[FRAME_GRID_ROWS], const std::vector<cv::KeyPoint> &keys) {
  for (size_t i = 0; i < keys.size(); i++) {
    const int px = (int)roundf((keys[i].pt.x - Frame::mnMinX) * Frame::mfGridElementWidthInv);
    const int py = (int)roundf((keys[i].pt.y - Frame::mnMinY) * Frame::mfGridElementHeightInv);
    if (px < 0 || px >= FRAME_GRID_COLS || py < 0 || py >= FRAME_GRID_ROWS) continue;
    grid[px][py].push_back(i);
  }
}

void pyramid(Frame &F, const float *scaleFactors, int nlevels) {
  F.mnScaleLevels = nlevels;
  F.mvScaleFactors.assign(scaleFactors, scaleFactors + nlevels);
  F.mfScaleFactor = nlevels > 1 ? scaleFactors[1] : 1.f;
  F.mfLogScaleFactor = logf(F.mfScaleFactor);
}

/* Frame.cc:379-380 (the cell sizes) and the static bounds */
void bounds(const refm_frame &f) {
  Frame::mnMinX = f.minX; Frame::mnMaxX = f.maxX; Frame::mnMinY = f.minY; Frame::mnMaxY = f.maxY;
  Frame::mfGridElementWidthInv = (float)FRAME_GRID_COLS / (Frame::mnMaxX - Frame::mnMinX);
  Frame::mfGridElementHeightInv = (float)FRAME_GRID_ROWS / (Frame::mnMaxY - Frame::mnMinY);
}

void descriptors(cv::Mat &m, int row0, const uint8_t *d, int n) {
  for (int i = 0; i < n; i++) memcpy(m.ptr<uint8_t>(row0 + i), d + 32 * (size_t)i, 32);
}

/* a mono / rectified frame (right == NULL) or a fisheye-stereo one: mvKeys ++ mvKeysRight, two grids, one mvpMapPoints */
void build_frame(Frame &F, const refm_frame &left, const refm_frame *right) {
  bounds(left);
  pyramid(F, left.scaleFactors, left.nlevels);
  F.mvKeys = keypoints(left);
  if (!right) {
    F.N = left.N;
    F.mvKeysUn = F.mvKeys;
    F.mvuRight.assign((size_t)left.N, -1.f);
    if (left.uRight) F.mvuRight.assign(left.uRight, left.uRight + left.N);
    F.mDescriptors.create(std::max(F.N, 1), 32, CV_8U);
    descriptors(F.mDescriptors, 0, left.desc, left.N);
    fill_grid(F.mGrid, F.mvKeysUn);
  } else {
    F.Nleft = left.N; F.Nright = right->N; F.N = left.N + right->N;
    F.mvKeysRight = keypoints(*right);
    F.mDescriptors.create(std::max(F.N, 1), 32, CV_8U);
    descriptors(F.mDescriptors, 0, left.desc, left.N);
    descriptors(F.mDescriptors, left.N, right->desc, right->N);
    fill_grid(F.mGrid, F.mvKeys);
    fill_grid(F.mGridRight, F.mvKeysRight);
  }
  F.mvpMapPoints.assign((size_t)F.N, (MapPoint *)NULL);
  F.mvbOutlier.assign((size_t)F.N, false);
}

void slots_in(Frame &F, Points &pts, const int32_t *slot, const uint8_t *slot_obs) {
  for (int i = 0; i < F.N; i++)
    if (slot[i] >= 0) F.mvpMapPoints[i] = pts.make(slot[i], slot_obs[i] ? 1 : 0);
}

void slots_out(const std::vector<MapPoint *> &v, int32_t *slot, uint8_t *slot_obs) {
  for (size_t i = 0; i < v.size(); i++) {
    Point *p = static_cast<Point *>(v[i]);
    slot[i] = p ? p->tag : -1;
    if (slot_obs) slot_obs[i] = p && p->Observations() > 0 ? 1 : 0;
  }
}

cv::Mat matrix(const float *v, int rows, int cols, int stride) {
  cv::Mat m(rows, cols, CV_32F);
  for (int y = 0; y < rows; y++)
    for (int x = 0; x < cols; x++) m.at<float>(y, x) = v[y * stride + x];
  return m;
}

/* GeometricCamera's destructor is not virtual: each object is owned through its own class */
struct Camera {
  std::unique_ptr<ORB_SLAM3::Pinhole> pinhole;
  std::unique_ptr<ORB_SLAM3::KannalaBrandt8> kb8;
  Camera(int cam_type, const float *params) {
    if (cam_type == 0) pinhole.reset(new ORB_SLAM3::Pinhole(std::vector<float>(params, params + 4)));
    if (cam_type == 1) kb8.reset(new ORB_SLAM3::KannalaBrandt8(std::vector<float>(params, params + 8)));
  }
  ORB_SLAM3::GeometricCamera *get() const { return pinhole ? (ORB_SLAM3::GeometricCamera *)pinhole.get() : kb8.get(); }
};

/* the keyframe side of the BoW searches from an orc_keyframe record; n_left != -1 makes it a rig (mvKeys ++ mvKeysRight) */
void build_bow_frame(Frame &F, const refm_keyframe &k, int n_left, Points *pts, ORB_SLAM3::GeometricCamera *second) {
  F.N = k.N;
  std::vector<cv::KeyPoint> keys((size_t)k.N);
  for (int i = 0; i < k.N; i++) {
    keys[i].pt.x = k.kx[i]; keys[i].pt.y = k.ky[i];
    keys[i].octave = k.octave[i]; keys[i].angle = k.angle[i];
  }
  if (n_left == -1) {
    F.mvKeys = keys;
    F.mvKeysUn = keys;
  } else {
    F.Nleft = n_left; F.Nright = k.N - n_left;
    F.mvKeys.assign(keys.begin(), keys.begin() + n_left);
    F.mvKeysRight.assign(keys.begin() + n_left, keys.end());
    F.mpCamera2 = second;
  }
  F.mDescriptors.create(std::max(k.N, 1), 32, CV_8U);
  descriptors(F.mDescriptors, 0, k.desc, k.N);
  F.mvpMapPoints.assign((size_t)k.N, (MapPoint *)NULL);
  F.mvbOutlier.assign((size_t)k.N, false);
  if (pts)
    for (int i = 0; i < k.N; i++)
      if (k.has_mp[i] == 1) F.mvpMapPoints[i] = pts->make(i, 1);
      else if (k.has_mp[i] == 2) { Point *p = pts->make(i, 1); p->bad(true); F.mvpMapPoints[i] = p; }
  for (int a = 0; a < k.n_nodes; a++) {
    std::vector<unsigned int> &v = F.mFeatVec[k.node_id[a]]; /* FeatureVector is a std::map: ascending node ids */
    for (int j = k.node_start[a]; j < k.node_start[a + 1]; j++) v.push_back((unsigned int)k.node_idx[j]);
  }
}

}  // namespace

extern "C" {

/* ORBmatcher::DescriptorDistance (:2463): two 32-byte descriptors as 1 x 32 CV_8U rows */
int refm_descriptor_distance(const uint8_t *a, const uint8_t *b) {
  cv::Mat ma(1, 32, CV_8U), mb(1, 32, CV_8U);
  memcpy(ma.ptr<uint8_t>(0), a, 32);
  memcpy(mb.ptr<uint8_t>(0), b, 32);
  return ORBmatcher::DescriptorDistance(ma, mb);
}

/* ORBmatcher::ComputeThreeMaxima (:2416) on L bins of the given sizes; ind1..3 start at -1 as every caller sets them */
void refm_three_maxima(const int *sizes, int L, int *ind1, int *ind2, int *ind3) {
  std::vector<std::vector<int> > histo((size_t)L);
  for (int i = 0; i < L; i++) histo[i].assign((size_t)sizes[i], 0);
  Matcher m(0.6f, true);
  int a = -1, b = -1, c = -1;
  m.ComputeThreeMaxima(histo.data(), L, a, b, c);
  *ind1 = a; *ind2 = b; *ind3 = c;
}

/* ORBmatcher::RadiusByViewingCos (:216) */
float refm_radius_by_viewing_cos(float viewCos) {
  Matcher m(0.6f, true);
  return m.RadiusByViewingCos(viewCos);
}

/* Frame::GetFeaturesInArea as this driver defines it (unpinned), so that a test can compare the enumeration order on its own */
int refm_get_features_in_area(const refm_frame *f, float x, float y, float r, int minLevel, int maxLevel, int32_t *out) {
  Frame F;
  build_frame(F, *f, NULL);
  const std::vector<size_t> v = F.GetFeaturesInArea(x, y, r, minLevel, maxLevel);
  for (size_t i = 0; i < v.size(); i++) out[i] = (int32_t)v[i];
  return (int)v.size();
}

/* SearchByProjection(Frame&, vector<MapPoint*>&, th, bFarPoints, thFarPoints) (:44).  right == NULL: mono / rectified stereo, the
   arrays of orc_search_by_projection_mp.  right != NULL: a fisheye-stereo frame, the arrays of orc_search_by_projection_mp_fisheye
   (projXR / projYR / viewCosR / levelR / in_view_r are the right camera's; leftToRight / rightToLeft the stereo partners).
   in_view = mbTrackInView, bad = isBad() (NULL: none), trackDepth = mTrackDepth (NULL: 0). */
int refm_search_by_projection_mp(const refm_frame *left, const refm_frame *right, const int32_t *leftToRight, const int32_t *rightToLeft, int nq,
                                 const uint8_t *in_view, const uint8_t *in_view_r, const uint8_t *bad, const float *trackDepth,
                                 const uint8_t *qdesc, const float *projX, const float *projY, const float *viewCos, const int32_t *level,
                                 const float *projXR, const float *projYR, const float *viewCosR, const int32_t *levelR, const uint8_t *qobs,
                                 float th, int bFarPoints, float thFarPoints, float nnratio, int32_t *slot, uint8_t *slot_obs) {
  Frame F;
  build_frame(F, *left, right);
  if (right) {
    F.mvLeftToRightMatch.assign(leftToRight, leftToRight + left->N);
    F.mvRightToLeftMatch.assign(rightToLeft, rightToLeft + right->N);
  }
  Points pts;
  slots_in(F, pts, slot, slot_obs);
  std::vector<MapPoint *> queries((size_t)nq);
  for (int q = 0; q < nq; q++) {
    Point *p = pts.make(q, qobs ? (qobs[q] ? 1 : 0) : 1);
    p->descriptor(qdesc + 32 * (size_t)q);
    p->bad(bad && bad[q]);
    p->mbTrackInView = in_view[q] != 0;
    p->mTrackProjX = projX[q]; p->mTrackProjY = projY[q];
    p->mTrackViewCos = viewCos[q];
    p->mnTrackScaleLevel = level[q];
    p->mTrackDepth = trackDepth ? trackDepth[q] : 0.f;
    p->mTrackProjXR = projXR ? projXR[q] : 0.f;
    if (right) {
      p->mbTrackInViewR = in_view_r[q] != 0;
      p->mTrackProjYR = projYR[q];
      p->mTrackViewCosR = viewCosR[q];
      p->mnTrackScaleLevelR = levelR[q];
    }
    queries[q] = p;
  }
  ORBmatcher matcher(nnratio, true);
  const int n = matcher.SearchByProjection(F, queries, th, bFarPoints != 0, thFarPoints);
  slots_out(F.mvpMapPoints, slot, slot_obs);
  return n;
}

/* SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono) (:2027), the arrays of orc_search_by_projection_ff;
   right / Trl != NULL: a fisheye-stereo current frame, the arrays of orc_search_by_projection_ff_fisheye.
   has_mp: 0 = no map point, 1 = a map point, 2 = a map point flagged in mvbOutlier.  Tcw / Tlw 4 x 4, Trl 3 x 4, row-major. */
int refm_search_by_projection_ff(const refm_frame *left, const refm_frame *right, int nLast, const uint8_t *has_mp, const float *Xw,
                                 const uint8_t *mpdesc, const int32_t *lastOctave, const float *lastAngle, const uint8_t *qobs, const float *Tcw,
                                 const float *Tlw, const float *Trl, int camType, const float *camParams, float mb, float mbf, float th, int bMono,
                                 int checkOri, int32_t *slot, uint8_t *slot_obs) {
  const Camera cam(camType, camParams);
  if (!cam.get()) return -1;
  Frame Cur, Last;
  build_frame(Cur, *left, right);
  Cur.mTcw = matrix(Tcw, 4, 4, 4);
  Cur.mb = mb; Cur.mbf = mbf;
  Cur.mpCamera = cam.get();
  if (right) Cur.mTrl = matrix(Trl, 3, 4, 4);
  Points pts;
  slots_in(Cur, pts, slot, slot_obs);
  Last.N = nLast;
  Last.mTcw = matrix(Tlw, 4, 4, 4);
  Last.mvKeys.resize((size_t)nLast);
  Last.mvpMapPoints.assign((size_t)nLast, (MapPoint *)NULL);
  Last.mvbOutlier.assign((size_t)nLast, false);
  for (int i = 0; i < nLast; i++) {
    Last.mvKeys[i].octave = lastOctave[i];
    Last.mvKeys[i].angle = lastAngle[i];
    if (!has_mp[i]) continue;
    Point *p = pts.make(i, qobs ? (qobs[i] ? 1 : 0) : 1);
    p->position(Xw + 3 * (size_t)i);
    p->descriptor(mpdesc + 32 * (size_t)i);
    Last.mvpMapPoints[i] = p;
    Last.mvbOutlier[i] = has_mp[i] == 2;
  }
  Last.mvKeysUn = Last.mvKeys;
  ORBmatcher matcher(0.9f, checkOri != 0);
  const int n = matcher.SearchByProjection(Cur, Last, th, bMono != 0);
  slots_out(Cur.mvpMapPoints, slot, slot_obs);
  return n;
}

/* SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound, th, ORBdist) (:2291), the arrays of
   orc_search_by_projection_kf.  state: 0 = no map point, 1 = a map point, 2 = a bad one, 3 = one that is in sAlreadyFound. */
int refm_search_by_projection_kf(const refm_frame *cur, int nKF, const uint8_t *state, const float *Xw, const uint8_t *mpdesc, const float *kfAngle,
                                 const float *maxDist, const float *minDist, const float *Tcw, int camType, const float *camParams, float th,
                                 int ORBdist, int checkOri, int32_t *slot, uint8_t *slot_obs) {
  const Camera cam(camType, camParams);
  if (!cam.get()) return -1;
  Frame Cur, Fk;
  build_frame(Cur, *cur, NULL);
  Cur.mTcw = matrix(Tcw, 4, 4, 4);
  Cur.mpCamera = cam.get();
  Points pts;
  slots_in(Cur, pts, slot, slot_obs);
  std::set<MapPoint *> found;
  Fk.N = nKF;
  Fk.mvKeysUn.resize((size_t)nKF);
  Fk.mvpMapPoints.assign((size_t)nKF, (MapPoint *)NULL);
  for (int i = 0; i < nKF; i++) {
    Fk.mvKeysUn[i].angle = kfAngle[i];
    if (!state[i]) continue;
    Point *p = pts.make(i, 1);
    p->position(Xw + 3 * (size_t)i);
    p->descriptor(mpdesc + 32 * (size_t)i);
    p->distances(maxDist[i], minDist[i]);
    p->bad(state[i] == 2);
    if (state[i] == 3) found.insert(p);
    Fk.mvpMapPoints[i] = p;
  }
  Fk.mvKeys = Fk.mvKeysUn;
  KeyFrame KF(Fk, NULL, NULL);
  ORBmatcher matcher(0.9f, checkOri != 0);
  const int n = matcher.SearchByProjection(Cur, &KF, found, th, ORBdist);
  slots_out(Cur.mvpMapPoints, slot, slot_obs);
  return n;
}

/* SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (:273), the records of orc_search_by_bow_kf_frame_stereo.  Nleft = F.Nleft;
   kfNleft = pKF->NLeft (!= -1 gives the keyframe a second camera, so that its angles come from mvKeys / mvKeysRight).
   KF->has_mp: 0 = none, 1 = a map point, 2 = a bad one.  matchF[F.N] = the keyframe keypoint whose point the frame keypoint got. */
int refm_search_by_bow(const refm_keyframe *KFrec, const refm_keyframe *Frec, int Nleft, int kfNleft, float nnratio, int checkOri, int32_t *matchF) {
  const float pin[4] = {1.f, 1.f, 0.f, 0.f};
  const Camera second(0, pin); /* only its address is read: `!pKF->mpCamera2`, `!F.mpCamera2` */
  Points pts;
  Frame Fk, F;
  build_bow_frame(Fk, *KFrec, kfNleft, &pts, second.get());
  build_bow_frame(F, *Frec, Nleft, NULL, second.get());
  KeyFrame KF(Fk, NULL, NULL);
  std::vector<MapPoint *> matches;
  ORBmatcher matcher(nnratio, checkOri != 0);
  const int n = matcher.SearchByBoW(&KF, F, matches);
  if ((int)matches.size() != F.N) return -2;
  slots_out(matches, matchF, NULL);
  return n;
}

/* SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) (:722), the arrays of orc_search_for_initialization.
   prevMatched [n1][2] in / out. */
int refm_search_for_initialization(int n1, const int32_t *octave1, const float *angle1, const uint8_t *desc1, const refm_frame *F2rec,
                                   float *prevMatched, int windowSize, float nnratio, int checkOri, int32_t *vnMatches12) {
  Frame F1, F2;
  build_frame(F2, *F2rec, NULL);
  F1.N = n1;
  F1.mvKeysUn.resize((size_t)n1);
  for (int i = 0; i < n1; i++) { F1.mvKeysUn[i].octave = octave1[i]; F1.mvKeysUn[i].angle = angle1[i]; }
  F1.mvKeys = F1.mvKeysUn;
  F1.mDescriptors.create(std::max(n1, 1), 32, CV_8U);
  descriptors(F1.mDescriptors, 0, desc1, n1);
  std::vector<cv::Point2f> prev((size_t)n1);
  for (int i = 0; i < n1; i++) prev[i] = cv::Point2f(prevMatched[2 * i], prevMatched[2 * i + 1]);
  std::vector<int> m12;
  ORBmatcher matcher(nnratio, checkOri != 0);
  const int n = matcher.SearchForInitialization(F1, F2, prev, m12, windowSize);
  if ((int)m12.size() != n1) return -2;
  for (int i = 0; i < n1; i++) {
    vnMatches12[i] = m12[i];
    prevMatched[2 * i] = prev[i].x; prevMatched[2 * i + 1] = prev[i].y;
  }
  return n;
}

}  // extern "C"
