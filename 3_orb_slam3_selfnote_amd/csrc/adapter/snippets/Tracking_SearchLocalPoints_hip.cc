// Tracking_SearchLocalPoints_hip.cc -- drop-in body of void Tracking::SearchLocalPoints(), replacing src/Tracking.cc:3449-3539.
//
// Like the other member snippets: delete (or #if 0) those lines of src/Tracking.cc and add this file to the library's sources
// (INTEGRATION.md).  The frame's own points are marked on the host as before; then the local map is flattened and one call,
// orbm_search_local_points, runs Frame::isInFrustum (Frame.cc:572-661, with MapPoint::PredictScale through the device's glibc-exact
// logf) for every local map point and SearchByProjection(Frame&, const vector<MapPoint*>&, th, bFarPoints, thFarPoints) over them:
// no per-point host loop with five MapPoint mutex locks before the search.  The results are written back into the MapPoints and the
// frame as the reference leaves them.  Fisheye-stereo frames (Nleft != -1) go through orbm_search_local_points_fisheye: Frame::isInFrustumChecks
// (Frame.cc:1270-1343) per camera, both halves of the search (ORBmatcher.cc:44-214) and the stereo-partner writes, one call as well.
#include "Tracking.h"

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "Atlas.h"
#include "Frame.h"
#include "LocalMapping.h"
#include "MapPoint.h"
#include "ORBmatcher.h"
#include "orbhip.h"

namespace ORB_SLAM3 {

namespace {
orbm_t *local_points_matcher() {   // one handle per thread, as in ORBmatcher_hip.cc
  thread_local orbm_t *m = nullptr;
  if (!m) {
    const char *e = std::getenv("ORBHIP_DEVICE");
    m = orbm_create(e ? std::atoi(e) : 0);
    if (!m) throw std::runtime_error("Tracking::SearchLocalPoints: orbm_create failed (no usable HIP device; there is no CPU fallback)");
  }
  return m;
}

// The raw mfMaxDistance / mfMinDistance (PredictScale divides the raw value, the getters return it scaled by 1.2f / 0.8f), read
// through a pointer-to-member formed in a derived class under mMutexPos - the accessor of ORBmatcher_hip.cc.
struct MapPointRawLP : MapPoint {
  static float MapPoint::*max_distance() { return &MapPointRawLP::mfMaxDistance; }
  static float MapPoint::*min_distance() { return &MapPointRawLP::mfMinDistance; }
  static std::mutex MapPoint::*mutex_pos() { return &MapPointRawLP::mMutexPos; }
};

void vec3_of(const cv::Mat &M, float *o) { for (int r = 0; r < 3; r++) o[r] = M.at<float>(r); }
}  // namespace

void Tracking::SearchLocalPoints() {
  // Do not search map points already matched (:3453-3471)
  for (std::vector<MapPoint *>::iterator vit = mCurrentFrame.mvpMapPoints.begin(), vend = mCurrentFrame.mvpMapPoints.end(); vit != vend; vit++) {
    MapPoint *pMP = *vit;
    if (!pMP) continue;
    if (pMP->isBad()) {
      *vit = static_cast<MapPoint *>(NULL);
    } else {
      pMP->IncreaseVisible();
      pMP->mnLastFrameSeen = mCurrentFrame.mnId;
      pMP->mbTrackInView = false;
      pMP->mbTrackInViewR = false;
    }
  }

  // The search threshold (:3508-3534)
  float th = 1;
  if (mSensor == System::RGBD) th = 3;
  if (mpAtlas->isImuInitialized()) {
    if (mpAtlas->GetCurrentMap()->GetIniertialBA2()) th = 2;
    else th = 3;
  } else if (!mpAtlas->isImuInitialized() && (mSensor == System::IMU_MONOCULAR || mSensor == System::IMU_STEREO)) {
    th = 10;
  }
  if (mCurrentFrame.mnId < mnLastRelocFrameId + 2) th = 5;
  if (mState == LOST || mState == RECENTLY_LOST) th = 15;

  // Flatten the local map (Tracking::mvpLocalMapPoints) and the frame
  const int nmp = (int)mvpLocalMapPoints.size();
  if (nmp == 0) return;
  std::vector<uint8_t> eligible(nmp, 0), mpdesc((size_t)nmp * 32, 0), obs(nmp, 0), in_view(nmp, 0);
  std::vector<float> Xw((size_t)nmp * 3, 0.f), normal((size_t)nmp * 3, 0.f), dmax(nmp, 0.f), dmin(nmp, 0.f);
  std::vector<float> px(nmp), py(nmp), pxr(nmp), depth(nmp), vcos(nmp);
  std::vector<int32_t> level(nmp), match(nmp);
  for (int i = 0; i < nmp; i++) {
    MapPoint *pMP = mvpLocalMapPoints[i];
    if (pMP->mnLastFrameSeen == mCurrentFrame.mnId || pMP->isBad()) continue;   // :3483-3487
    eligible[i] = 1;
    vec3_of(pMP->GetWorldPos(), &Xw[3 * i]);
    vec3_of(pMP->GetNormal(), &normal[3 * i]);
    {
      std::unique_lock<std::mutex> lock(pMP->*MapPointRawLP::mutex_pos());
      dmax[i] = pMP->*MapPointRawLP::max_distance();
      dmin[i] = pMP->*MapPointRawLP::min_distance();
    }
    std::memcpy(&mpdesc[32 * (size_t)i], pMP->GetDescriptor().ptr<uint8_t>(), 32);
    obs[i] = pMP->Observations() > 0;
  }
  float Tcw[16];
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) Tcw[r * 4 + c] = mCurrentFrame.mTcw.at<float>(r, c);
  std::vector<int32_t> slot(mCurrentFrame.N, -1);
  std::vector<uint8_t> slot_obs(mCurrentFrame.N, 0);
  for (int i = 0; i < mCurrentFrame.N; i++)   // pre-existing holders: an id no local map point has
    if (mCurrentFrame.mvpMapPoints[i]) { slot[i] = 1 << 30; slot_obs[i] = mCurrentFrame.mvpMapPoints[i]->Observations() > 0; }
  if (mCurrentFrame.Nleft != -1) {   // fisheye stereo: Frame::isInFrustumChecks per camera (Frame.cc:650-660, :1270-1343), ORBmatcher.cc:44-214
    Frame &F = mCurrentFrame;
    std::vector<orbx_keypoint_t> keys((size_t)F.N);   // raw keypoints [mvKeys ; mvKeysRight] (GetFeaturesInArea, Frame.cc:791-793)
    if (F.Nleft > 0) std::memcpy(keys.data(), F.mvKeys.data(), sizeof(orbx_keypoint_t) * (size_t)F.Nleft);
    if (F.N > F.Nleft) std::memcpy(keys.data() + F.Nleft, F.mvKeysRight.data(), sizeof(orbx_keypoint_t) * (size_t)(F.N - F.Nleft));
    std::vector<int32_t> l2r(F.mvLeftToRightMatch.begin(), F.mvLeftToRightMatch.end()), r2l(F.mvRightToLeftMatch.begin(), F.mvRightToLeftMatch.end());
    l2r.resize((size_t)F.Nleft, -1);
    r2l.resize((size_t)(F.N - F.Nleft), -1);
    float Trl[12], tlr[3];
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 4; c++) Trl[r * 4 + c] = F.mTrl.at<float>(r, c);
      tlr[r] = F.mTlr.at<float>(r, 3);                 // mTlr.rowRange(0,3).col(3), Frame.cc:1280
    }
    const int ct = (int)F.mpCamera->GetType(), ct2 = (int)F.mpCamera2->GetType();
    float cp[8] = {0.f}, cp2[8] = {0.f};
    for (int k = 0; k < (ct == 0 ? 4 : 8); k++) cp[k] = F.mpCamera->getParameter(k);
    for (int k = 0; k < (ct2 == 0 ? 4 : 8); k++) cp2[k] = F.mpCamera2->getParameter(k);   // Frame.cc:1299
    std::vector<uint8_t> in_view_r(nmp, 0);
    std::vector<float> pyr(nmp), depth_r(nmp), vcos_r(nmp);
    std::vector<int32_t> level_r(nmp);
    for (int i = 0; i < nmp; i++) depth[i] = mvpLocalMapPoints[i]->mTrackDepth;   // in/out: the far-point test reads it where the left check fails (ORBmatcher.cc:56)
    orbm_frame_t f;
    f.n = F.N;
    f.keys_un = keys.data();
    f.descriptors = F.mDescriptors.data;
    f.u_right = nullptr;
    f.min_x = Frame::mnMinX; f.max_x = Frame::mnMaxX; f.min_y = Frame::mnMinY; f.max_y = Frame::mnMaxY;
    const orbm_local_map_t map = {nmp, eligible.data(), Xw.data(), normal.data(), dmax.data(), dmin.data(), mpdesc.data(), obs.data(), Tcw};
    const orbm_track_rig_t track = {in_view.data(), in_view_r.data(), px.data(), py.data(), depth.data(), vcos.data(), pxr.data(), pyr.data(),
                                    depth_r.data(), vcos_r.data(), level.data(), level_r.data()};
    const int rc = orbm_search_local_points_fisheye(local_points_matcher(), &f, F.Nleft, l2r.data(), r2l.data(), F.mvScaleFactors.data(), F.mnScaleLevels,
                                                    F.mfLogScaleFactor, &map, Trl, tlr, ct, cp, ct2, cp2, 0.5f, th, mpLocalMapper->mbFarPoints ? 1 : 0,
                                                    mpLocalMapper->mThFarPoints, 0.8f, slot.data(), slot_obs.data(), nullptr, &track);
    if (rc < 0) throw std::runtime_error(std::string("Tracking::SearchLocalPoints (liborbhip): ") + orbm_last_error(local_points_matcher()));
    // Write back what isInFrustum leaves behind for Nleft != -1 (Frame.cc:651-657, :1327-1340) and Tracking.cc:3490-3501
    for (int i = 0; i < nmp; i++) {
      if (!eligible[i]) continue;
      MapPoint *pMP = mvpLocalMapPoints[i];
      pMP->mbTrackInView = in_view[i] != 0;
      pMP->mbTrackInViewR = in_view_r[i] != 0;
      pMP->mnTrackScaleLevel = level[i];
      pMP->mnTrackScaleLevelR = level_r[i];
      if (in_view[i]) { pMP->mTrackProjX = px[i]; pMP->mTrackProjY = py[i]; pMP->mTrackViewCos = vcos[i]; pMP->mTrackDepth = depth[i]; }
      if (in_view_r[i]) { pMP->mTrackProjXR = pxr[i]; pMP->mTrackProjYR = pyr[i]; pMP->mTrackViewCosR = vcos_r[i]; pMP->mTrackDepthR = depth_r[i]; }
      if (in_view[i] || in_view_r[i]) pMP->IncreaseVisible();
      if (in_view[i]) F.mmProjectPoints[pMP->mnId] = cv::Point2f(pMP->mTrackProjX, pMP->mTrackProjY);
    }
    for (int k = 0; k < F.N; k++)   // slots this call filled, stereo partners included (ORBmatcher.cc:130-133, :200-206), hold a local-map index
      if (slot[k] >= 0 && slot[k] < nmp) F.mvpMapPoints[k] = mvpLocalMapPoints[slot[k]];
    return;
  }
  orbm_frame_t f;
  f.n = mCurrentFrame.N;
  f.keys_un = reinterpret_cast<const orbx_keypoint_t *>(mCurrentFrame.mvKeysUn.data());
  f.descriptors = mCurrentFrame.mDescriptors.data;
  f.u_right = mCurrentFrame.mvuRight.empty() ? nullptr : mCurrentFrame.mvuRight.data();
  f.min_x = Frame::mnMinX; f.max_x = Frame::mnMaxX; f.min_y = Frame::mnMinY; f.max_y = Frame::mnMaxY;
  GeometricCamera *cam = mCurrentFrame.mpCamera;
  const int cam_type = (int)cam->GetType();
  float cam_params[8] = {0.f};
  for (int k = 0; k < (cam_type == 0 ? 4 : 8); k++) cam_params[k] = cam->getParameter(k);
  const orbm_local_map_t map = {nmp, eligible.data(), Xw.data(), normal.data(), dmax.data(), dmin.data(), mpdesc.data(), obs.data(), Tcw};
  const orbm_track_t track = {in_view.data(), px.data(), py.data(), pxr.data(), depth.data(), vcos.data(), level.data()};
  const int rc = orbm_search_local_points(local_points_matcher(), &f, mCurrentFrame.mvScaleFactors.data(), mCurrentFrame.mnScaleLevels,
                                          mCurrentFrame.mfLogScaleFactor, &map, cam_type, cam_params, mCurrentFrame.mbf, 0.5f, th,
                                          mpLocalMapper->mbFarPoints ? 1 : 0, mpLocalMapper->mThFarPoints, 0.8f, slot.data(), slot_obs.data(),
                                          match.data(), &track);
  if (rc < 0) throw std::runtime_error(std::string("Tracking::SearchLocalPoints (liborbhip): ") + orbm_last_error(local_points_matcher()));

  // Write back what isInFrustum and the search leave behind (Frame.cc:576-644, Tracking.cc:3490-3501, ORBmatcher.cc:124)
  for (int i = 0; i < nmp; i++) {
    if (!eligible[i]) continue;
    MapPoint *pMP = mvpLocalMapPoints[i];
    pMP->mbTrackInView = in_view[i] != 0;
    pMP->mTrackProjX = px[i];
    pMP->mTrackProjY = py[i];
    if (!in_view[i]) continue;
    pMP->mTrackProjXR = pxr[i];
    pMP->mTrackDepth = depth[i];
    pMP->mnTrackScaleLevel = level[i];
    pMP->mTrackViewCos = vcos[i];
    pMP->IncreaseVisible();
    mCurrentFrame.mmProjectPoints[pMP->mnId] = cv::Point2f(pMP->mTrackProjX, pMP->mTrackProjY);
  }
  for (int k = 0; k < mCurrentFrame.N; k++)   // slots this call filled hold a local-map index
    if (slot[k] >= 0 && slot[k] < nmp) mCurrentFrame.mvpMapPoints[k] = mvpLocalMapPoints[slot[k]];
}

}  // namespace ORB_SLAM3
