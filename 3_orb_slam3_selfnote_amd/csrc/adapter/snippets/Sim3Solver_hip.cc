// Sim3Solver_hip.cc -- a whole-file replacement of src/Sim3Solver.cc against the reference's unmodified include/Sim3Solver.h: every
// member the header declares is defined here.  Remove src/Sim3Solver.cc from the library's sources and add this file.
//
// What stays the reference's: the constructor's filtering of the matches (:85-110, :119-125, :134-135), SetRansacParameters' bookkeeping,
// and the drawing of the minimal sets with DUtils::Random::RandomInt in the reference's order (:199-213) - only this side of the call can
// continue libc rand()'s stream, and the library never calls rand().  Everything behind the draw - the camera coordinates and projections
// of the constructor, ComputeSim3 and CheckInliers of every iteration of the chunk, the running best - is one call per iterate
// (orbm_sim3_solve; include/orbhip.h, SIM3 RULE).
//
// One difference from the reference, stated in INTEGRATION.md: a chunk that converges at its iteration `it` has already drawn the sets of
// its later iterations, so rand() is advanced by up to 3 * (chunk - it - 1) more draws.  A chunk that does not converge draws exactly what
// the reference draws.
//
// Where the flat arrays live: the header cannot grow a member, and a solver may be copied, so a side table would not do.  The header
// declares two members that src/Sim3Solver.cc never touches, mvSigmaSquare1 / mvSigmaSquare2 (std::vector<size_t>); they carry the bytes
// of the floats the call needs: per kept pair the world position and mvLevelSigma2 entry of its map point (four floats, two size_t), and
// behind the pairs the keyframe's pose (sixteen floats).  mvX3Dc1/2 and mvP1im1/2 stay empty: the library forms them (csrc/orb_ref_sim3.h).
#include "Sim3Solver.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "Thirdparty/DBoW2/DUtils/Random.h"
#include "orbhip.h"

namespace ORB_SLAM3 {

namespace {
orbm_t *sim3_matcher() {   // one handle per thread: the solver runs on the loop-closing thread
  thread_local orbm_t *m = nullptr;
  if (!m) {
    const char *e = std::getenv("ORBHIP_DEVICE");
    m = orbm_create(e ? std::atoi(e) : 0);
    if (!m) throw std::runtime_error("Sim3Solver: orbm_create failed (no usable HIP device; there is no CPU fallback)");
  }
  return m;
}

static_assert(sizeof(size_t) == 2 * sizeof(float), "two floats per size_t");
void push_floats(std::vector<size_t> &v, const float *f, size_t pairs_of_floats) {
  for (size_t k = 0; k < pairs_of_floats; k++) {
    size_t w;
    std::memcpy(&w, f + 2 * k, sizeof(w));
    v.push_back(w);
  }
}
// [N][4] pair floats and 16 pose floats out of a carrier
void pull_floats(const std::vector<size_t> &v, int N, std::vector<float> &X, std::vector<float> &sigma2, float *Tcw) {
  std::vector<float> f(2 * v.size());
  std::memcpy(f.data(), v.data(), sizeof(size_t) * v.size());
  X.resize(3 * (size_t)N); sigma2.resize((size_t)N);
  for (int i = 0; i < N; i++) {
    std::memcpy(&X[3 * (size_t)i], &f[4 * (size_t)i], 3 * sizeof(float));
    sigma2[(size_t)i] = f[4 * (size_t)i + 3];
  }
  std::memcpy(Tcw, &f[4 * (size_t)N], 16 * sizeof(float));
}
void camera_of(GeometricCamera *cam, int32_t &type, float *params) {
  type = (int32_t)cam->GetType();
  for (int k = 0; k < (type == 0 ? 4 : 8); k++) params[k] = cam->getParameter(k);
}
}  // namespace

Sim3Solver::Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const std::vector<MapPoint *> &vpMatched12, const bool bFixScale,
                       std::vector<KeyFrame *> vpKeyFrameMatchedMP)
    : mnIterations(0), mnBestInliers(0), mbFixScale(bFixScale), pCamera1(pKF1->mpCamera), pCamera2(pKF2->mpCamera) {
  bool bDifferentKFs = false;
  if (vpKeyFrameMatchedMP.empty()) {
    bDifferentKFs = true;   // the reference's own naming: the flag is set when NO per-match keyframes were given (:48-52)
    vpKeyFrameMatchedMP = std::vector<KeyFrame *>(vpMatched12.size(), pKF2);
  }
  mpKF1 = pKF1;
  mpKF2 = pKF2;
  std::vector<MapPoint *> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
  mN1 = (int)vpMatched12.size();
  mvpMapPoints1.reserve(mN1);
  mvpMapPoints2.reserve(mN1);
  mvpMatches12 = vpMatched12;
  mvnIndices1.reserve(mN1);
  mvAllIndices.reserve(mN1);

  size_t idx = 0;
  KeyFrame *pKFm = pKF2;
  for (int i1 = 0; i1 < mN1; i1++) {
    if (!vpMatched12[i1]) continue;
    MapPoint *pMP1 = vpKeyFrameMP1[i1];
    MapPoint *pMP2 = vpMatched12[i1];
    if (!pMP1) continue;
    if (pMP1->isBad() || pMP2->isBad()) continue;
    if (bDifferentKFs) pKFm = vpKeyFrameMatchedMP[i1];
    const int indexKF1 = std::get<0>(pMP1->GetIndexInKeyFrame(pKF1));
    const int indexKF2 = std::get<0>(pMP2->GetIndexInKeyFrame(pKFm));
    if (indexKF1 < 0 || indexKF2 < 0) continue;
    const cv::KeyPoint &kp1 = pKF1->mvKeysUn[indexKF1];
    const cv::KeyPoint &kp2 = pKFm->mvKeysUn[indexKF2];
    const float sigmaSquare1 = pKF1->mvLevelSigma2[kp1.octave];
    const float sigmaSquare2 = pKFm->mvLevelSigma2[kp2.octave];
    mvnMaxError1.push_back(9.210 * sigmaSquare1);
    mvnMaxError2.push_back(9.210 * sigmaSquare2);
    mvpMapPoints1.push_back(pMP1);
    mvpMapPoints2.push_back(pMP2);
    mvnIndices1.push_back(i1);
    const cv::Mat X3D1w = pMP1->GetWorldPos(), X3D2w = pMP2->GetWorldPos();
    const float a[4] = {X3D1w.at<float>(0), X3D1w.at<float>(1), X3D1w.at<float>(2), sigmaSquare1};
    const float b[4] = {X3D2w.at<float>(0), X3D2w.at<float>(1), X3D2w.at<float>(2), sigmaSquare2};
    push_floats(mvSigmaSquare1, a, 2);
    push_floats(mvSigmaSquare2, b, 2);
    mvAllIndices.push_back(idx);
    idx++;
  }
  // the poses the reference reads at :72-75, behind the pairs
  const cv::Mat Tcw1 = pKF1->GetPose(), Tcw2 = pKF2->GetPose();
  float T1[16], T2[16];
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) { T1[4 * r + c] = Tcw1.at<float>(r, c); T2[4 * r + c] = Tcw2.at<float>(r, c); }
  push_floats(mvSigmaSquare1, T1, 8);
  push_floats(mvSigmaSquare2, T2, 8);

  mK1 = pKF1->mK;
  mK2 = pKF2->mK;
  SetRansacParameters();
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations) {
  mRansacProb = probability;
  mRansacMinInliers = minInliers;
  N = (int)mvpMapPoints1.size();
  mvbInliersi.resize(N);
  mRansacMaxIts = orbm_sim3_ransac_iterations(probability, minInliers, maxIterations, N);   // :161-171
  mnIterations = 0;
}

cv::Mat Sim3Solver::iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers) {
  bool bConverge;
  cv::Mat best = iterate(nIterations, bNoMore, vbInliers, nInliers, bConverge);
  return bConverge ? best : cv::Mat();   // the four-argument overload returns the transform on convergence only (:234, :242)
}

cv::Mat Sim3Solver::iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers, bool &bConverge) {
  bNoMore = false;
  bConverge = false;
  vbInliers = std::vector<bool>(mN1, false);
  nInliers = 0;
  if (N < mRansacMinInliers) {
    bNoMore = true;
    return cv::Mat();
  }
  // the sets of this call's iterations, :194-213: the same calls of DUtils::Random in the same order
  const int chunk = std::max(0, std::min(nIterations, mRansacMaxIts - mnIterations));
  if (chunk == 0) {
    if (mnIterations >= mRansacMaxIts) bNoMore = true;
    return cv::Mat();
  }
  std::vector<int32_t> sets((size_t)chunk * 3);
  std::vector<size_t> vAvailableIndices;
  for (int it = 0; it < chunk; it++) {
    vAvailableIndices = mvAllIndices;
    for (short i = 0; i < 3; ++i) {
      const int randi = DUtils::Random::RandomInt(0, (int)vAvailableIndices.size() - 1);
      sets[(size_t)it * 3 + i] = (int32_t)vAvailableIndices[randi];
      vAvailableIndices[randi] = vAvailableIndices.back();
      vAvailableIndices.pop_back();
    }
  }

  std::vector<float> Xw1, Xw2, sigma2_1, sigma2_2;
  float Tcw1[16], Tcw2[16], cam1[8] = {}, cam2[8] = {};
  pull_floats(mvSigmaSquare1, N, Xw1, sigma2_1, Tcw1);
  pull_floats(mvSigmaSquare2, N, Xw2, sigma2_2, Tcw2);
  std::vector<int32_t> idx1(mvnIndices1.begin(), mvnIndices1.end());
  orbm_sim3_problem_t P;
  P.n1 = mN1; P.N = N;
  P.idx1 = idx1.data(); P.Xw1 = Xw1.data(); P.Xw2 = Xw2.data(); P.sigma2_1 = sigma2_1.data(); P.sigma2_2 = sigma2_2.data();
  P.Tcw1 = Tcw1; P.Tcw2 = Tcw2;
  camera_of(pCamera1, P.cam_type1, cam1);
  camera_of(pCamera2, P.cam_type2, cam2);
  P.cam_params1 = cam1; P.cam_params2 = cam2;
  P.fix_scale = mbFixScale ? 1 : 0; P.min_inliers = mRansacMinInliers;
  P.iterations_done = mnIterations; P.max_iterations = mRansacMaxIts;
  std::vector<uint8_t> best_mask((size_t)N + 1), vb((size_t)mN1 + 1);
  orbm_sim3_result_t R;
  R.best_mask = best_mask.data(); R.vbInliers = vb.data();
  orbm_t *m = sim3_matcher();
  const int rc = orbm_sim3_solve(m, &P, chunk, sets.data(), mnBestInliers, &R, NULL);
  if (rc < 0) throw std::runtime_error(std::string("Sim3Solver::iterate: ") + orbm_last_error(m));

  mnIterations += R.it_stop;
  cv::Mat bestSim3;
  if (R.improved) {   // :219-226, :292-299
    mnBestInliers = R.best_inliers;
    mvbBestInliers.assign(N, false);
    for (int i = 0; i < N; i++) mvbBestInliers[i] = best_mask[i] != 0;
    mBestT12 = cv::Mat(4, 4, CV_32F);
    mBestRotation = cv::Mat(3, 3, CV_32F);
    mBestTranslation = cv::Mat(3, 1, CV_32F);
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) mBestT12.at<float>(r, c) = R.T12[4 * r + c];
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) mBestRotation.at<float>(r, c) = R.R12[3 * r + c];
      mBestTranslation.at<float>(r) = R.t12[r];
    }
    mBestScale = R.s12;
    bestSim3 = mBestT12;
  }
  if (R.converged) {   // :228-235, :301-309
    nInliers = R.best_inliers;
    for (int i = 0; i < mN1; i++) vbInliers[i] = vb[i] != 0;
    bConverge = true;
    return mBestT12;
  }
  if (R.no_more) bNoMore = true;
  return bestSim3;
}

cv::Mat Sim3Solver::find(std::vector<bool> &vbInliers12, int &nInliers) {
  bool bFlag;
  return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
}

cv::Mat Sim3Solver::GetEstimatedRotation() { return mBestRotation.clone(); }

cv::Mat Sim3Solver::GetEstimatedTranslation() { return mBestTranslation.clone(); }

float Sim3Solver::GetEstimatedScale() { return mBestScale; }

// The protected members below ran inside the loop of iterate; the loop is the library's now and nothing reaches them (the class has no
// friend and nothing derives from it).  They are defined because the header declares them.
void Sim3Solver::ComputeCentroid(cv::Mat &, cv::Mat &, cv::Mat &) { throw std::logic_error("Sim3Solver::ComputeCentroid runs inside orbm_sim3_solve"); }

void Sim3Solver::ComputeSim3(cv::Mat &, cv::Mat &) { throw std::logic_error("Sim3Solver::ComputeSim3 runs inside orbm_sim3_solve"); }

void Sim3Solver::CheckInliers() { throw std::logic_error("Sim3Solver::CheckInliers runs inside orbm_sim3_solve"); }

void Sim3Solver::Project(const std::vector<cv::Mat> &, std::vector<cv::Mat> &, cv::Mat, GeometricCamera *) {
  throw std::logic_error("Sim3Solver::Project runs inside orbm_sim3_solve");
}

void Sim3Solver::FromCameraToImage(const std::vector<cv::Mat> &, std::vector<cv::Mat> &, GeometricCamera *) {
  throw std::logic_error("Sim3Solver::FromCameraToImage runs inside orbm_sim3_solve");
}

}  // namespace ORB_SLAM3
