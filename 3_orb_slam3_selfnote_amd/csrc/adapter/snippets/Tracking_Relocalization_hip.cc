// Tracking_Relocalization_hip.cc -- the BoW searches of bool Tracking::Relocalization() (src/Tracking.cc:3796-3816) as ONE call for
// all relocalisation candidates (orbm_search_by_bow_candidates) instead of one ORBmatcher::SearchByBoW(pKF, mCurrentFrame, ...) call -
// one staging of the frame's descriptors, one launch, one download, one synchronisation - per candidate.
//
// A helper class, not a member of ORBmatcher.  Add this file to the library's sources and make one edit in src/Tracking.cc
// (INTEGRATION.md): in front of the loop at :3796
//     RelocalizationBoW bow(vpCandidateKFs, mCurrentFrame, 0.75f, true, vvpMapPointMatches);
// and inside it, in place of the call at :3803,
//     int nmatches = bow.nmatches[i];
// The loop keeps its own statements: the isBad() test that sets vbDiscarded[i], `nmatches < 15`, the MLPnPsolver set-up.
//
// Why the searches may be made before the loop - the INDEPENDENCE RULE of include/orbhip.h: each search writes only its own
// vvpMapPointMatches[i], and nothing the loop body does (a flag, a solver built from the frame and that vector) is read by a later
// search.  A candidate that isBad() when the helper runs is skipped (its vector stays empty and its count 0), which is the reference's
// `continue`; isBad() is read once here and once by the loop, as the reference reads it once.
#include <list>   // Map.h names std::list without including it
#include <vector>

#include "Tracking.h"
#include "ORBmatcher.h"
#include "SearchByBoW_candidates_hip.h"

namespace ORB_SLAM3 {

struct RelocalizationBoW {
  std::vector<int> nmatches;   // per candidate: what matcher.SearchByBoW(pKF, F, vvpMapPointMatches[i]) returns; 0 for a bad one

  RelocalizationBoW(const std::vector<KeyFrame *> &vpCandidateKFs, Frame &F, float nnratio, bool checkOri,
                    std::vector<std::vector<MapPoint *> > &vvpMapPointMatches)
      : nmatches(vpCandidateKFs.size(), 0) {
    using namespace bow_candidates;
    const size_t K = vpCandidateKFs.size();
    if (K == 0) return;
    std::vector<Flat> flat(K);
    std::vector<std::vector<MapPoint *> > mps(K);
    std::vector<orbm_keyframe_t> tab(K);
    std::vector<uint8_t> skip(K, 0);
    for (size_t i = 0; i < K; i++) {
      KeyFrame *pKF = vpCandidateKFs[i];
      if (pKF->isBad()) { skip[i] = 1; std::memset(&tab[i], 0, sizeof(tab[i])); continue; }              // :3799-3800
      if ((F.Nleft != -1) != (pKF->mpCamera2 != NULL)) throw std::logic_error("Tracking::Relocalization: frame and keyframe from different camera rigs");
      mps[i] = pKF->GetMapPointMatches();
      flat[i].keyframe_against_frame(pKF, mps[i]);
      tab[i] = flat[i].k;
    }
    Flat frame;
    frame.frame(F);
    std::vector<int32_t> rows(K * (size_t)F.N + 1, -1), counts(K, 0);
    checked(orbm_search_by_bow_candidates(matcher(), (int)K, tab.data(), &frame.k, F.Nleft, skip.data(), nnratio, checkOri ? 1 : 0, rows.data(),
                                          counts.data()),
            "Tracking::Relocalization");
    for (size_t i = 0; i < K; i++) {
      if (skip[i]) continue;
      vvpMapPointMatches[i].assign(F.N, static_cast<MapPoint *>(NULL));                                   // ORBmatcher.cc:277
      const int32_t *row = &rows[i * (size_t)F.N];
      for (int k = 0; k < F.N; k++)
        if (row[k] >= 0) vvpMapPointMatches[i][k] = mps[i][row[k]];                                        // ORBmatcher.cc:389, :409
      nmatches[i] = counts[i];
    }
  }
};

}  // namespace ORB_SLAM3
