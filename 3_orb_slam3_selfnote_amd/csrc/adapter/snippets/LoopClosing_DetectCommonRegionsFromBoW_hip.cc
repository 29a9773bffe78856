// LoopClosing_DetectCommonRegionsFromBoW_hip.cc -- the BoW searches of bool LoopClosing::DetectCommonRegionsFromBoW(...)
// (src/LoopClosing.cc:724-739) as ONE call for a candidate and its covisibles (orbm_search_by_bow_keyframes_candidates) instead of one
// ORBmatcher::SearchByBoW(mpCurrentKF, vpCovKFi[j], ...) call - one staging of the current keyframe, one launch, one download, one
// synchronisation - per keyframe.
//
// A helper class, not a member of ORBmatcher.  Add this file to the library's sources and make one edit in src/LoopClosing.cc
// (INTEGRATION.md): in front of the loop at :724
//     CovisibleBoW bow(mpCurrentKF, vpCovKFi, 0.9f, true, vvpMatchedMPs);
// and inside it, in place of the call at :731,
//     int num = bow.num[j];
// The loop keeps its own statements: the NULL / isBad() `continue` and the arg-max over num; the merge at :745-775 reads
// vvpMatchedMPs[j] as before.
//
// Why the searches may be made before the loop - the INDEPENDENCE RULE of include/orbhip.h: each search writes only its own
// vvpMatchedMPs[j] and the loop body changes two integers.  A keyframe that is NULL or isBad() when the helper runs is skipped: its
// vector stays empty, as the reference's `continue` leaves it.
#include <list>   // Map.h names std::list without including it
#include <vector>

#include "LoopClosing.h"
#include "ORBmatcher.h"
#include "SearchByBoW_candidates_hip.h"

namespace ORB_SLAM3 {

struct CovisibleBoW {
  std::vector<int> num;   // per keyframe: what matcherBoW.SearchByBoW(pKF1, vpKFs[j], vvpMatchedMPs[j]) returns; 0 for a skipped one

  CovisibleBoW(KeyFrame *pKF1, const std::vector<KeyFrame *> &vpKFs, float nnratio, bool checkOri, std::vector<std::vector<MapPoint *> > &vvpMatchedMPs)
      : num(vpKFs.size(), 0) {
    using namespace bow_candidates;
    const size_t K = vpKFs.size();
    if (K == 0) return;
    const std::vector<MapPoint *> mps1 = pKF1->GetMapPointMatches();
    Flat first;
    first.keyframe_against_keyframe(pKF1, mps1);
    std::vector<Flat> flat(K);
    std::vector<std::vector<MapPoint *> > mps(K);
    std::vector<orbm_keyframe_t> tab(K);
    std::vector<uint8_t> skip(K, 0);
    for (size_t j = 0; j < K; j++) {
      if (!vpKFs[j] || vpKFs[j]->isBad()) { skip[j] = 1; std::memset(&tab[j], 0, sizeof(tab[j])); continue; }   // :726-727
      mps[j] = vpKFs[j]->GetMapPointMatches();
      flat[j].keyframe_against_keyframe(vpKFs[j], mps[j]);
      tab[j] = flat[j].k;
    }
    const size_t n1 = mps1.size();
    std::vector<int32_t> rows(K * n1 + 1, -1), counts(K, 0);
    checked(orbm_search_by_bow_keyframes_candidates(matcher(), &first.k, (int)K, tab.data(), skip.data(), nnratio, checkOri ? 1 : 0, rows.data(),
                                                    counts.data()),
            "LoopClosing::DetectCommonRegionsFromBoW");
    for (size_t j = 0; j < K; j++) {
      if (skip[j]) continue;
      vvpMatchedMPs[j].assign(n1, static_cast<MapPoint *>(NULL));                                          // ORBmatcher.cc:852
      const int32_t *row = &rows[j * n1];
      for (size_t i = 0; i < n1; i++)
        if (row[i] >= 0) vvpMatchedMPs[j][i] = mps[j][row[i]];                                              // ORBmatcher.cc:927
      num[j] = counts[j];
    }
  }
};

}  // namespace ORB_SLAM3
