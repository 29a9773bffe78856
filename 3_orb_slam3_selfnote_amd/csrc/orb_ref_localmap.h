// orb_ref_localmap.h -- Tracking::UpdateLocalKeyFrames / UpdateLocalPoints (Tracking.cc:3559-3762) and the counter and lists of
// KeyFrame::UpdateConnections (KeyFrame.cc:407-492), stated once for the host entries orbm_update_local_map_host /
// orbm_update_connections_host and the kernels of orb_localmap_kernels.h; held against the literal model of tests/update_local_map_model.py.
// Integer compares only.  Where the reference's result depends on pointer values it depends on their ORDER alone, and kf_rank stands for
// that order (RANK RULE, include/orbhip.h).
//
// The tables (orbm_map_graph_t): keyframe g is a slot, kf_rank[g] its place in address order; a ROW is one element of a keyframe's
// mvpMapPoints, an ENTRY one element of a map point's mObservations.  The entries of a bad point are never read.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <vector>

#define ORB_REF __host__ __device__ __forceinline__

#define LM_BEST 10          // GetBestCovisibilityKeyFrames(10) (Tracking.cc:3690)
#define LM_LIMIT 80         // `mvpLocalKeyFrames.size()>80` (:3684), `<80` (:3737)
#define LM_TAIL_TRIPS 20    // `const int Nd = 20` (:3742)
#define LM_MAX_ROWS 15360   // rows of one keyframe (ORBM_MAX_KEYPOINTS): the stride of lm_point_key

// :3603-3617 / KeyFrame.cc:424-428: a slot or row votes when it holds a point that is not bad
ORB_REF bool lm_point_votes(int point, bool point_bad) { return point >= 0 && !point_bad; }
// :3614-3617 the slot of a bad point is set to NULL
ORB_REF bool lm_slot_nulled(int point, bool point_bad) { return point >= 0 && point_bad; }
// KeyFrame.cc:434 `mit->first->mnId==mnId || mit->first->isBad() || mit->first->GetMap() != mpMap`: no count
ORB_REF bool conn_entry_counts(int k, int t, bool k_bad, int k_map, int t_map) { return k != t && !k_bad && k_map == t_map; }
// :3666 / KeyFrame.cc:459 `it->second>max`: strict, so the first in iteration (rank) order keeps a tie
ORB_REF bool lm_beats(int count, int max) { return count > max; }
// :3684 at the top of every trip of the expansion
ORB_REF bool lm_expansion_stops(int size) { return size > LM_LIMIT; }
// :3737
ORB_REF bool lm_tail_runs(bool inertial, int size) { return inertial && size < LM_LIMIT; }
// KeyFrame.cc:464 `mit->second>=th`
ORB_REF bool conn_is_pair(int count, int th) { return count >= th; }
// The place of a row in UpdateLocalPoints' walk (:3566-3571): keyframes in reverse list order, rows in row order.  The smallest key of a
// point is its first occurrence.  (G + 23) * 15360 < 2^32.
ORB_REF uint32_t lm_point_key(int pos_reversed, int row) { return (uint32_t)pos_reversed * (uint32_t)LM_MAX_ROWS + (uint32_t)row; }
// rank as the high word of an ascending 64-bit sort key
ORB_REF uint64_t lm_rank_key(int32_t rank, int g) { return ((uint64_t)((uint32_t)rank ^ 0x80000000u) << 32) | (uint32_t)g; }

#undef ORB_REF

// What both members read (the fields of orbm_map_graph_t)
struct LmGraph {
  int G; const int32_t *kf_rank; const uint8_t *kf_bad; const int32_t *kf_map, *kf_row_start, *row_point, *kf_best, *kf_child_start, *kf_child,
      *kf_parent, *kf_prev;
  int P; const uint8_t *pt_bad; const int32_t *obs_start, *obs_kf;
};

// the voted keyframes in rank order: iteration of map<KeyFrame*,int>
static inline std::vector<int> lm_in_rank_order(const LmGraph &M, const std::vector<int32_t> &count) {
  std::vector<uint64_t> keys;
  for (int g = 0; g < M.G; g++) if (count[(size_t)g] > 0) keys.push_back(lm_rank_key(M.kf_rank[g], g));
  std::sort(keys.begin(), keys.end());
  std::vector<int> order;
  for (uint64_t k : keys) order.push_back((int)(uint32_t)k);
  return order;
}

// UpdateLocalKeyFrames + UpdateLocalPoints, one object at a time in the reference's order.  slot_bad [N] is written for every slot.
static inline void lm_update_local_map_host(const LmGraph &M, int N, const int32_t *frame_point, bool inertial, int last_kf, std::vector<int32_t> &local_kf,
                                            int *kf_max, int *max_votes, uint8_t *slot_bad, std::vector<int32_t> &local_point) {
  std::vector<int32_t> count((size_t)M.G, 0);
  for (int s = 0; s < N; s++) {                                                   // :3599-3619
    const int p = frame_point[s];
    const bool bad = p >= 0 && M.pt_bad[p];
    slot_bad[s] = lm_slot_nulled(p, bad);
    if (!lm_point_votes(p, bad)) continue;
    for (int e = M.obs_start[p]; e < M.obs_start[p + 1]; e++) count[(size_t)M.obs_kf[e]]++;   // :3612, no filter on the keyframe
  }
  std::vector<uint8_t> mark((size_t)M.G, 0);                                      // mnTrackReferenceForFrame == mCurrentFrame.mnId (STAMP NOTE)
  local_kf.clear();
  int max = 0, best = -1;
  for (int g : lm_in_rank_order(M, count)) {                                      // :3658-3675
    if (M.kf_bad[g]) continue;
    if (lm_beats(count[(size_t)g], max)) { max = count[(size_t)g]; best = g; }
    local_kf.push_back(g); mark[(size_t)g] = 1;
  }
  const size_t first = local_kf.size();                                           // itEndKF is taken before the loop (:3680)
  for (size_t i = 0; i < first; i++) {
    if (lm_expansion_stops((int)local_kf.size())) break;
    const int g = local_kf[i];
    for (int j = 0; j < LM_BEST; j++) {                                           // :3693-3705
      const int n = M.kf_best[(size_t)g * LM_BEST + j];
      if (n < 0) break;                                                           // the vector has ended
      if (!M.kf_bad[n] && !mark[(size_t)n]) { local_kf.push_back(n); mark[(size_t)n] = 1; break; }
    }
    for (int c = M.kf_child_start[g]; c < M.kf_child_start[g + 1]; c++) {         // :3708-3720, in set order
      const int n = M.kf_child[c];
      if (!M.kf_bad[n] && !mark[(size_t)n]) { local_kf.push_back(n); mark[(size_t)n] = 1; break; }
    }
    const int par = M.kf_parent[g];                                               // :3723-3732: no isBad test, and the break leaves the outer loop
    if (par >= 0 && !mark[(size_t)par]) { local_kf.push_back(par); mark[(size_t)par] = 1; break; }
  }
  if (lm_tail_runs(inertial, (int)local_kf.size())) {                             // :3737-3754
    int t = last_kf;
    for (int i = 0; i < LM_TAIL_TRIPS; i++) {
      if (t < 0) break;
      if (!mark[(size_t)t]) { local_kf.push_back(t); mark[(size_t)t] = 1; t = M.kf_prev[t]; }
    }
  }
  *kf_max = best; *max_votes = max;
  std::vector<uint8_t> pmark((size_t)M.P, 0);
  local_point.clear();
  for (size_t j = local_kf.size(); j-- > 0;) {                                    // :3566-3586
    const int g = local_kf[j];
    for (int r = M.kf_row_start[g]; r < M.kf_row_start[g + 1]; r++) {
      const int p = M.row_point[r];
      if (p < 0 || pmark[(size_t)p]) continue;
      if (M.pt_bad[p]) continue;
      local_point.push_back(p); pmark[(size_t)p] = 1;
    }
  }
}

// KFcounter and the two ordered vectors of UpdateConnections for target t (KeyFrame.cc:409-484).  conn_*: the counter in rank order;
// ord_*: mvpOrderedConnectedKeyFrames / mvOrderedWeights.  An empty counter leaves everything empty, kf_max -1 and nmax 0.
static inline void conn_update_host(const LmGraph &M, int t, int th, std::vector<int32_t> &conn_kf, std::vector<int32_t> &conn_w, std::vector<int32_t> &ord_kf,
                                    std::vector<int32_t> &ord_w, int *kf_max, int *nmax) {
  std::vector<int32_t> count((size_t)M.G, 0);
  for (int r = M.kf_row_start[t]; r < M.kf_row_start[t + 1]; r++) {               // :420-439
    const int p = M.row_point[r];
    if (!lm_point_votes(p, p >= 0 && M.pt_bad[p])) continue;
    for (int e = M.obs_start[p]; e < M.obs_start[p + 1]; e++) {
      const int k = M.obs_kf[e];
      if (conn_entry_counts(k, t, M.kf_bad[k], M.kf_map[k], M.kf_map[t])) count[(size_t)k]++;
    }
  }
  conn_kf.clear(); conn_w.clear(); ord_kf.clear(); ord_w.clear();
  int max = 0, best = -1;
  std::vector<uint64_t> pairs;                                                    // (weight, place in rank order): what sort(vPairs) compares
  for (int g : lm_in_rank_order(M, count)) {                                      // :455-469
    const int w = count[(size_t)g];
    if (lm_beats(w, max)) { max = w; best = g; }
    if (conn_is_pair(w, th)) pairs.push_back(((uint64_t)(uint32_t)w << 32) | (uint32_t)conn_kf.size());
    conn_kf.push_back(g); conn_w.push_back(w);
  }
  *kf_max = best; *nmax = max;
  if (conn_kf.empty()) return;                                                    // :442
  if (pairs.empty())                                                              // :471-475
    for (size_t i = 0; i < conn_kf.size(); i++) if (conn_kf[i] == best) pairs.push_back(((uint64_t)(uint32_t)max << 32) | (uint32_t)i);
  std::sort(pairs.begin(), pairs.end());                                          // :477
  for (size_t i = pairs.size(); i-- > 0;) {                                       // push_front: the sorted order reversed (:480-484)
    ord_kf.push_back(conn_kf[(size_t)(uint32_t)pairs[i]]); ord_w.push_back((int32_t)(pairs[i] >> 32));
  }
}
