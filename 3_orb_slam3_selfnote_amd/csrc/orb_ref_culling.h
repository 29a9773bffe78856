// orb_ref_culling.h -- the body of LocalMapping::KeyFrameCulling's loop (LocalMapping.cc:1204-1266) and what KeyFrame::SetBadFlag
// (KeyFrame.cc:670-677) does, through MapPoint::EraseObservation (MapPoint.cc:168-202) and MapPoint::SetBadFlag (MapPoint.cc:217-226),
// to the three things that loop reads: Observations(), GetObservations() and isBad() of a map point.  Stated once for the host entry
// orbm_keyframe_culling_host and the kernels of orb_culling_kernels.h; held against the literal model of tests/keyframe_culling_model.py.
// Integer compares, two float compares (:1217) and one float product with one float compare (:1266); no contraction, no libm call.
//
// The tables (include/orbhip.h, orbm_culling_t): a row is one keypoint of one local keyframe, an entry is one (keyframe, map point) pair
// of mObservations.  An entry is LIVE while its obs_kf is not CULL_DEAD and its point is not bad: a bad point's mObservations is empty
// (MapPoint.cc:225), so the entries of a point that is bad at loop entry are never read either.
#pragma once
#include <stdint.h>

#define ORB_REF __host__ __device__ __forceinline__

#define CULL_TH_OBS 3      // `int nObs = 3; const int thObs=nObs;` (:1204-1205)
#define CULL_DEAD (-2)     // obs_kf of an erased entry; -1 is a live observer outside the list

// :1210-1219: `pMP`, `!pMP->isBad()`, and where the call is not monocular `mvDepth[i]>mThDepth || mvDepth[i]<0` skips the row
ORB_REF bool cull_row_counts(int point, bool point_bad, bool mono, float depth, float th_depth) {
  if (point < 0 || point_bad) return false;
  if (!mono && (depth > th_depth || depth < 0)) return false;
  return true;                                   // `nMPs++` (:1221)
}
// `pMP->Observations()>thObs` (:1222): only then the observations are walked
ORB_REF bool cull_walks_entries(int n_obs) { return n_obs > CULL_TH_OBS; }
// :1232 `pKFi==pKF` skips the keyframe's own entry, :1250 `scaleLeveli<=scaleLevel+1`
ORB_REF bool cull_entry_hits(int obs_kf, int k, int obs_level, int row_level) {
  return obs_kf != CULL_DEAD && obs_kf != k && obs_level <= row_level + 1;
}
// `nObs>thObs` (:1253, :1257); the break at the fourth hit changes nothing
ORB_REF bool cull_redundant(int hits) { return hits > CULL_TH_OBS; }
// `nRedundantObservations>redundant_th*nMPs` (:1266): int * float is a float product, the int on the left is converted to float
ORB_REF bool cull_test(int n_red, float redundant_th, int n_mps) { return (float)n_red > redundant_th * (float)n_mps; }
// MapPoint.cc:179-187 `nObs-=2` / `nObs--`, then :195 `if(nObs<=2) bBad=true`
ORB_REF int cull_erased_n_obs(int n_obs, int w) { return n_obs - w; }
ORB_REF bool cull_turns_bad(int n_obs) { return n_obs <= 2; }

#undef ORB_REF

// The whole loop on the host, one object at a time in the loop's order (orbm_keyframe_culling_host, and the statement the kernels equal).
// bad / n_obs / obs_kf are the caller's mutable copies; obs_kf of an erased entry becomes CULL_DEAD.
struct CullTables {
  int K; const uint8_t *skip; const float *th_depth; const int32_t *row_start, *row_point, *row_level; const float *row_depth;
  const int32_t *obs_start, *obs_level; const uint8_t *obs_w; bool mono; float redundant_th;
};
static inline void cull_counts_host(const CullTables &T, int k, const uint8_t *bad, const int32_t *n_obs, const int32_t *obs_kf, int *n_mps, int *n_red) {
  int mps = 0, red = 0;
  for (int i = T.row_start[k]; i < T.row_start[k + 1]; i++) {
    const int p = T.row_point[i];
    if (!cull_row_counts(p, p >= 0 && bad[p], T.mono, T.mono ? 0.f : T.row_depth[i], T.th_depth[k])) continue;
    mps++;
    if (!cull_walks_entries(n_obs[p])) continue;
    int hits = 0;
    for (int e = T.obs_start[p]; e < T.obs_start[p + 1]; e++) hits += cull_entry_hits(obs_kf[e], k, T.obs_level[e], T.row_level[i]);
    red += cull_redundant(hits);
  }
  *n_mps = mps; *n_red = red;
}
static inline void cull_erase_host(const CullTables &T, int c, uint8_t *bad, int32_t *n_obs, int32_t *obs_kf) {
  for (int i = T.row_start[c]; i < T.row_start[c + 1]; i++) {       // KeyFrame.cc:670-677, in row order
    const int p = T.row_point[i];
    if (p < 0 || bad[p]) continue;                                   // a bad point holds no entries
    for (int e = T.obs_start[p]; e < T.obs_start[p + 1]; e++) {
      if (obs_kf[e] != c) continue;                                  // `mObservations.count(pKF)` (MapPoint.cc:173)
      n_obs[p] = cull_erased_n_obs(n_obs[p], T.obs_w[e]);
      obs_kf[e] = CULL_DEAD;                                         // `mObservations.erase(pKF)` (:189)
      if (cull_turns_bad(n_obs[p])) bad[p] = 1;                      // MapPoint::SetBadFlag: mbBad, mObservations.clear()
      break;
    }
  }
}
