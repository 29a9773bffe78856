// orb_culling_kernels.h -- LocalMapping::KeyFrameCulling (LocalMapping.cc:1158-1310) on the device: orbm_keyframe_culling and
// orbm_keyframe_culling_open / _step.  Every compare is a function of orb_ref_culling.h, the host's own statement.
//
//   k_cull_count  grid (tile of 256 rows, keyframe): the LOOP-ENTRY status of every row (bit 0 counts in nMPs, bit 1 redundant) into
//                 row_stat, and the per-keyframe sums by ballot counts and one vector atomic per wavefront and sum.
//   k_cull_walk   one workgroup runs the sequential loop (SEQUENTIAL CULLING RULE, include/orbhip.h).  Until a keyframe has been erased
//                 a decision is the entry sums alone.  An erase walks the culled keyframe's rows, claims the keyframe's entry of each
//                 point with one compare-and-swap (two rows that hold the point find one entry: one of them wins), lowers n_obs, may
//                 turn the point bad and marks it touched.  A later keyframe re-evaluates only its rows with a touched point and adds the
//                 difference to its entry sums.
//
// One row's list: a lane walks its own row's list while it has at most CULL_LANE_MAX entries (with about ten observations per point 64
// rows advance together); rows with longer lists are taken one after the other by the whole wavefront in 64-entry tiles with a ballot
// count, so there is no cap on the entries of a point.  Both forms stop at the fourth hit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "orb_ref_culling.h"

#ifndef CULL_LANE_MAX   // measurements build it with 0 (every list by the wavefront) and with a huge value (every list by its lane)
#define CULL_LANE_MAX 64
#endif
#define CULL_WALK_THREADS 1024

struct CullParams {
  int K;
  const uint8_t *skip, *erasable;     // [K]
  const float *th_depth;              // [K]
  const int32_t *row_start;           // [K + 1]
  const int32_t *row_point, *row_level;   // [R]
  const float *row_depth;             // [R], not read when mono
  const int32_t *obs_start;           // [P + 1]
  const int32_t *obs_level;           // [E]
  const uint8_t *obs_w;               // [E]
  int mono; float redundant_th;
  // state the loop changes
  uint8_t *bad;                       // [P]
  int32_t *n_obs;                     // [P]
  int32_t *obs_kf;                    // [E], CULL_DEAD once erased
  uint8_t *touched;                   // [P] the point's state differs from loop entry
  // loop-entry status
  uint8_t *row_stat;                  // [R]
  int32_t *sum_mps, *sum_red;         // [K]
};

struct CullWalkParams {
  int k_begin;          // first keyframe of this launch
  int erase_first;      // a keyframe to erase before walking (the stepwise form's `applied`), or -1
  int any_erased;       // an erase has been applied in an earlier launch
  int stop_at_pass;     // 1: the stepwise form, return at the first unskipped keyframe that passes; 0: the one-call form
  int32_t *n_mps, *n_red;   // [K] written for every keyframe walked
  uint8_t *culled;      // [K] one-call form
  int32_t *result;      // [1] the passing keyframe's index, or K
};

// Status of row i of keyframe k from the current state: bit 0 counts in nMPs, bit 1 redundant.  Called by all 64 lanes of a wavefront
// together (active = this lane has a row); the long lists are walked by the wavefront.
__device__ __forceinline__ int cull_row_status(const CullParams &P, int k, int i, bool active) {
  const int lane = threadIdx.x & 63;
  int stat = 0, s0 = 0, s1 = 0, level = 0;
  bool is_long = false;
  if (active) {
    const int p = P.row_point[i];
    const bool bad = p >= 0 && P.bad[p] != 0;
    if (cull_row_counts(p, bad, P.mono != 0, P.mono ? 0.f : P.row_depth[i], P.th_depth[k])) {
      stat = 1;
      if (cull_walks_entries(P.n_obs[p])) {
        s0 = P.obs_start[p]; s1 = P.obs_start[p + 1]; level = P.row_level[i];
        if (s1 - s0 > CULL_LANE_MAX) is_long = true;
        else {
          int hits = 0;
          for (int e = s0; e < s1 && !cull_redundant(hits); e += 4) {   // four entries' loads in flight: the walk is a chain of latencies
            int kf[4], lv[4];
#pragma unroll
            for (int j = 0; j < 4; j++) { const int ee = min(e + j, s1 - 1); kf[j] = P.obs_kf[ee]; lv[j] = P.obs_level[ee]; }
#pragma unroll
            for (int j = 0; j < 4; j++) hits += e + j < s1 && cull_entry_hits(kf[j], k, lv[j], level);
          }
          if (cull_redundant(hits)) stat = 3;
        }
      }
    }
  }
  unsigned long long longs = __ballot(is_long);
  while (longs) {
    const int src = (int)__builtin_ctzll(longs);
    longs &= longs - 1;
    const int b0 = __builtin_amdgcn_readlane(s0, src), b1 = __builtin_amdgcn_readlane(s1, src), lv = __builtin_amdgcn_readlane(level, src);
    int hits = 0;
    for (int base = b0; base < b1 && !cull_redundant(hits); base += 64) {
      const int e = base + lane;
      const bool hit = e < b1 && cull_entry_hits(P.obs_kf[e], k, P.obs_level[e], lv);
      hits += __popcll(__ballot(hit));
    }
    if (lane == src && cull_redundant(hits)) stat = 3;
  }
  return stat;
}

__global__ __launch_bounds__(256) void k_cull_count(CullParams P) {
  const int k = blockIdx.y;
  if (P.skip[k]) return;                                         // :1200: no counts
  const int r0 = P.row_start[k], r1 = P.row_start[k + 1];
  const int i = r0 + blockIdx.x * 256 + threadIdx.x;
  if (r0 + (int)blockIdx.x * 256 >= r1) return;                  // wave-uniform: the whole block lies behind the keyframe's rows
  const bool active = i < r1;
  const int stat = cull_row_status(P, k, i, active);
  if (active) P.row_stat[i] = (uint8_t)stat;
  const int mps = __popcll(__ballot((stat & 1) != 0)), red = __popcll(__ballot((stat & 2) != 0));
  if ((threadIdx.x & 63) == 0) {
    if (mps) atomicAdd(P.sum_mps + k, mps);
    if (red) atomicAdd(P.sum_red + k, red);
  }
}

// KeyFrame::SetBadFlag's loop over mvpMapPoints (KeyFrame.cc:670-677) for keyframe c, by the whole workgroup
__device__ __forceinline__ void cull_erase(const CullParams &P, int c) {
  const int r1 = P.row_start[c + 1];
  for (int i = P.row_start[c] + (int)threadIdx.x; i < r1; i += CULL_WALK_THREADS) {
    const int p = P.row_point[i];
    if (p < 0 || P.bad[p]) continue;                             // a second row of p may see the winner's bad[p] or not: it loses the claim either way
    const int s1 = P.obs_start[p + 1];
    for (int e = P.obs_start[p]; e < s1; e++) {
      if (P.obs_kf[e] != c) continue;
      if (atomicCAS(P.obs_kf + e, c, CULL_DEAD) == c) {          // the one row that erases this point
        const int n = cull_erased_n_obs(P.n_obs[p], P.obs_w[e]);
        P.n_obs[p] = n;
        if (cull_turns_bad(n)) P.bad[p] = 1;
        P.touched[p] = 1;
      }
      break;
    }
  }
  __syncthreads();                                               // the workgroup's own stores, visible to all of it
}

__global__ __launch_bounds__(CULL_WALK_THREADS) void k_cull_walk(CullParams P, CullWalkParams W) {
  __shared__ int s_mps, s_red;
  const int lane = threadIdx.x & 63;
  bool any = W.any_erased != 0;
  if (W.erase_first >= 0) { cull_erase(P, W.erase_first); any = true; }
  for (int k = W.k_begin; k < P.K; k++) {
    if (P.skip[k]) {
      if (threadIdx.x == 0) { W.n_mps[k] = 0; W.n_red[k] = 0; if (W.culled) W.culled[k] = 0; }
      continue;
    }
    int mps = P.sum_mps[k], red = P.sum_red[k];
    if (any) {
      if (threadIdx.x == 0) { s_mps = 0; s_red = 0; }
      __syncthreads();
      const int r0 = P.row_start[k], r1 = P.row_start[k + 1];
      for (int base = r0 + (int)(threadIdx.x & ~63u); base < r1; base += CULL_WALK_THREADS) {   // wave-uniform bounds
        const int i = base + lane;
        bool active = false;
        if (i < r1) { const int p = P.row_point[i]; active = p >= 0 && P.touched[p] != 0; }
        if (!__ballot(active)) continue;
        const int now = cull_row_status(P, k, i, active), was = active ? (int)P.row_stat[i] : 0;
        const int dm = __popcll(__ballot((now & 1) != 0)) - __popcll(__ballot((was & 1) != 0));
        const int dr = __popcll(__ballot((now & 2) != 0)) - __popcll(__ballot((was & 2) != 0));
        if (lane == 0) { if (dm) atomicAdd(&s_mps, dm); if (dr) atomicAdd(&s_red, dr); }
      }
      __syncthreads();
      mps += s_mps; red += s_red;
      __syncthreads();                                           // all have read the sums before the next keyframe clears them
    }
    const bool pass = cull_test(red, P.redundant_th, mps);
    if (threadIdx.x == 0) { W.n_mps[k] = mps; W.n_red[k] = red; }
    if (pass && W.stop_at_pass) {
      if (threadIdx.x == 0) *W.result = k;
      return;
    }
    const bool cull = pass && P.erasable[k] != 0;                // mbNotErase: SetBadFlag returns without erasing (KeyFrame.cc:650-655)
    if (threadIdx.x == 0 && W.culled) W.culled[k] = cull;
    if (cull) { cull_erase(P, k); any = true; }
  }
  if (threadIdx.x == 0) *W.result = P.K;
}
