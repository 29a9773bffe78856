// orb_newpoints_kernels.h -- the geometric body of LocalMapping::CreateNewMapPoints' loop (LocalMapping.cc:605-880) on the rows the
// one-call SearchForTriangulation kernels left in device memory, and the ordered list of new map points (include/orbhip.h, SEQUENTIAL
// RULE).  The arithmetic is new_point_geometry of orb_ref_newpoints.h, the host's own definition.
#pragma once
#include "orb_match_kernels.h"
#include "orb_ref_newpoints.h"

// The body over arrays of pairs (orbm_new_point_geometry_device): one pair per lane, both keyframes' constants by value
struct NewPointPairsParams {
  orbm_new_point_camera_t c1, c2;
  const orbm_new_point_obs_t *obs1, *obs2;
  float scale_factor1, th_far_points;
  int far_points, n;
  uint8_t *status;
  float *x3d;   // [n][3], written on acceptance
};
__global__ __launch_bounds__(256) void k_new_point_pairs(NewPointPairsParams P) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P.n) return;
  P.status[i] = (uint8_t)new_point_geometry(P.c1, P.c2, P.obs1[i], P.obs2[i], P.scale_factor1, P.far_points, P.th_far_points, P.x3d + 3 * (size_t)i);
}

// One lane per (neighbour j, keypoint idx1 of the new keyframe); a lane without a match writes ORBM_NP_NO_MATCH and leaves.  The Jacobi
// sweeps of jacobi_svd4_last_row are bounded (30), so a lane cannot spin; lanes of one wavefront mix neighbours and outcomes, the
// per-keyframe constants are therefore vector loads from the table `cams` ([0] the new keyframe, [1 + j] neighbour j).
struct NewPointsParams {
  TriNbParams in;                        // block, nb, kp1, ur1, n1, matches12 of the search that ran in front
  const orbm_new_point_camera_t *cams;   // [K + 1]
  const float *stereo1;                  // [n1][3] = mvDepth, mvKeys.pt of the new keyframe, NULL when it has no stereo keypoint
  const uint64_t *stereo2;               // [K] byte offset of the same table of neighbour j in the block, ~0: none
  int K;
  float scale_factor1, th_far_points;
  int far_points;
  uint8_t *status;                       // [K][n1]
  float *x3d;                            // [K][n1][3], written on acceptance
  int32_t *first;                        // [n1] smallest neighbour with an accepted pair, pre-filled with 0x7f7f7f7f
  orbm_new_point_t *list;                // [n1]: an idx1 appears at most once
  int32_t *total;
};

__device__ __forceinline__ orbm_new_point_obs_t np_load_obs(const float *kp, const float *ur, const float *stereo, int idx, int n_left) {
  const float *k = kp + (size_t)idx * 7;
  orbm_new_point_obs_t o;
  o.x = k[0]; o.y = k[1]; o.octave = __float_as_int(k[5]);
  o.u_right = ur ? ur[idx] : -1.f;
  o.depth = 0.f; o.key_x = 0.f; o.key_y = 0.f;
  if (stereo && o.u_right >= 0) { o.depth = stereo[3 * (size_t)idx]; o.key_x = stereo[3 * (size_t)idx + 1]; o.key_y = stereo[3 * (size_t)idx + 2]; }
  o.right = n_left >= 0 && idx >= n_left;
  return o;
}

__global__ __launch_bounds__(256) void k_new_points_geometry(NewPointsParams P) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t n1 = (size_t)P.in.n1;
  if (e >= (size_t)P.K * n1) return;
  const int32_t idx2 = P.in.matches12[e];
  if (idx2 < 0) { P.status[e] = ORBM_NP_NO_MATCH; return; }
  const int j = (int)(e / n1), idx1 = (int)(e - (size_t)j * n1);
  const TriNb &N = P.in.nb[j];
  const orbm_new_point_camera_t &c1 = P.cams[0], &c2 = P.cams[1 + j];
  const uint64_t st2 = P.stereo2[j];
  const orbm_new_point_obs_t o1 = np_load_obs(P.in.kp1, P.in.ur1, P.stereo1, idx1, c1.n_left);
  const orbm_new_point_obs_t o2 = np_load_obs((const float *)(P.in.block + N.kp2), P.in.ur1 ? (const float *)(P.in.block + N.ur2) : nullptr,
                                              st2 == ~(uint64_t)0 ? nullptr : (const float *)(P.in.block + st2), idx2, c2.n_left);
  float x3D[3];
  const int st = new_point_geometry(c1, c2, o1, o2, P.scale_factor1, P.far_points, P.th_far_points, x3D);
  P.status[e] = (uint8_t)st;
  if (st != ORBM_NP_ACCEPTED) return;
  P.x3d[3 * e] = x3D[0]; P.x3d[3 * e + 1] = x3D[1]; P.x3d[3 * e + 2] = x3D[2];
  atomicMin(&P.first[idx1], j);
}

// The list in the reference's creation order (j ascending, idx1 ascending): block j emits the pairs (j, idx1) with first[idx1] == j.
// Its place in the list is the number of entries of the neighbours in front of it = #{idx1 : first[idx1] < j} (an exclusive scan of the
// per-neighbour counts, formed by every block for itself: no block waits for another), then a running prefix over its own row, 256
// keypoints at a time.  The last block also writes the total.
__global__ __launch_bounds__(256) void k_new_points_emit(NewPointsParams P) {
  const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n1 = P.in.n1;
  __shared__ int s_base, s_wave[4];
  if (tid == 0) s_base = 0;
  __syncthreads();
  int before = 0;
  for (int i = tid; i < n1; i += 256) before += P.first[i] < j;
  if (before) atomicAdd(&s_base, before);
  __syncthreads();
  int at = s_base;
  for (int c = 0; c < n1; c += 256) {
    const int idx1 = c + tid;
    const bool mine = idx1 < n1 && P.first[idx1] == j;
    const unsigned long long votes = __ballot(mine);
    if (lane == 0) s_wave[wave] = __popcll(votes);
    __syncthreads();
    int pos = at + __popcll(votes & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) pos += s_wave[w];
    const int chunk = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    if (mine && pos < n1) {
      const size_t e = (size_t)j * (size_t)n1 + (size_t)idx1;
      orbm_new_point_t p;
      p.neighbour = j; p.idx1 = idx1; p.idx2 = P.in.matches12[e];
      p.x3D[0] = P.x3d[3 * e]; p.x3D[1] = P.x3d[3 * e + 1]; p.x3D[2] = P.x3d[3 * e + 2];
      P.list[pos] = p;
    }
    at += chunk;
    __syncthreads();
  }
  if (j == P.K - 1 && tid == 0) *P.total = at;
}
