// orb_twoview_kernels.h -- TwoViewReconstruction::Reconstruct on the device (include/orbhip.h, TWO-VIEW RULE): the 2 x iterations
// hypotheses of FindHomography / FindFundamental, their scores against every match, the winner per model with its inlier mask, and
// CheckRT for every motion hypothesis.  The arithmetic is orb_ref_twoview.h, the host's own definition.
#pragma once
#include "orb_ref_twoview.h"

struct TvModelParams {
  float T1[9], T2inv[9], T2t[9];   // Normalize's T1, T2.inv(), T2.t()
  const float *pn1, *pn2;          // the normalised keypoints of both frames [n][2]
  const int32_t *first, *second;   // mvMatches12 [N]
  const int32_t *sets;             // mvSets [iterations][8]
  const float4 *mx;                // per match: kp1.pt, kp2.pt
  int iterations, N;
  float invSigmaSquare;
  float *H21, *H12, *F21;          // [iterations][9]
  float *score;                    // [2][iterations]: CheckHomography, CheckFundamental
  int32_t *best;                   // [2] the winning iteration or -1
  float *best_score;               // [2] SH, SF
  float *best_M;                   // [2][9] H21, F21 of the winners (zeros without one)
  uint8_t *mask;                   // [2][N] vbMatchesInliersH, vbMatchesInliersF
};

// The hypothesis of one (model, iteration): the set's eight normalised pairs gathered, then ComputeH21 / ComputeF21 with their SVDs, the
// denormalisation and, for H, the inverse.  Sixteen lanes per hypothesis, four hypotheses per wavefront, the matrices in LDS.  A lane
// takes element k = lane of a rotation's row updates (16 x 9: all sixteen; 8 x 9: nine; V: nine or eight); the ordered sums are formed by
// every lane from LDS, the same address in all sixteen lanes, and everything else is run by all sixteen alike, storing equal values.  The
// lanes of a group take every branch together (they hold the same p, a, b), groups diverge from each other.  Every loop of the Jacobi
// is bounded (max(m, 30) sweeps, 100 completion attempts): a lane cannot spin.  (One lane per hypothesis with the matrices of 64 lanes in
// LDS was measured at twice the time and is not kept: DESIGN.md section 5.)
#define TV_WS_STRIDE (TV_WS_FLOATS + 1)
struct TvLanes16 {
  int lane;
  __device__ __forceinline__ int first() const { return lane; }
  __device__ __forceinline__ int step() const { return 16; }
  __device__ __forceinline__ void sync() const {   // the group's LDS stores in front of its loads: one wavefront, its LDS accesses stay in order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
};
__global__ __launch_bounds__(64) void k_tv_hypotheses(TvModelParams P) {
  __shared__ float s_ws[4 * TV_WS_STRIDE];
  __shared__ double s_W[4 * TV_WS_DOUBLES];
  const int group = threadIdx.x >> 4;
  const TvLanes16 lanes{(int)threadIdx.x & 15};
  const int item = blockIdx.x * 4 + group;
  if (item >= 2 * P.iterations) return;
  const int model = item >= P.iterations, it = item - model * P.iterations;
  float *ws = s_ws + group * TV_WS_STRIDE;
  double *W = s_W + group * TV_WS_DOUBLES;
  float q[32];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int idx = P.sets[8 * it + j];
    const int i1 = P.first[idx], i2 = P.second[idx];
    q[4 * j] = P.pn1[2 * i1]; q[4 * j + 1] = P.pn1[2 * i1 + 1]; q[4 * j + 2] = P.pn2[2 * i2]; q[4 * j + 3] = P.pn2[2 * i2 + 1];
  }
  float M21[9], M12[9];
  if (model == 0) {
    tv_homography(q, P.T1, P.T2inv, ws, W, M21, M12, lanes);
    if (lanes.lane == 0)
#pragma unroll
      for (int k = 0; k < 9; k++) { P.H21[9 * it + k] = M21[k]; P.H12[9 * it + k] = M12[k]; }
  } else {
    tv_fundamental(q, P.T1, P.T2t, ws, W, M21, lanes);
    if (lanes.lane == 0)
#pragma unroll
      for (int k = 0; k < 9; k++) P.F21[9 * it + k] = M21[k];
  }
}

// One wavefront per (iteration, model).  A step evaluates 64 matches, one per lane; the score is then added in the reference's order
// - match ascending, the first image's term before the second's, into one float - by every lane alike from the lanes' terms.
__global__ __launch_bounds__(64) void k_tv_score(TvModelParams P) {
  const int it = blockIdx.x, model = blockIdx.y, lane = threadIdx.x;
  float M21[9], M12[9];
#pragma unroll
  for (int k = 0; k < 9; k++) { M21[k] = (model ? P.F21 : P.H21)[9 * it + k]; M12[k] = P.H12[9 * it + k]; }
  float score = 0;
  for (int base = 0; base < P.N; base += 64) {
    const int i = base + lane;
    TvTerms r;
    r.t1 = r.t2 = 0.f; r.in1 = r.in2 = false;
    if (i < P.N) {
      const float4 m = P.mx[i];
      r = tv_check_model(model, M21, M12, m.x, m.y, m.z, m.w, P.invSigmaSquare);
    }
    // A term that is not added becomes +0: score is never -0 (it starts at +0 and every added term is th - chiSquare >= +0 or NaN), so
    // score + 0 is score, bit for bit, and the loop needs no branch.
    const float t1 = r.in1 ? r.t1 : 0.f, t2 = r.in2 ? r.t2 : 0.f;
    const int cnt = P.N - base < 64 ? P.N - base : 64;
    for (int l = 0; l < cnt; l++) {   // l is the wavefront's own: the terms of lane l come over the scalar unit
      score += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t1), l));
      score += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t2), l));
    }
  }
  if (lane == 0) P.score[model * P.iterations + it] = score;
}

// One block per model: the FIRST iteration with the strictly greatest score above 0 (`currentScore > score` from score = 0, in order: a
// NaN never wins), then that iteration's inlier mask and matrix.  Without a winner the mask and the matrix are zeros.
__global__ __launch_bounds__(256) void k_tv_winner(TvModelParams P) {
  const int model = blockIdx.x, tid = threadIdx.x;
  __shared__ float s_score[256];
  __shared__ float s_top;
  __shared__ int s_best;
  if (tid == 0) { s_top = 0.f; s_best = -1; }
  for (int c = 0; c < P.iterations; c += 256) {
    if (c + tid < P.iterations) s_score[tid] = P.score[model * P.iterations + c + tid];
    __syncthreads();
    if (tid == 0) {
      const int cnt = P.iterations - c < 256 ? P.iterations - c : 256;
      float top = s_top;
      int best = s_best;
      for (int k = 0; k < cnt; k++)
        if (s_score[k] > top) { top = s_score[k]; best = c + k; }
      s_top = top; s_best = best;
    }
    __syncthreads();
  }
  const int best = s_best;
  if (tid == 0) { P.best[model] = best; P.best_score[model] = s_top; }
  float M21[9], M12[9];
#pragma unroll
  for (int k = 0; k < 9; k++) {
    M21[k] = best < 0 ? 0.f : (model ? P.F21 : P.H21)[9 * best + k];
    M12[k] = best < 0 ? 0.f : P.H12[9 * best + k];
  }
  if (tid < 9) P.best_M[9 * model + tid] = best < 0 ? 0.f : (model ? P.F21 : P.H21)[9 * best + tid];
  for (int i = tid; i < P.N; i += 256) {
    bool in = false;
    if (best >= 0) {
      const float4 m = P.mx[i];
      const TvTerms r = tv_check_model(model, M21, M12, m.x, m.y, m.z, m.w, P.invSigmaSquare);
      in = r.in1 && r.in2;
    }
    P.mask[(size_t)model * P.N + i] = in;
  }
}

// CheckRT: one lane per (match, hypothesis).  vP3D and vbGood are indexed by the first keypoint and arrive zeroed; a first keypoint
// belongs to one match, so no two lanes write one entry.  The accepted cosParallax values go to a list in arrival order: the reference
// sorts it, and equal values are interchangeable.
struct TvCheckParams {
  const TvCamera *cams;   // [nhyp]
  const float4 *mx;
  const int32_t *first;
  const uint8_t *mask;    // [N]
  int nhyp, N, n1;
  float *p3d;             // [nhyp][n1][3]
  uint8_t *good;          // [nhyp][n1]
  uint8_t *status;        // [nhyp][N]
  int32_t *nGood;         // [nhyp], zeroed
  float *cos_list;        // [nhyp][N]
  float *cos_rank;        // [nhyp] the value at rank min(50, nGood - 1) of the ascending list; 0 for an empty one
};
__global__ __launch_bounds__(256) void k_tv_check_rt(TvCheckParams P) {
  const int i = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y;
  if (i >= P.N) return;
  const size_t e = (size_t)h * P.N + i;
  if (!P.mask[i]) { P.status[e] = TV_NOT_INLIER; return; }
  const float4 m = P.mx[i];
  float p[3], cp = 0.f;
  const int st = tv_check_rt(P.cams[h], m.x, m.y, m.z, m.w, p, &cp);
  P.status[e] = (uint8_t)st;
  if (st != TV_GOOD && st != TV_LOW_PARALLAX) return;
  const size_t k = (size_t)h * P.n1 + P.first[i];
  P.p3d[3 * k] = p[0]; P.p3d[3 * k + 1] = p[1]; P.p3d[3 * k + 2] = p[2];
  if (st == TV_GOOD) P.good[k] = 1;
  const int slot = atomicAdd(&P.nGood[h], 1);
  P.cos_list[(size_t)h * P.N + slot] = cp;
}

// vCosParallax[min(50, size - 1)] of the sorted list by a rank count, as k_stereo_median selects its median: x is the answer when
// #{y < x} <= rank < #{y <= x}.  One lane per accepted value, blockIdx.y the hypothesis; the list passes through LDS 1024 values at a time,
// every lane reading the same word.  Lanes that hold equal answers store the same bits.
__global__ __launch_bounds__(256) void k_tv_cos_rank(TvCheckParams P) {
  const int h = blockIdx.y, tid = threadIdx.x, a = blockIdx.x * 256 + tid;
  const int n = P.nGood[h];
  if (n == 0) { if (a == 0) P.cos_rank[h] = 0.f; return; }
  if ((int)blockIdx.x * 256 >= n) return;   // the whole block: n and blockIdx are its own
  __shared__ float s_list[1024];
  const float *list = P.cos_list + (size_t)h * P.N;
  const int rank = n - 1 < 50 ? n - 1 : 50;
  const float x = a < n ? list[a] : 0.f;
  int less = 0, leq = 0;
  for (int c = 0; c < n; c += 1024) {
    const int cnt = n - c < 1024 ? n - c : 1024;
    for (int k = tid; k < cnt; k += 256) s_list[k] = list[c + k];
    __syncthreads();
    for (int b = 0; b < cnt; b++) { const float y = s_list[b]; less += y < x; leq += y <= x; }
    __syncthreads();
  }
  if (a < n && less <= rank && rank < leq) P.cos_rank[h] = x;
}
