// orb_sim3_kernels.h -- Sim3Solver on the device (include/orbhip.h, SIM3 RULE): the quaternion of every iteration's Horn hypothesis, the
// inlier count and mask of every (iteration, pair), and the ordered pass that finds the stop iteration and the best.  The arithmetic is
// orb_ref_sim3.h, the host's own definition; the double-libm tail between the first two kernels runs on the host (sim3_tail).
#pragma once
#include "orb_ref_sim3.h"

#define SIM3_SET_FLOATS 28   // per iteration: Sim3Set (Pr1, Pr2, O1, O2) and the quaternion row
static_assert(sizeof(Sim3Set) == 24 * sizeof(float), "Sim3Set is 24 floats");

struct Sim3Params {
  const float *X1, *X2;        // mvX3Dc1, mvX3Dc2 [N][3]
  const float *im1, *im2;      // mvP1im1, mvP2im2 [N][2]
  const float *th1, *th2;      // mvnMaxError1/2 as the float they are compared as [N]
  const int32_t *idx1;         // mvnIndices1 [N]
  const int32_t *sets;         // [iterations][3]
  int iterations, N, n1, words;   // words = ceil(N / 64)
  int cam1, cam2;
  float p1[8], p2[8];
  float *set_out;              // [iterations][SIM3_SET_FLOATS]
  const float *T;              // [iterations][32]: T12, T21 row-major 4 x 4
  int32_t *counts;             // [iterations]
  uint64_t *mask_words;        // [iterations][words]
  int best_in, min_inliers, done, max_its;
  int32_t *pass;               // [6] Sim3Pass
  uint8_t *best_mask;          // [N]
  uint8_t *vb;                 // [n1]
};

// One lane per iteration: the set's three pairs gathered as columns, both centroids, M, N and the float Jacobi.  Every loop of the Jacobi
// is bounded (480 rotations): a lane cannot spin.  The Jacobi's matrices live in the lane's own slice of LDS, at an odd stride so that
// the 64 lanes' equal offsets fall into different banks; no other lane reads a slice, so no barrier is needed.  (With the matrices in
// registers every access at the pivot's indices became a chain of selects: 97.7 us per launch of 300 against the figure in DESIGN.md
// section 5.)
#define SIM3_WS_STRIDE (SIM3_WS_FLOATS + 1)
#define SIM3_IW_STRIDE (SIM3_WS_INTS + 1)
__global__ __launch_bounds__(64) void k_sim3_hypotheses(Sim3Params P) {
  __shared__ float s_ws[64 * SIM3_WS_STRIDE];
  __shared__ int s_iw[64 * SIM3_IW_STRIDE];
  const int it = blockIdx.x * 64 + threadIdx.x;
  if (it >= P.iterations) return;
  float P1[9], P2[9];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const int idx = P.sets[3 * it + c];
#pragma unroll
    for (int r = 0; r < 3; r++) { P1[3 * r + c] = P.X1[3 * idx + r]; P2[3 * r + c] = P.X2[3 * idx + r]; }   // copyTo(P3Dc1i.col(i)) :208-209
  }
  Sim3Set S;
  float q[4];
  sim3_quaternion(P1, P2, S, q, s_ws + threadIdx.x * SIM3_WS_STRIDE, s_iw + threadIdx.x * SIM3_IW_STRIDE);
  float *o = P.set_out + (size_t)SIM3_SET_FLOATS * it;
#pragma unroll
  for (int k = 0; k < 9; k++) { o[k] = S.Pr1[k]; o[9 + k] = S.Pr2[k]; }
#pragma unroll
  for (int k = 0; k < 3; k++) { o[18 + k] = S.O1[k]; o[21 + k] = S.O2[k]; }
#pragma unroll
  for (int k = 0; k < 4; k++) o[24 + k] = q[k];
}

// One wavefront per iteration.  It walks the pairs in strides of 64, one pair per lane, both projections through the camera models' own
// project; one ballot per stride is the stride's 64-bit mask word, and its population count is added to the iteration's count.
__global__ __launch_bounds__(64) void k_sim3_check(Sim3Params P) {
  const int it = blockIdx.x, lane = threadIdx.x;
  float T12[12], T21[12];
#pragma unroll
  for (int k = 0; k < 12; k++) { T12[k] = P.T[32 * (size_t)it + k]; T21[k] = P.T[32 * (size_t)it + 16 + k]; }
  int count = 0;
  for (int base = 0, w = 0; base < P.N; base += 64, w++) {
    const int i = base + lane;
    bool in = false;
    if (i < P.N)
      in = sim3_inlier(T12, T21, P.cam1, P.p1, P.cam2, P.p2, P.X1 + 3 * i, P.X2 + 3 * i, P.im1 + 2 * i, P.im2 + 2 * i, P.th1[i], P.th2[i]);
    const uint64_t word = __ballot(in);
    count += __popcll(word);
    if (lane == 0) P.mask_words[(size_t)it * P.words + w] = word;
  }
  if (lane == 0) P.counts[it] = count;
}

// One workgroup: the ordered pass of the SIM3 RULE, then the best iteration's mask as bytes and, on convergence, spread through idx1 into
// vbInliers (zeros otherwise).  The pass is the first wavefront's: 64 counts at a time, one per lane, read back in order over the scalar
// unit (v_readlane), every lane walking the same scalars.  (One lane reading the counts one by one, from memory or from LDS, took 36
// and 24 us for 300 iterations.)  idx1 is ascending, so no two pairs share an entry.
__global__ __launch_bounds__(256) void k_sim3_winner(Sim3Params P) {
  const int tid = threadIdx.x;
  __shared__ Sim3Pass s_pass;
  for (int i = tid; i < P.n1; i += 256) P.vb[i] = 0;
  if (tid < 64) {
    const int limit = sim3_pass_limit(P.iterations, P.done, P.max_its);
    Sim3Pass R = sim3_pass_begin(P.best_in);
    bool go = true;
    for (int c = 0; c < limit && go; c += 64) {
      const int mine = c + tid < limit ? P.counts[c + tid] : 0;
      const int cnt = limit - c < 64 ? limit - c : 64;
      for (int l = 0; l < cnt && go; l++) go = sim3_pass_take(R, __builtin_amdgcn_readlane(mine, l), P.min_inliers);
    }
    sim3_pass_end(R, P.done, P.max_its);
    if (tid == 0) {
      s_pass = R;
      P.pass[0] = R.converged; P.pass[1] = R.it_stop; P.pass[2] = R.best_it;
      P.pass[3] = R.best_inliers; P.pass[4] = R.improved; P.pass[5] = R.no_more;
    }
  }
  __syncthreads();
  const int best = s_pass.best_it;
  const bool spread = s_pass.converged != 0;
  for (int i = tid; i < P.N; i += 256) {
    const bool in = best >= 0 && ((P.mask_words[(size_t)best * P.words + (i >> 6)] >> (i & 63)) & 1);
    P.best_mask[i] = in;
    if (spread && in) P.vb[P.idx1[i]] = 1;
  }
}
