// orb_fuse_sim3_kernels.h -- LoopClosing::SearchAndFuse (LoopClosing.cc:2631-2707): the search part of the Sim3 overload
// ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (ORBmatcher.cc:1664-1786) for ONE list of loop / merge map points against ALL
// corrected keyframes of a call (orbm_fuse_sim3_keyframes).
//
// The search is k_fuse_keyframes' (orb_fuse_kernels.h: claimless, one lane = one (target, point), the minimum of distance, then walk
// order, over the target's keypoints streamed through LDS in chunks of 256) without the chi-square gate, mvuRight and inv_sigma2: the
// staged keypoint is 12 bytes, not 20.  It is a kernel of its own, not an instantiation of one shared body, because of the shape.
// In loop closing most (target, point) pairs fail the depth or the image-bounds gate, and a workgroup with ONE live lane still streams
// the whole keyframe.  So there are two launches (where both forms are measured):
//   k_fuse_sim3_gate    grid (blocks of points, T): the gates of ORBmatcher.cc:1692-1735 through the shared expressions of
//                       orb_ref_geometry.h and orblg::ref_logf, and GetFeaturesInArea's cell window; a dead pair gets -1 / 256, a live
//                       one is appended to its target's list (one vector atomic per wavefront);
//   k_fuse_sim3_search  the same grid over the lists: block b of target t takes entries [256 b, 256 b + 256) and leaves at once where
//                       there are none.  Results scatter to (t, i), so the order of a list cannot change a row.
// What differs between targets is read from a per-target record in device memory (blockIdx.y selects it: scalar loads).
#pragma once
#include "orb_fuse_kernels.h"

// One corrected keyframe; the arrays lie in the call's staged block at byte offsets from its base (FuseTarget of orb_fuse_kernels.h
// without mvuRight, mvInvLevelSigma2 and bf).  Tcw / Ow are decompose_sim3's (orbhip.hip) of the target's Scw, computed once on the host.
struct FuseSim3Target {
  unsigned long long kp_off, desc_off;
  int n;
  float min_x, max_x, min_y, max_y, inv_w, inv_h;   // bounds, mfGridElementWidthInv / HeightInv (Frame.cc:379-380)
  float sf[16];
  int nlevels; float log_sf;
  float Tcw[16], Ow[3];
  int cam_type; float cam[8];
};
// A staged keypoint: position, octave | gx << 8 | gy << 16 | in-grid << 24 (FuseCand's first three fields)
struct FuseSim3Cand { float x, y; uint32_t bits; };

struct FuseLists { int32_t *list; int32_t *count; };   // [T][nP] point indices, [T] live pairs (zeroed by the upload)

// What the gates leave of a pair: query position, radius, predicted level, cell window
struct FuseGateOut { bool live; float u, v, rad; int lvl, cx0, cx1, cy0, cy1; };

__device__ __forceinline__ FuseGateOut fuse_sim3_gates(const FuseSim3Target &K, const FusePoints &P, size_t o, int i) {
  FuseGateOut g;
  g.live = false; g.u = 0.f; g.v = 0.f; g.rad = 0.f; g.lvl = 0;
  if (i < P.nP && P.valid[o]) {
    const float tcw[3] = {K.Tcw[3], K.Tcw[7], K.Tcw[11]};
    const float xw[3] = {P.Xw[3 * (size_t)i], P.Xw[3 * (size_t)i + 1], P.Xw[3 * (size_t)i + 2]};
    float pc[3];
    mat3_mul_add(K.Tcw, xw, tcw, pc);                                          // :1699
    if (!(pc[2] < 0.0f)) {                                                     // :1702
      float ux, vy;
      project(K.cam_type, K.cam, pc[0], pc[1], pc[2], ux, vy);                 // :1710
      if (is_in_image(ux, vy, K.min_x, K.max_x, K.min_y, K.max_y)) {           // :1713
        const float po[3] = {xw[0] - K.Ow[0], xw[1] - K.Ow[1], xw[2] - K.Ow[2]};
        const float dist = norm3(po);                                          // :1720
        if (!outside_scale_range(dist, P.min_dist, P.max_dist, (size_t)i)) {   // :1722
          const float pn[3] = {P.normal[3 * (size_t)i], P.normal[3 * (size_t)i + 1], P.normal[3 * (size_t)i + 2]};
          if (!(dot3_double(po, pn) < 0.5 * (double)dist)) {                   // :1728, Mat::dot in double
            g.lvl = level_from_log(orblg::ref_logf(P.max_dist[i] / dist), K.log_sf, K.nlevels);
            g.u = ux; g.v = vy;
            g.rad = P.th * K.sf[g.lvl];                                        // :1735
            g.live = true;
          }
        }
      }
    }
  }
  // KeyFrame::GetFeaturesInArea's cell window and early returns (load_query of orb_match_kernels.h)
  g.cx0 = max(0, (int)floorf((g.u - K.min_x - g.rad) * K.inv_w)); g.cx1 = min(63, (int)ceilf((g.u - K.min_x + g.rad) * K.inv_w));
  g.cy0 = max(0, (int)floorf((g.v - K.min_y - g.rad) * K.inv_h)); g.cy1 = min(47, (int)ceilf((g.v - K.min_y + g.rad) * K.inv_h));
  g.live = g.live && g.cx0 < 64 && g.cx1 >= 0 && g.cy0 < 48 && g.cy1 >= 0;
  return g;
}

__global__ __launch_bounds__(FUSE_NT) void k_fuse_sim3_gate(const FuseSim3Target *targets, FusePoints P, FuseLists Lst) {
  const int t = blockIdx.y, i = blockIdx.x * FUSE_NT + threadIdx.x;
  const FuseSim3Target &K = targets[t];
  const size_t o = (size_t)t * P.nP + i;
  const FuseGateOut g = fuse_sim3_gates(K, P, o, i);
  if (i < P.nP && !g.live) { P.best_idx[o] = -1; P.best_dist[o] = 256; }
  const unsigned long long mask = __builtin_amdgcn_ballot_w64(g.live);
  if (mask) {   // wavefront-aggregated append: one atomic per wavefront
    const int lane = threadIdx.x & 63, leader = __builtin_ctzll(mask);
    int base = 0;
    if (lane == leader) base = atomicAdd(&Lst.count[t], (int)__builtin_popcountll(mask));
    base = __shfl(base, leader, 64);
    if (g.live) Lst.list[(size_t)t * P.nP + base + (int)__builtin_popcountll(mask & ((1ull << lane) - 1ull))] = i;
  }
}

__global__ __launch_bounds__(FUSE_NT) void k_fuse_sim3_search(const uint8_t *block, const FuseSim3Target *targets, FusePoints P, FuseLists Lst) {
  __shared__ uint4 sDesc[FUSE_CH * 2];
  __shared__ FuseSim3Cand sCand[FUSE_CH];
  const int tid = threadIdx.x, t = blockIdx.y;
  const int cnt = Lst.count[t];
  if ((int)(blockIdx.x * FUSE_NT) >= cnt) return;   // uniform: nothing listed for this block
  const int j = blockIdx.x * FUSE_NT + tid;
  const int i = j < cnt ? Lst.list[(size_t)t * P.nP + j] : P.nP;
  const FuseSim3Target &K = targets[t];
  const size_t o = (size_t)t * P.nP + i;
  const FuseGateOut g = fuse_sim3_gates(K, P, o, i);   // the gates again (all pass): u, v, radius, level and window of the listed pair
  const bool live = g.live;
  const float u = g.u, v = g.v, rad = g.rad;
  const int lvl = g.lvl, cx0 = g.cx0, cx1 = g.cx1, cy0 = g.cy0, cy1 = g.cy1;
  uint32_t qd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (live) {
    const uint4 *qp = reinterpret_cast<const uint4 *>(P.mpdesc + 32 * (size_t)i);
    const uint4 a = qp[0], b = qp[1];
    qd[0] = a.x; qd[1] = a.y; qd[2] = a.z; qd[3] = a.w; qd[4] = b.x; qd[5] = b.y; qd[6] = b.z; qd[7] = b.w;
  }
  const int n = K.n;
  const float *kp = reinterpret_cast<const float *>(block + K.kp_off);
  const uint4 *desc = reinterpret_cast<const uint4 *>(block + K.desc_off);
  uint32_t best = 0xffffffffu;
  int bidx = -1;
  for (int base = 0; base < n; base += FUSE_CH) {
    const int m = min(FUSE_CH, n - base);
    __syncthreads();
    if (tid < 2 * m) sDesc[tid] = desc[(size_t)base * 2 + tid];
    if (tid + FUSE_NT < 2 * m) sDesc[tid + FUSE_NT] = desc[(size_t)base * 2 + tid + FUSE_NT];
    if (tid < m) {
      const size_t k = (size_t)(base + tid);
      FuseSim3Cand c;
      c.x = kp[k * 7]; c.y = kp[k * 7 + 1];
      const int oct = __float_as_int(kp[k * 7 + 5]);
      const int gx = (int)roundf((c.x - K.min_x) * K.inv_w), gy = (int)roundf((c.y - K.min_y) * K.inv_h);
      const bool in = gx >= 0 && gx < 64 && gy >= 0 && gy < 48;
      c.bits = (uint32_t)(oct & 0xff) | ((uint32_t)(gx & 0xff) << 8) | ((uint32_t)(gy & 0xff) << 16) | (in ? (1u << 24) : 0u);
      sCand[tid] = c;
    }
    __syncthreads();
    const int mu = __builtin_amdgcn_readfirstlane(m);
    for (int c = 0; c < mu; c++) {
      const FuseSim3Cand cm = sCand[c];
      const int oct = cm.bits & 0xff, gx = (cm.bits >> 8) & 0xff, gy = (cm.bits >> 16) & 0xff;
      // in grid, inside the cell window, level window [lvl - 1, lvl] (:1753), |dx| < r and |dy| < r (KeyFrame::GetFeaturesInArea)
      const bool ok = live && ((cm.bits >> 24) & 1u) && gx >= cx0 && gx <= cx1 && gy >= cy0 && gy <= cy1 && oct >= lvl - 1 && oct <= lvl &&
                      fabsf(cm.x - u) < rad && fabsf(cm.y - v) < rad;
      if (__builtin_amdgcn_ballot_w64(ok)) {
        const uint4 a = sDesc[2 * c], b = sDesc[2 * c + 1];
        int d0 = popc_acc(a.x ^ qd[0], 0), d1 = popc_acc(b.x ^ qd[4], 0);
        d0 = popc_acc(a.y ^ qd[1], d0); d1 = popc_acc(b.y ^ qd[5], d1);
        d0 = popc_acc(a.z ^ qd[2], d0); d1 = popc_acc(b.z ^ qd[6], d1);
        d0 = popc_acc(a.w ^ qd[3], d0); d1 = popc_acc(b.w ^ qd[7], d1);
        const uint32_t key = ((uint32_t)(d0 + d1) << 12) | cell_of(cm.bits);
        if (ok && key < best) { best = key; bidx = base + c; }
      }
    }
  }
  if (i < P.nP) {
    const int dist = (int)(best >> 12);
    const bool hit = bidx >= 0 && dist <= ORBM_TH_LOW;                         // :1768
    P.best_idx[o] = hit ? bidx : -1;
    P.best_dist[o] = hit ? dist : 256;
  }
}
