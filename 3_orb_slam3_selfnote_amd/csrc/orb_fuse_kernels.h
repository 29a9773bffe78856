// orb_fuse_kernels.h -- LocalMapping::SearchInNeighbors (LocalMapping.cc:909-1058): the search part of ORBmatcher::Fuse(pKF, vpMapPoints,
// th, bRight) (ORBmatcher.cc:1425-1620) for ONE list of map points against ALL target keyframes of a call (orbm_fuse_keyframes).
//
// Fuse is claimless: a keypoint that has received a map point stays a candidate (:1622-1640), so a point's answer depends on the
// keyframe alone - neither on the other points nor on the other targets - and none of the claim / top-k machinery of
// orb_match_kernels.h is needed.  One lane = one (target, point): the gates of fuse_core (orbhip.hip) through the shared expressions
// of orb_ref_geometry.h, then the minimum of the reduction key of orb_match_kernels.h - distance, then the walk order of
// GetFeaturesInArea (ix outer, iy inner, insertion order) - over the target's keypoints, streamed through LDS.
//
// Shape: 256 lanes per workgroup, chunks of 256 keypoints (one per lane to stage: 32 descriptor bytes and a 20-byte
// record, 13 KB of LDS per workgroup), grid (blocks of points, T).  What differs between targets - keypoint count, bounds, camera, pose,
// scale tables - is read from a per-target record in device memory (blockIdx.y selects it: scalar loads), not from the kernel arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "orb_common.h"
#include "orb_logf.h"
#include "orb_ref_geometry.h"
#include "orb_match_kernels.h"

#define FUSE_NT 256
#define FUSE_CH 256

// One target keyframe.  The arrays lie in the call's staged block at byte offsets from its base (the base moves when the block grows,
// the offsets do not); ur_off = FUSE_NO_UR: mvuRight absent, every keypoint monocular (-1).
#define FUSE_NO_UR (~(unsigned long long)0)
struct FuseTarget {
  unsigned long long kp_off, desc_off, ur_off;
  int n;
  float min_x, max_x, min_y, max_y, inv_w, inv_h;   // bounds, mfGridElementWidthInv / HeightInv (Frame.cc:379-380)
  float sf[16], inv_sigma2[16];
  int nlevels; float log_sf;
  float Tcw[16], Ow[3];
  int cam_type; float cam[8];
  float bf;
};

struct FusePoints {
  int nP;
  const uint8_t *valid;          // [T][nP]
  const float *Xw, *normal;      // [nP][3]
  const uint8_t *mpdesc;         // [nP][32], 16-byte aligned
  const float *max_dist, *min_dist;
  float th;
  int32_t *best_idx, *best_dist; // [T][nP]
};

// A staged keypoint: position, octave | gx << 8 | gy << 16 | in-grid << 24 (CandMeta's layout; Fuse has no occupants, so usable =
// in grid), mvuRight, mvInvLevelSigma2[octave]
struct FuseCand { float x, y; uint32_t bits; float ur, is2; };

__global__ __launch_bounds__(FUSE_NT) void k_fuse_keyframes(const uint8_t *block, const FuseTarget *targets, FusePoints P) {
  __shared__ uint4 sDesc[FUSE_CH * 2];
  __shared__ FuseCand sCand[FUSE_CH];
  const int tid = threadIdx.x, t = blockIdx.y;
  const int i = blockIdx.x * FUSE_NT + tid;
  const FuseTarget &K = targets[t];
  const size_t o = (size_t)t * P.nP + i;
  // (a) the gates of fuse_core, ORBmatcher.cc:1455-1524
  bool live = false;
  float u = 0.f, v = 0.f, ur = 0.f, rad = 0.f;
  int lvl = 0;
  if (i < P.nP && P.valid[o]) {
    const float tcw[3] = {K.Tcw[3], K.Tcw[7], K.Tcw[11]};
    const float xw[3] = {P.Xw[3 * (size_t)i], P.Xw[3 * (size_t)i + 1], P.Xw[3 * (size_t)i + 2]};
    float pc[3];
    mat3_mul_add(K.Tcw, xw, tcw, pc);                                          // :1472
    if (!(pc[2] < 0.0f)) {                                                     // :1475
      const float invz = 1 / pc[2];                                            // :1481
      float ux, vy;
      project(K.cam_type, K.cam, pc[0], pc[1], pc[2], ux, vy);                 // :1487
      if (is_in_image(ux, vy, K.min_x, K.max_x, K.min_y, K.max_y)) {           // :1490
        const float po[3] = {xw[0] - K.Ow[0], xw[1] - K.Ow[1], xw[2] - K.Ow[2]};
        const float dist = norm3(po);                                          // :1502
        if (!outside_scale_range(dist, P.min_dist, P.max_dist, (size_t)i)) {   // :1505
          const float pn[3] = {P.normal[3 * (size_t)i], P.normal[3 * (size_t)i + 1], P.normal[3 * (size_t)i + 2]};
          if (!(dot3_double(po, pn) < 0.5 * (double)dist)) {                   // :1514, Mat::dot in double
            lvl = level_from_log(orblg::ref_logf(P.max_dist[i] / dist), K.log_sf, K.nlevels);   // MapPoint::PredictScale
            u = ux; v = vy; ur = ux - K.bf * invz;                             // :1495
            rad = P.th * K.sf[lvl];                                            // :1524
            live = true;
          }
        }
      }
    }
  }
  // KeyFrame::GetFeaturesInArea's cell window and early returns (load_query of orb_match_kernels.h)
  const int cx0 = max(0, (int)floorf((u - K.min_x - rad) * K.inv_w)), cx1 = min(63, (int)ceilf((u - K.min_x + rad) * K.inv_w));
  const int cy0 = max(0, (int)floorf((v - K.min_y - rad) * K.inv_h)), cy1 = min(47, (int)ceilf((v - K.min_y + rad) * K.inv_h));
  live = live && cx0 < 64 && cx1 >= 0 && cy0 < 48 && cy1 >= 0;
  // (b) nothing to search: leave before the keyframe is touched
  if (!__syncthreads_or(live)) {
    if (i < P.nP) { P.best_idx[o] = -1; P.best_dist[o] = 256; }
    return;
  }
  uint32_t qd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (live) {
    const uint4 *qp = reinterpret_cast<const uint4 *>(P.mpdesc + 32 * (size_t)i);
    const uint4 a = qp[0], b = qp[1];
    qd[0] = a.x; qd[1] = a.y; qd[2] = a.z; qd[3] = a.w; qd[4] = b.x; qd[5] = b.y; qd[6] = b.z; qd[7] = b.w;
  }
  const int n = K.n;
  const float *kp = reinterpret_cast<const float *>(block + K.kp_off);
  const uint4 *desc = reinterpret_cast<const uint4 *>(block + K.desc_off);
  const float *uright = K.ur_off == FUSE_NO_UR ? nullptr : reinterpret_cast<const float *>(block + K.ur_off);
  // (d) the key: dist << 12 | ix * 48 + iy; candidates arrive in index order and the comparison is strict, so among equal keys the
  // lowest index stays - the first minimum of the walk order, which the reference's strict `<` keeps (:1611)
  uint32_t best = 0xffffffffu;
  int bidx = -1;
  for (int base = 0; base < n; base += FUSE_CH) {
    const int m = min(FUSE_CH, n - base);
    __syncthreads();
    // (c) the chunk: descriptor rows (two coalesced passes), one record per keypoint
    if (tid < 2 * m) sDesc[tid] = desc[(size_t)base * 2 + tid];
    if (tid + FUSE_NT < 2 * m) sDesc[tid + FUSE_NT] = desc[(size_t)base * 2 + tid + FUSE_NT];
    if (tid < m) {
      const size_t k = (size_t)(base + tid);
      FuseCand c;
      c.x = kp[k * 7]; c.y = kp[k * 7 + 1];
      const int oct = __float_as_int(kp[k * 7 + 5]);
      c.ur = uright ? uright[k] : -1.f;
      c.is2 = K.inv_sigma2[oct & 15];
      // Frame::PosInGrid, Frame.cc:815-825 (cand_bits of orb_match_kernels.h without an occupant)
      const int gx = (int)roundf((c.x - K.min_x) * K.inv_w), gy = (int)roundf((c.y - K.min_y) * K.inv_h);
      const bool in = gx >= 0 && gx < 64 && gy >= 0 && gy < 48;
      c.bits = (uint32_t)(oct & 0xff) | ((uint32_t)(gx & 0xff) << 8) | ((uint32_t)(gy & 0xff) << 16) | (in ? (1u << 24) : 0u);
      sCand[tid] = c;
    }
    __syncthreads();
    const int mu = __builtin_amdgcn_readfirstlane(m);
    for (int c = 0; c < mu; c++) {
      const FuseCand cm = sCand[c];   // uniform index: a broadcast read
      const int oct = cm.bits & 0xff, gx = (cm.bits >> 8) & 0xff, gy = (cm.bits >> 16) & 0xff;
      // cand_passes(): in grid, inside the cell window, level window [lvl - 1, lvl] (:1555), |dx| < r and |dy| < r (Frame.cc:803-806)
      bool ok = live && ((cm.bits >> 24) & 1u) && gx >= cx0 && gx <= cx1 && gy >= cy0 && gy <= cy1 && oct >= lvl - 1 && oct <= lvl &&
                fabsf(cm.x - u) < rad && fabsf(cm.y - v) < rad;
      {                                                                        // the chi-square gate of SCAN_FUSE, :1585-1608
        const float ex = u - cm.x, ey = v - cm.y;
        float e2 = ex * ex + ey * ey;
        double lim = 5.99;
        if (cm.ur >= 0.f) { const float er = ur - cm.ur; e2 = e2 + er * er; lim = 7.8; }
        ok = ok && !((double)(e2 * cm.is2) > lim);
      }
      if (__builtin_amdgcn_ballot_w64(ok)) {                                   // no lane passes: no distance
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
    const bool hit = bidx >= 0 && dist <= ORBM_TH_LOW;                         // :1622
    P.best_idx[o] = hit ? bidx : -1;
    P.best_dist[o] = hit ? dist : 256;
  }
}
