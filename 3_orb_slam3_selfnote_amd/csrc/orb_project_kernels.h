// orb_project_kernels.h -- the parts of SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono)
// (ORBmatcher.cc:2027-2289, Nleft == -1 and Nleft != -1) that surround the Hamming search: the projection of the last frame's map points into
// the current frame (:2038-2118) in front of k_match_scan / k_match_resolve, and the rotation-histogram pruning (:2177-2185,
// :2263-2286) behind them.  With both on the device a whole batch of frame pairs runs without touching the host
// (BASELINE config 5: KannalaBrandt8 projection inside the search).
//
// Every operation is the IEEE-754 single / double operation of the reference's expression in source order (no contraction),
// and the libm calls of KannalaBrandt8::project go through the bit-exact replicas of glibc's atan2f (orb_atan2f.h) and
// sinf / cosf (orb_sincos.h), so u, v - and with them the search windows - carry the same bits as on the host.  The expressions
// themselves are the host loops' own functions (orb_ref_geometry.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "orb_common.h"
#include "orb_logf.h"
#include "orb_ref_geometry.h"

// The current frame of a projection search: image bounds, scale factors, camera (host: fill_view)
struct ViewParams {
  float min_x, max_x, min_y, max_y;
  float sf[16]; int nlevels;
  int cam_type; float cam[8];
};

// The query arrays a projection kernel writes for the search behind it (same stride as its input side; host: carve_query_scratch).
// moq: where the search may put match_of_query when the caller has no array for it.
struct QueryScratch { float *u, *v, *r, *ur; int32_t *minl, *maxl, *moq; uint8_t *flags; };

__device__ __forceinline__ void store_query(const QueryScratch &Q, size_t o, float u, float v, float rad, float ur, int minl, int maxl, uint8_t fl) {
  Q.u[o] = u; Q.v[o] = v; Q.r[o] = rad; Q.ur[o] = ur;
  Q.minl[o] = minl; Q.maxl[o] = maxl; Q.flags[o] = fl;
}

struct LastFrameParams {
  // last-frame side; problem p is at element offset p * last_stride
  const uint8_t *has_mp;   // LastFrame.mvpMapPoints[i] && !LastFrame.mvbOutlier[i]
  const float *Xw;         // pMP->GetWorldPos(), 3 floats per keypoint
  const float *last_kp;    // LastFrame.mvKeys as 7 floats per keypoint (octave = word 5, angle = word 3)
  const uint8_t *obs;      // pMP->Observations() > 0, or NULL = all 1
  const float *Tcw, *Tlw;  // row-major 4x4 per problem (16 floats)
  int last_stride; LiveCount last_n;   // live count of problem p: last_n.at(p, last_stride)
  ViewParams V;
  float mb, mbf, th; int bMono;
  QueryScratch Q;          // out
};

// ORBmatcher.cc:2038-2052 (per pair, recomputed by every thread from scalar loads) and :2062-2118 for last-frame keypoint i of
// problem p (o = p * last_stride + i, n = the problem's live count): (u, v, radius, level window, right coordinate, flags) of
// its query in the (left) image; fl = 0: the point takes no part.  xc = x3Dc (:2072), valid where fl != 0.
struct LastFrameQuery { float u, v, rad, ur; int minl, maxl; uint8_t fl; };

__device__ __forceinline__ LastFrameQuery lastframe_query(const LastFrameParams &P, int p, int i, int n, size_t o, float *xc) {
  LastFrameQuery q = {0.f, 0.f, 0.f, 0.f, -1, -1, 0};
  if (i < n && P.has_mp[o]) {
    const float *Tcw = P.Tcw + (size_t)p * 16, *Tlw = P.Tlw + (size_t)p * 16;
    const float tcw[3] = {Tcw[3], Tcw[7], Tcw[11]}, tlw[3] = {Tlw[3], Tlw[7], Tlw[11]};
    float twc[3], tlc[3];
    camera_centre(Tcw, twc);           // :2041
    mat3_mul_add(Tlw, twc, tlw, tlc);  // :2047
    const bool bForward = tlc[2] > P.mb && !P.bMono, bBackward = -tlc[2] > P.mb && !P.bMono;  // :2051-2052
    const float xw[3] = {P.Xw[3 * o], P.Xw[3 * o + 1], P.Xw[3 * o + 2]};
    mat3_mul_add(Tcw, xw, tcw, xc);                          // :2072
    const float invzc = (float)(1.0 / (double)xc[2]);        // :2076
    if (!(invzc < 0)) {
      float ux, vy;
      project(P.V.cam_type, P.V.cam, xc[0], xc[1], xc[2], ux, vy);  // :2091
      const bool inside = inside_bounds(ux, vy, P.V.min_x, P.V.max_x, P.V.min_y, P.V.max_y);  // :2094-2097
      const int oct = __float_as_int(P.last_kp[7 * o + 5]);
      if (inside && oct >= 0 && oct < P.V.nlevels) {
        q.u = ux; q.v = vy;
        q.rad = P.th * P.V.sf[oct];                                 // :2105
        lastframe_level_window(bForward, bBackward, oct, q.minl, q.maxl);   // :2113-2118
        q.ur = ux - P.mbf * invzc;                                  // :2141
        q.fl = query_flags(P.obs, o);
      }
    }
  }
  return q;
}

// One thread per last-frame keypoint -> query i.
__global__ __launch_bounds__(256) void k_lastframe_project(LastFrameParams P) {
  const int p = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int n = P.last_n.at(p, P.last_stride);
  if (i >= P.last_stride) return;
  const size_t o = (size_t)p * P.last_stride + i;
  float xc[3];
  const LastFrameQuery q = lastframe_query(P, p, i, n, o, xc);
  store_query(P.Q, o, q.u, q.v, q.rad, q.ur, q.minl, q.maxl, q.fl);
}

// The same loop for a fisheye-stereo current frame (CurrentFrame.Nleft != -1, :2027-2289 with the right-camera pass :2189-2256):
// last-frame keypoint i makes the queries 2i (left image, the arithmetic above) and 2i + 1 (right image: x3Dr = Rrl * x3Dc + trl
// through the frame's own camera, :2190-2192; radius and level window of the left query, :2197-2207; no bounds or depth test,
// the reference has none).  A point the left half drops makes neither.  The search reads 32 descriptor bytes per QUERY, so the
// point's descriptor is written twice here (qdesc) next to the side bytes; query_n[p] = 2 * the live count.
struct RigProjectParams {
  float Trl[12];           // CurrentFrame.mTrl, row-major 3x4
  const uint8_t *mpdesc;   // 32 bytes per last-frame keypoint (16-byte aligned)
  uint8_t *qdesc, *qside;  // out: 32 bytes and one byte per query, problem p at query offset p * 2 * last_stride
  int32_t *query_n;        // out: [npairs]
};

__global__ __launch_bounds__(256) void k_lastframe_project_rig(LastFrameParams P, RigProjectParams G) {
  const int p = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int n = P.last_n.at(p, P.last_stride);
  if (i == 0) G.query_n[p] = 2 * n;
  if (i >= P.last_stride) return;
  const size_t o = (size_t)p * P.last_stride + i;
  float xc[3];
  const LastFrameQuery q = lastframe_query(P, p, i, n, o, xc);
  float ur = 0.f, vr = 0.f;
  if (q.fl) {
    const float trl[3] = {G.Trl[3], G.Trl[7], G.Trl[11]};
    float xr[3];
    mat3_mul_add(G.Trl, xc, trl, xr);                                  // :2190
    project(P.V.cam_type, P.V.cam, xr[0], xr[1], xr[2], ur, vr);       // :2192 (mpCamera, not mpCamera2)
  }
  store_query(P.Q, 2 * o, q.u, q.v, q.rad, 0.f, q.minl, q.maxl, q.fl);     // Nleft != -1: no mvuRight test (:2139)
  store_query(P.Q, 2 * o + 1, ur, vr, q.rad, 0.f, q.minl, q.maxl, q.fl);
  G.qside[2 * o] = 0; G.qside[2 * o + 1] = 1;
  if (i < n) {
    const uint4 *src = reinterpret_cast<const uint4 *>(G.mpdesc + 32 * o);
    uint4 *dst = reinterpret_cast<uint4 *>(G.qdesc + 64 * o);
    const uint4 a = src[0], b = src[1];
    dst[0] = a; dst[1] = b; dst[2] = a; dst[3] = b;
  }
}

// ------------------------------------------------------------------------------------------------------------
// Tracking::SearchLocalPoints (Tracking.cc:3449-3539): Frame::isInFrustum(pMP, viewingCosLimit) for every local map point
// (Frame.cc:572-661, Nleft == -1) with MapPoint::PredictScale (MapPoint.cc:587-602) through the glibc logf replica
// (orb_logf.h), then the query preparation of SearchByProjection(Frame&, const vector<MapPoint*>&, th, bFarPoints,
// thFarPoints) (ORBmatcher.cc:44-73) in front of k_match_walk / k_match_scan / k_match_resolve.  One thread per local map
// point; the frame's pose is read per problem.
// ------------------------------------------------------------------------------------------------------------
struct LocalMapParams {
  // local map side; problem p is at element offset p * map_stride
  const uint8_t *eligible;          // !pMP->isBad() && pMP->mnLastFrameSeen != CurrentFrame.mnId
  const float *Xw, *normal;         // GetWorldPos(), GetNormal(): 3 floats per point
  const float *max_dist, *min_dist; // raw mfMaxDistance / mfMinDistance
  const uint8_t *obs;               // Observations() > 0, or NULL = all 1
  const float *Tcw;                 // CurrentFrame.mTcw, row-major 4x4 per problem
  int map_stride; LiveCount map_n;     // live count of problem p: map_n.at(p, map_stride)
  ViewParams V; float log_sf;
  float mbf, view_cos_limit, th; int bFarPoints; float th_far;
  // out: the MapPoint fields isInFrustum writes (caller arrays, same stride)
  uint8_t *in_view; float *proj_x, *proj_y, *proj_xr, *depth, *view_cos; int32_t *level;
  QueryScratch Q;                   // out: the queries of the projection search
};

__global__ __launch_bounds__(256) void k_local_map_project(LocalMapParams P) {
  const int p = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int n = P.map_n.at(p, P.map_stride);
  if (i >= P.map_stride) return;
  const size_t o = (size_t)p * P.map_stride + i;
  float u = 0.f, v = 0.f, rad = 0.f, ur = 0.f;
  int minl = -1, maxl = -1;
  uint8_t fl = 0;
  if (i < n) {
    if (!P.eligible[o]) {
      P.in_view[o] = 0;
    } else {
      const float *T = P.Tcw + (size_t)p * 16;
      const float tcw[3] = {T[3], T[7], T[11]};
      float Ow[3];
      camera_centre(T, Ow);                                       // mOw, Frame.cc:538
      const float xw[3] = {P.Xw[3 * o], P.Xw[3 * o + 1], P.Xw[3 * o + 2]};
      float pc[3];
      mat3_mul_add(T, xw, tcw, pc);                               // Pc = mRcw*P + mtcw (Frame.cc:586)
      const float pc_dist = norm3(pc);                            // :587
      const float invz = 1.0f / pc[2];                            // :591, float division
      bool in_view = false;
      float px = -1.f, py = -1.f;                                 // :577-578
      float vcos = 0.f;
      int lvl = 0;
      if (!(pc[2] < 0.0f)) {                                      // :592 (-0 and +0 pass)
        float ux, vy;
        project(P.V.cam_type, P.V.cam, pc[0], pc[1], pc[2], ux, vy);   // :595
        if (inside_bounds(ux, vy, P.V.min_x, P.V.max_x, P.V.min_y, P.V.max_y)) {   // :599-602; a NaN projection passes
          px = ux; py = vy;                                       // :605-606
          const float po[3] = {xw[0] - Ow[0], xw[1] - Ow[1], xw[2] - Ow[2]};
          const float dist = norm3(po);                           // :612
          if (!outside_scale_range(dist, P.min_dist, P.max_dist, o)) {   // :614
            const float pn[3] = {P.normal[3 * o], P.normal[3 * o + 1], P.normal[3 * o + 2]};
            vcos = (float)(dot3_double(po, pn) / (double)dist);   // :624, Mat::dot in double
            if (!(vcos < P.view_cos_limit)) {                     // :626
              const float ratio = P.max_dist[o] / dist;           // PredictScale, MapPoint.cc:593-596
              lvl = level_from_log(orblg::ref_logf(ratio), P.log_sf, P.V.nlevels);
              in_view = true;
            }
          }
        }
      }
      P.in_view[o] = in_view ? 1 : 0;
      P.proj_x[o] = px; P.proj_y[o] = py;
      if (in_view) {                                              // :635-644
        const float xr = px - P.mbf * invz;
        P.proj_xr[o] = xr; P.depth[o] = pc_dist; P.level[o] = lvl; P.view_cos[o] = vcos;
        // ORBmatcher.cc:52-73.  A NaN projection finds no candidate in the reference (every |dx| < r test is false): left out.
        if (!(P.bFarPoints && pc_dist > P.th_far) && px == px && py == py) {
          float r = radius_by_viewing_cos(vcos);                  // :216-222
          if (P.th != 1.0f) r *= P.th;                            // :47, :69-70
          u = px; v = py; rad = r * P.V.sf[lvl];                  // :73
          minl = lvl - 1; maxl = lvl;
          ur = xr;
          fl = query_flags(P.obs, o);
        }
      }
    }
  }
  store_query(P.Q, o, u, v, rad, ur, minl, maxl, fl);
}

// ------------------------------------------------------------------------------------------------------------
// The same member for a fisheye-stereo frame (Frame::Nleft != -1): Frame::isInFrustum's else branch (Frame.cc:650-660), i.e.
// Frame::isInFrustumChecks (Frame.cc:1270-1343) once per camera, then the query preparation of both halves of
// SearchByProjection(Frame&, const vector<MapPoint*>&, th, bFarPoints, thFarPoints) (ORBmatcher.cc:44-73 left, :145-151 right).
// Local map point i makes the queries 2i (left image) and 2i + 1 (right image), their side bytes and the doubled descriptor,
// as k_lastframe_project_rig does; query_n[p] = 2 * the live count.  The launch also builds MatchParams::partner from the
// frame's mvLeftToRightMatch / mvRightToLeftMatch (:132-133, :199-200).
// ------------------------------------------------------------------------------------------------------------
struct RigLocalParams {
  float Trl[12], tlr[3];     // Frame::mTrl (row-major 3x4) and mTlr.col(3)
  int cam_type2; float cam2[8];   // mpCamera2 (Frame.cc:1299)
  const uint8_t *mpdesc;     // 32 bytes per local map point (16-byte aligned)
  // out: the R fields of isInFrustumChecks (caller arrays, map stride); proj_xr is LocalMapParams::proj_xr
  uint8_t *in_view_r; float *proj_yr, *depth_r, *view_cos_r; int32_t *level_r;
  uint8_t *qdesc, *qside; int32_t *query_n;   // out, as RigProjectParams
  // partner table: keypoint k < Nleft -> Nleft + l2r[k], k >= Nleft -> r2l[k - Nleft]; an entry outside the other image's live
  // range counts as -1.  partner == NULL: none is built.
  const int32_t *l2r, *r2l;  // [npairs][frame_stride], either may be NULL
  int32_t *partner;          // out: [npairs][frame_stride]
  int frame_stride; LiveCount frame_n, nleft;   // N = frame_n.at(p, frame_stride), Nleft = nleft.at(p, N)
};

// Frame::isInFrustumChecks (Frame.cc:1289-1325) for one camera: T = [mR | mt] (row stride 4), twc, the camera, point o.
struct FrustumSide { bool ok; float u, v, depth, vcos; int level; };

__device__ __forceinline__ FrustumSide frustum_side(const LocalMapParams &P, const float *T, const float *twc, int cam_type, const float *cam,
                                                    const float *xw, size_t o) {
  FrustumSide s = {false, 0.f, 0.f, 0.f, 0.f, -1};
  const float t[3] = {T[3], T[7], T[11]};
  float pc[3];
  mat3_mul_add(T, xw, t, pc);                                     // Pc = mR*P + mt (:1289)
  s.depth = norm3(pc);                                            // :1290
  if (pc[2] < 0.0f) return s;                                     // :1294 (-0 and +0 pass)
  project(cam_type, cam, pc[0], pc[1], pc[2], s.u, s.v);          // :1299-1300
  if (!inside_bounds(s.u, s.v, P.V.min_x, P.V.max_x, P.V.min_y, P.V.max_y)) return s;   // :1302-1305; a NaN projection passes
  const float po[3] = {xw[0] - twc[0], xw[1] - twc[1], xw[2] - twc[2]};
  const float dist = norm3(po);                                   // :1311
  if (outside_scale_range(dist, P.min_dist, P.max_dist, o)) return s;   // :1313
  const float pn[3] = {P.normal[3 * o], P.normal[3 * o + 1], P.normal[3 * o + 2]};
  s.vcos = (float)(dot3_double(po, pn) / (double)dist);           // :1319, Mat::dot in double
  if (s.vcos < P.view_cos_limit) return s;                        // :1321
  const float ratio = P.max_dist[o] / dist;                       // PredictScale, MapPoint.cc:593-596
  s.level = level_from_log(orblg::ref_logf(ratio), P.log_sf, P.V.nlevels);   // :1325
  s.ok = true;
  return s;
}

__global__ __launch_bounds__(256) void k_local_map_project_rig(LocalMapParams P, RigLocalParams G) {
  const int p = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int n = P.map_n.at(p, P.map_stride);
  if (i == 0) G.query_n[p] = 2 * n;
  if (G.partner) {
    const int fn = G.frame_n.at(p, G.frame_stride), nl = G.nleft.at(p, fn);
    const size_t fo = (size_t)p * G.frame_stride;
    for (int k = i; k < G.frame_stride; k += gridDim.x * 256) {
      int pr = -1;
      if (k < nl) {
        const int r = G.l2r ? G.l2r[fo + k] : -1;
        if (r >= 0 && r < fn - nl) pr = nl + r;
      } else if (k < fn) {
        const int l = G.r2l ? G.r2l[fo + (k - nl)] : -1;
        if (l >= 0 && l < nl) pr = l;
      }
      G.partner[fo + k] = pr;
    }
  }
  if (i >= P.map_stride) return;
  const size_t o = (size_t)p * P.map_stride + i;
  float uL = 0.f, vL = 0.f, radL = 0.f, uR = 0.f, vR = 0.f, radR = 0.f;
  int lvlL = 0, lvlR = 0;
  uint8_t flL = 0, flR = 0;
  if (i < n) {
    if (!P.eligible[o]) {
      P.in_view[o] = 0; G.in_view_r[o] = 0;
    } else {
      const float *T = P.Tcw + (size_t)p * 16;
      float Ow[3], Tr[12], Or[3];
      camera_centre(T, Ow);                                       // mOw, Frame.cc:538
      rig_right_pose(T, G.Trl, Tr);                               // Frame.cc:1278-1279
      rig_right_centre(T, G.tlr, Ow, Or);                         // Frame.cc:1280
      const float xw[3] = {P.Xw[3 * o], P.Xw[3 * o + 1], P.Xw[3 * o + 2]};
      const FrustumSide L = frustum_side(P, T, Ow, P.V.cam_type, P.V.cam, xw, o);       // Frame.cc:656
      const FrustumSide R = frustum_side(P, Tr, Or, G.cam_type2, G.cam2, xw, o);        // Frame.cc:657
      P.in_view[o] = L.ok ? 1 : 0; G.in_view_r[o] = R.ok ? 1 : 0;  // :651-652, :656-657
      P.level[o] = L.level; G.level_r[o] = R.level;               // :653-654 (-1), :1330, :1337
      float depth = 0.f;
      if (L.ok) { P.proj_x[o] = L.u; P.proj_y[o] = L.v; P.view_cos[o] = L.vcos; P.depth[o] = depth = L.depth; }   // :1335-1339
      else if (P.bFarPoints && R.ok) depth = P.depth[o];          // mTrackDepth as the MapPoint held it (ORBmatcher.cc:56)
      if (R.ok) { P.proj_xr[o] = R.u; G.proj_yr[o] = R.v; G.view_cos_r[o] = R.vcos; G.depth_r[o] = R.depth; }     // :1328-1332
      // ORBmatcher.cc:53-56.  A NaN projection finds no candidate in the reference (every |dx| < r test is false): left out.
      if ((L.ok || R.ok) && !(P.bFarPoints && depth > P.th_far)) {
        if (L.ok && L.u == L.u && L.v == L.v) {                   // :62-73
          float r = radius_by_viewing_cos(L.vcos);
          if (P.th != 1.0f) r *= P.th;
          uL = L.u; vL = L.v; radL = r * P.V.sf[L.level]; lvlL = L.level;
          flL = query_flags(P.obs, o);
        }
        if (R.ok && R.level != -1 && R.u == R.u && R.v == R.v) {  // :145-151: no th factor (:148)
          uR = R.u; vR = R.v; radR = radius_by_viewing_cos(R.vcos) * P.V.sf[R.level]; lvlR = R.level;
          flR = query_flags(P.obs, o);
        }
      }
    }
  }
  store_query(P.Q, 2 * o, uL, vL, radL, 0.f, flL ? lvlL - 1 : -1, flL ? lvlL : -1, flL);   // Nleft != -1: no mvuRight test (:93)
  store_query(P.Q, 2 * o + 1, uR, vR, radR, 0.f, flR ? lvlR - 1 : -1, flR ? lvlR : -1, flR);
  G.qside[2 * o] = 0; G.qside[2 * o + 1] = 1;
  if (i < n) {
    const uint4 *src = reinterpret_cast<const uint4 *>(G.mpdesc + 32 * o);
    uint4 *dst = reinterpret_cast<uint4 *>(G.qdesc + 64 * o);
    const uint4 a = src[0], b = src[1];
    dst[0] = a; dst[1] = b; dst[2] = a; dst[3] = b;
  }
}

// The search leaves QUERY ids (2i, 2i + 1) in the slots it writes; callers of this member hold local-map indices i.  The slot part
// of k_rot_prune<1> (two steps with a barrier: a converted value could equal another query's id), extended to the stereo partner's
// slot: query j with moq[j] = m owns slot[m] and slot[partner[m]] where it was the last writer.  Slots the search did not write
// are not touched.  One workgroup per problem.
struct RigSlotParams {
  const int32_t *moq; int map_stride; LiveCount map_n;
  const int32_t *partner;   // or NULL
  int32_t *slot; int frame_stride;
};

__global__ __launch_bounds__(256) void k_rig_slot_convert(RigSlotParams S) {
  const int p = blockIdx.x, t = threadIdx.x;
  const int n = 2 * S.map_n.at(p, S.map_stride);
  const size_t qo = 2 * (size_t)p * S.map_stride, ko = (size_t)p * S.frame_stride;
  for (int step = 0; step < 2; step++) {
    for (int j = t; j < n; j += 256) {
      const int m = S.moq[qo + j];
      if (m < 0) continue;
      const int from = step ? -2 - (j >> 1) : j, to = step ? j >> 1 : -2 - (j >> 1);
      if (S.slot[ko + m] == from) S.slot[ko + m] = to;
      const int pr = S.partner ? S.partner[ko + m] : -1;
      if (pr >= 0 && S.slot[ko + pr] == from) S.slot[ko + pr] = to;
    }
    __syncthreads();
  }
}

struct RotPruneParams {
  const float *last_kp;  // query side: angle of LastFrame.mvKeysUn[i] (word 3 of 7)
  int last_stride; LiveCount last_n;
  const float *cur_kp;   // CurrentFrame.mvKeysUn, 7 floats per keypoint
  int frame_stride;
  int32_t *moq;          // match_of_query (in/out: pruned matches become -1)
  int32_t *slot; uint8_t *slot_obs;
  int32_t *nmatches;     // per problem (in/out)
  int prune;             // 0: no histogram (checkOri off); only read by the two-queries-per-point form, which always runs
};

// ORBmatcher.cc:2177-2185 (histogram of the rotation between the matched keypoints) + ComputeThreeMaxima (:2416-2458) +
// :2263-2286 (matches outside the three dominant bins are undone).  One workgroup per frame pair; the bins only need their
// sizes (integer LDS atomics), the order inside a bin does not matter for what is kept.
// QS = 1: fisheye-stereo current frame, two queries (2i, 2i + 1) per last-frame keypoint i, moq [2 * last_stride] per problem.
// The search left QUERY ids in the slots it wrote; callers hold last-frame indices, so the slots are converted first: the holder
// of keypoint k is the LAST query that matched it, which is the one the search left there (slot[k] == j).  Two steps with a
// barrier between them - holder j marks its slot with -2 - (j >> 1), then marked slots become j >> 1 - because a converted
// value could equal another query's id.  Every accepted query has its histogram entry (:2185, :2252) and every pruned entry
// decrements nmatches (:2281-2282), so a keypoint matched by two queries counts twice, as in the reference.
template <int QS>
__global__ __launch_bounds__(256) void k_rot_prune(RotPruneParams R) {
  __shared__ int hist[32];
  __shared__ int keep[3];
  __shared__ int removed;
  const int p = blockIdx.x, t = threadIdx.x;
  const int n = R.last_n.at(p, R.last_stride) << QS;
  const size_t lo = (size_t)p * R.last_stride, qo = lo << QS, ko = (size_t)p * R.frame_stride;
  if (QS) {
    for (int j = t; j < n; j += 256) {
      const int m = R.moq[qo + j];
      if (m >= 0 && R.slot[ko + m] == j) R.slot[ko + m] = -2 - (j >> QS);
    }
    __syncthreads();
    for (int j = t; j < n; j += 256) {
      const int m = R.moq[qo + j];
      if (m >= 0 && R.slot[ko + m] == -2 - (j >> QS)) R.slot[ko + m] = j >> QS;
    }
    if (!R.prune) return;
    __syncthreads();
  }
  if (t < 32) hist[t] = 0;
  if (t == 0) removed = 0;
  __syncthreads();
  for (int i = t; i < n; i += 256) {
    const int m = R.moq[qo + i];
    if (m < 0) continue;
    const int bin = rot_bin(R.last_kp[7 * (lo + (i >> QS)) + 3] - R.cur_kp[7 * (ko + m) + 3]);
    if (bin >= 0 && bin < ORBM_HISTO_LENGTH) atomicAdd(&hist[bin], 1);
  }
  __syncthreads();
  if (t == 0) {
    int ind1, ind2, ind3;
    three_maxima(hist, ORBM_HISTO_LENGTH, ind1, ind2, ind3);
    keep[0] = ind1; keep[1] = ind2; keep[2] = ind3;
  }
  __syncthreads();
  const int k0 = keep[0], k1 = keep[1], k2 = keep[2];
  int mine = 0;
  for (int i = t; i < n; i += 256) {
    const int m = R.moq[qo + i];
    if (m < 0) continue;
    const int bin = rot_bin(R.last_kp[7 * (lo + (i >> QS)) + 3] - R.cur_kp[7 * (ko + m) + 3]);
    if (bin < 0 || bin >= ORBM_HISTO_LENGTH || bin == k0 || bin == k1 || bin == k2) continue;
    R.slot[ko + m] = -1;
    R.slot_obs[ko + m] = 0;
    R.moq[qo + i] = -1;
    mine++;
  }
  if (mine) atomicAdd(&removed, mine);
  __syncthreads();
  if (t == 0 && removed) R.nmatches[p] -= removed;
}

// ------------------------------------------------------------------------------------------------------------
// G0: Frame::UndistortKeyPoints (Frame.cc:837-870) for frames resident in HBM - the step between operator() and the
// searches in the Frame constructor.  cv::undistortPoints(pts, K, D, R = I, P = K) restated: five
// fixed-point iterations in double, every operation in source order (no contraction; fp64 division and the
// double -> float conversions are IEEE on gfx950), i.e. the same bits as the host function orbm_undistort_keypoints
// through the same undistort_point (orb_ref_geometry.h), which tests/test_gpu_distort.py checks.  One thread per keypoint; only pt changes (:862-868).
// ------------------------------------------------------------------------------------------------------------
struct UndistortParams {
  const float *keys;           // orbx_keypoint_t AoS viewed as floats, frame f at element offset f * key_stride
  float *keys_un;              // may alias keys
  int key_stride; LiveCount count;   // N of frame f: count.at(f, key_stride)
  float K[4], D[5]; int nD;
};

__global__ __launch_bounds__(256) void k_undistort(UndistortParams U) {
  const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  const int n = U.count.at(f, U.key_stride);
  if (i >= n) return;
  const size_t o = ((size_t)f * U.key_stride + i) * 7;
  float k[7];
#pragma unroll
  for (int t = 0; t < 7; t++) k[t] = U.keys[o + t];
  if (U.D[0] != 0.0f) undistort_point((double)k[0], (double)k[1], U.K, U.D, U.nD, &k[0], &k[1]);   // :839-843: D[0] == 0 copies
#pragma unroll
  for (int t = 0; t < 7; t++) U.keys_un[o + t] = k[t];
}

// ------------------------------------------------------------------------------------------------------------
// The Frame of a two-camera fisheye rig (Frame.cc:1162-1164, :1201) from two resident extractions: mvKeys followed by
// mvKeysRight, mDescriptors = vconcat(left, right), N = Nleft + Nright.  Frame f: the nL left entries, then the nR right
// entries directly behind them; entries beyond nL + nR are not written.  One thread per 16-byte half of a descriptor, then
// one per dword of a keypoint: the right image's keypoints land at (f * 2 * cap + nL) * 28 bytes, which is a multiple of 4
// only, so the key array moves as dwords (a wavefront still moves 256 contiguous bytes per instruction).
// ------------------------------------------------------------------------------------------------------------
struct RigConcatParams {
  const uint32_t *keysL, *keysR;   // [nframes][cap] keypoints as 7 dwords each
  const uint4 *descL, *descR;      // [nframes][cap] descriptors as 2 x 16 bytes each
  const int32_t *countsL, *countsR;   // [nframes][2], element 0 = n
  int cap;
  uint32_t *keys; uint4 *desc;     // out: [nframes][2 * cap]
  int32_t *n;                      // out: [nframes][2] = {nL + nR, nL}
};

__global__ __launch_bounds__(256) void k_rig_concat(RigConcatParams R) {
  const int f = blockIdx.y;
  const int nL = clamp_count(R.countsL[2 * (size_t)f], R.cap), nR = clamp_count(R.countsR[2 * (size_t)f], R.cap);
  const int N = nL + nR;   // <= 2 * cap
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t == 0) { R.n[2 * (size_t)f] = N; R.n[2 * (size_t)f + 1] = nL; }
  const size_t src = (size_t)f * R.cap, dst = (size_t)f * 2 * R.cap;
  if (t < 2LL * N) {                     // descriptor halves [0, 2 N)
    const int e = (int)(t >> 1), h = (int)(t & 1);
    R.desc[2 * (dst + e) + h] = e < nL ? R.descL[2 * (src + e) + h] : R.descR[2 * (src + (e - nL)) + h];
  } else if (t < 9LL * N) {              // keypoint dwords [0, 7 N)
    const long long w = t - 2LL * N;
    R.keys[7 * dst + w] = w < 7LL * nL ? R.keysL[7 * src + w] : R.keysR[7 * src + (w - 7LL * nL)];
  }
}
