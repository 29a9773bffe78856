// orb_rig_stereo_kernels.h -- Frame::ComputeStereoFishEyeMatches (Frame.cc:1228-1268) for resident rig batches: the brute-force
// knnMatch(k = 2) between the lapping rows of the two extractions on the matrix pipe (k_rig_stereo_knn2, the product of k_knn2_mfma),
// then Lowe's ratio test and KannalaBrandt8::TriangulateMatches, one match per lane (k_rig_stereo_triangulate).  One grid covers all
// frames; the per-frame row ranges are read from the extractions' own count arrays.
#pragma once
#include "orb_common.h"
#include "orb_match_mfma.h"
#include "orb_ref_triangulate.h"

struct RigStereoParams {
  const uint32_t *keysL, *keysR;   // [nframes][cap] keypoints of 7 words (x, y, size, angle, response, octave, class_id)
  const uint32_t *descL, *descR;   // [nframes][cap][8]
  const int32_t *countsL, *countsR;   // [nframes][2] = {n, monoIndex}
  int cap, out_stride, nlevels;
  float sigma2[16];                // mvLevelSigma2
  float Tlr[12], Tcw2[12];         // [R12 | t12] and rig_Tcw2 of it
  float cam1[8], cam2[8];
  int32_t *l2r, *r2l;              // [nframes][out_stride]
  float *depth, *p3d;              // [nframes][out_stride], [nframes][out_stride][3]
  int32_t *nmatches;               // [nframes][2] = {nMatches, descMatches} or NULL
  uint32_t *knn;                   // scratch [nframes][cap][2]: ham << 20 | train row, per lapping query row
};

// Frame f's counts as the extraction wrote them, taken into range: N in [0, cap], monoIndex in [0, N]
struct RigLap { int nL, monoL, nR, monoR; };
__device__ __forceinline__ RigLap rig_lap(const RigStereoParams &P, int f) {
  RigLap r;
  r.nL = clamp_count(P.countsL[2 * f], P.cap); r.monoL = clamp_count(P.countsL[2 * f + 1], r.nL);
  r.nR = clamp_count(P.countsR[2 * f], P.cap); r.monoR = clamp_count(P.countsR[2 * f + 1], r.nR);
  return r;
}

// Grid (ceil(cap / MF_NT), nframes).  Resets the frame's live output entries (:1236-1238; the triangulation kernel behind it on the
// stream writes matches only), then the two nearest right lapping rows of every left lapping row.
__global__ __launch_bounds__(MF_NT) void k_rig_stereo_knn2(RigStereoParams P) {
  __shared__ __align__(16) uint8_t sA[2][MF_TILE * 256];
  const int f = blockIdx.y, i = blockIdx.x * MF_NT + threadIdx.x;
  const RigLap lap = rig_lap(P, f);
  const size_t o = (size_t)f * P.out_stride;
  if (i < lap.nL) { P.l2r[o + i] = -1; P.depth[o + i] = -1.0f; }
  if (i < lap.nR) P.r2l[o + i] = -1;
  if (P.nmatches && i < 2) P.nmatches[2 * f + i] = 0;
  const int nq = lap.nL - lap.monoL, nc = lap.nR - lap.monoR;
  if ((int)(blockIdx.x * MF_NT) >= nq || nc < 2) return;   // the whole workgroup; fewer than two train rows: no match (:1253)
  const size_t fo = (size_t)f * P.cap;
  uint32_t mine[2];
  const int qi = knn2_mfma_pairs(P.descL + (fo + lap.monoL) * 8, nq, P.descR + (fo + lap.monoR) * 8, nc, blockIdx.x, sA, mine);
  if (qi < nq) *reinterpret_cast<uint2 *>(P.knn + (fo + qi) * 2) = make_uint2(mine[0], mine[1]);
}

// Grid (ceil(cap / 256), nframes): lane = left lapping row (:1252-1266, one iteration of the loop).  mvRightToLeftMatch keeps the
// LAST accepted left keypoint in left order, the sequential loop's result: an atomic maximum over the left indices.
__global__ __launch_bounds__(256) void k_rig_stereo_triangulate(RigStereoParams P) {
  const int f = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
  const RigLap lap = rig_lap(P, f);
  const int nq = lap.nL - lap.monoL, nc = lap.nR - lap.monoR;
  if ((int)(blockIdx.x * 256) >= nq || nc < 2) return;
  const size_t fo = (size_t)f * P.cap, o = (size_t)f * P.out_stride;
  bool desc_match = false, match = false;
  if (q < nq) {
    const uint2 k = *reinterpret_cast<const uint2 *>(P.knn + (fo + q) * 2);
    desc_match = fisheye_ratio_test((int)(k.x >> 20), (int)(k.y >> 20));
    if (desc_match) {
      const int li = q + lap.monoL, rj = (int)(k.x & 0xfffffu) + lap.monoR;
      const uint32_t *kl = P.keysL + (fo + li) * 7, *kr = P.keysR + (fo + rj) * 7;
      const int octL = (int)kl[5], octR = (int)kr[5];
      if (octL >= 0 && octL < P.nlevels && octR >= 0 && octR < P.nlevels) {   // mvLevelSigma2[octave], :1257
        float p3D[3];
        const float depth = kb8_triangulate_matches(P.cam1, P.cam2, __uint_as_float(kl[0]), __uint_as_float(kl[1]), __uint_as_float(kr[0]),
                                                    __uint_as_float(kr[1]), P.Tlr, P.Tcw2, P.sigma2[octL], P.sigma2[octR], p3D);
        if (depth > 0.0001f) {
          match = true;
          P.l2r[o + li] = rj;
          atomicMax(&P.r2l[o + rj], li);
          P.depth[o + li] = depth;
          float *d = P.p3d + (o + li) * 3;
          d[0] = p3D[0]; d[1] = p3D[1]; d[2] = p3D[2];
        }
      }
    }
  }
  if (P.nmatches) {
    const int nm = __popcll(__ballot(match)), nd = __popcll(__ballot(desc_match));
    if ((threadIdx.x & 63) == 0) {
      if (nm) atomicAdd(&P.nmatches[2 * f], nm);
      if (nd) atomicAdd(&P.nmatches[2 * f + 1], nd);
    }
  }
}

// The device build of the restated arithmetic on n items (orbm_fisheye_triangulate_device): the tests compare it with the host build,
// which the CPU tests compare with the numpy model.
struct TriangulateParams {
  const float *kp1, *kp2, *sigma1, *sigma2;   // [n][2], [n][2], [n], [n]
  float Tlr[12], Tcw2[12], cam1[8], cam2[8];
  float *depth, *p3d;                          // [n], [n][3]
  int n;
};
__global__ __launch_bounds__(256) void k_fisheye_triangulate(TriangulateParams P) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P.n) return;
  // p3D is written where TriangulateMatches reaches its end (:409), as the host loop of orbm_fisheye_triangulate does
  P.depth[i] = kb8_triangulate_matches(P.cam1, P.cam2, P.kp1[2 * i], P.kp1[2 * i + 1], P.kp2[2 * i], P.kp2[2 * i + 1], P.Tlr, P.Tcw2, P.sigma1[i],
                                       P.sigma2[i], P.p3d + 3 * (size_t)i);
}
