// orb_ref_mappoint.h -- MapPoint::UpdateNormalAndDepth (MapPoint.cc:486-545) stated once for the host entry orbm_map_point_normal_depth
// and k_update_map_points, under the contract of orb_ref_geometry.h / orb_ref_newpoints.h: IEEE-754 single / double operations in the
// reference's order, no contraction, correctly rounded divide and sqrt.
//   * `normali = mWorldPos - Owi` (:501, :507) and `PC = Pos - Ow` (:514): float subtraction per component.
//   * cv::norm(normali), cv::norm(PC): dot3_double and a double sqrt; `const float dist` (:516) rounds it once (norm3).
//   * `normal = normal + normali/cv::norm(normali)` (:502, :508): [OPENCV-UNVERIFIED], stated in mp_normal_term / mp_normal_add and nowhere
//     else.  OpenCV 3.4 builds ONE MatOp_AddEx expression with a = normali, alpha = 1.0 / norm (a double), b = normal, beta = 1, and
//     evaluates it with cv::scaleAdd; for CV_32F that is dst[i] = src1[i] * (float)alpha + src2[i]: alpha is rounded to float first, the
//     product is rounded to float, then the sum is rounded.  It is not fused and it is not a division by the norm.  Read from matop.cpp
//     and arithm.cpp, not checked against a build of OpenCV (unpinned list).
//   * `mNormalVector = normal/n` (:545): the "matrix divided by a scalar, assigned" form of orb_ref_newpoints.h,
//     (float)((double)v * (1.0 / (double)n)).
//   * mfMaxDistance = dist*levelScaleFactor (:543) a float product, mfMinDistance = mfMaxDistance/mvScaleFactors[nLevels-1] (:544) a float
//     division.
// The sum over the observations is sequential in the caller's order (std::map order, left index before right index of one keyframe).
// A point in a camera centre gives 1.0 / 0 = inf, 0 * inf = NaN and NaN from there on; nothing here tests for it.
#pragma once
#include "orb_ref_geometry.h"

#define ORB_REF __host__ __device__ __forceinline__

// normali / cv::norm(normali) as scaleAdd forms it: the three rounded products src1[i] * (float)alpha
ORB_REF void mp_normal_term(const float *pos, const float *centre, float *term) {
  const float normali[3] = {pos[0] - centre[0], pos[1] - centre[1], pos[2] - centre[2]};
  const float alpha = (float)(1.0 / sqrt(dot3_double(normali, normali)));
#pragma unroll
  for (int k = 0; k < 3; k++) term[k] = normali[k] * alpha;
}

// ... + src2[i]: one step of the walk
ORB_REF void mp_normal_add(float *normal, const float *term) {
#pragma unroll
  for (int k = 0; k < 3; k++) normal[k] = term[k] + normal[k];
}

// :514-516 and :543-545 from the finished sum over n entries
ORB_REF void mp_finish(const float *sum, int n, const float *pos, const float *ref_centre, float ref_scale, float ref_max_scale, float *normal,
                       float *min_dist, float *max_dist) {
  const float PC[3] = {pos[0] - ref_centre[0], pos[1] - ref_centre[1], pos[2] - ref_centre[2]};
  const float dist = norm3(PC);
  const float maxd = dist * ref_scale;
  *max_dist = maxd;
  *min_dist = maxd / ref_max_scale;
  const double inv = 1.0 / (double)n;
#pragma unroll
  for (int k = 0; k < 3; k++) normal[k] = (float)((double)sum[k] * inv);
}

// :486-545 for one map point with n >= 1 entries
ORB_REF void map_point_normal_depth(int n, const float *centre, const float *pos, const float *ref_centre, float ref_scale, float ref_max_scale,
                                    float *normal, float *min_dist, float *max_dist) {
  float sum[3] = {0.f, 0.f, 0.f}, term[3];   // cv::Mat::zeros(3,1,CV_32F)
  for (int e = 0; e < n; e++) {
    mp_normal_term(pos, centre + 3 * (size_t)e, term);
    mp_normal_add(sum, term);
  }
  mp_finish(sum, n, pos, ref_centre, ref_scale, ref_max_scale, normal, min_dist, max_dist);
}

#undef ORB_REF
