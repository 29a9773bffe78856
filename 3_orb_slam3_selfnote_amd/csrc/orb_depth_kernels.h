// orb_depth_kernels.h -- what an RGB-D (and a stereo) frame needs between undistortion and the next frame's stereo-mode search,
// for batches resident in HBM.  Included by orbhip.hip after orb_project_kernels.h (orb_ref_geometry.h).  One workgroup per frame
// in both kernels: a frame has about a thousand keypoints, a batch has hundreds of frames.
//   k_stereo_from_rgbd  Frame::ComputeStereoFromRGBD (Frame.cc:1082-1103): mvDepth / mvuRight from the depth image, with the
//                       convertTo(CV_32F, mDepthMapFactor) of Tracking::GrabImageRGBD (Tracking.cc:1075-1076) evaluated only at
//                       the keypoints' pixels: a gather of N pixels instead of a pass over rows x cols.
//   k_close_points      the depth-ordered rule of Tracking::UpdateLastFrame (Tracking.cc:2808-2860) and
//                       Tracking::CreateNewKeyFrame (:3345-3416), the close counts of Tracking::NeedNewKeyFrame (:3183-3204) and
//                       Frame::UnprojectStereo (Frame.cc:1105-1116).
#pragma once
#include "orb_sort.h"

// ---- Frame::ComputeStereoFromRGBD ------------------------------------------------------------------------------------------------

struct RgbdParams {
  const float *keys, *keys_un;                   // [nframes][cap] keypoints, 7 floats each: mvKeys (the pixel), mvKeysUn (pt.x)
  const int32_t *counts; int count_stride, cap;  // N of frame f = counts[f * count_stride]
  const uint8_t *img; int depth_type, rows, cols; size_t row_stride, frame_stride;   // strides in bytes
  float factor, mbf;
  float *uRight, *depth; int32_t *nstereo;       // [nframes][cap]; nstereo may be NULL
};

__device__ __forceinline__ int depth_live(const int32_t *counts, int count_stride, int f, int cap) {
  return clamp_count(counts[(size_t)f * count_stride], cap);
}

// One pixel of `imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor)` (Tracking.cc:1076).  [OPENCV-UNVERIFIED]: cvtScale for
// 16U -> 32F and for 32F -> 32F works in float with a float scale and beta = 0, i.e. (float)raw * scale (+ 0.0f, which changes
// no value that passes d > 0).  The reference skips the conversion when the image is CV_32F and the factor is (within 1e-5 of)
// 1 (:1075); multiplying by 1.0f is exact, so that case needs no path of its own: the caller passes depth_factor = 1.
__device__ __forceinline__ float depth_at(const uint8_t *img, int depth_type, size_t row_stride, int r, int c, float factor) {
  const uint8_t *row = img + (size_t)r * row_stride;
  const float raw = depth_type == 0 ? (float)reinterpret_cast<const uint16_t *>(row)[c] : reinterpret_cast<const float *>(row)[c];
  return raw * factor;
}

__global__ __launch_bounds__(256) void k_stereo_from_rgbd(RgbdParams P) {
  __shared__ int s_n;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int n = depth_live(P.counts, P.count_stride, f, P.cap);
  const float *keys = P.keys + (size_t)f * P.cap * 7, *keys_un = P.keys_un + (size_t)f * P.cap * 7;
  const uint8_t *img = P.img + (size_t)f * P.frame_stride;
  float *uRight = P.uRight + (size_t)f * P.cap, *depth = P.depth + (size_t)f * P.cap;
  if (tid == 0) s_n = 0;
  __syncthreads();
  int mine = 0;
  for (int i = tid; i < n; i += 256) {
    // imDepth.at<float>(v, u) with float arguments (Frame.cc:1092-1095): both are converted to int, i.e. truncated
    const int r = x86_cvtt_f32_i32(keys[(size_t)i * 7 + 1]), c = x86_cvtt_f32_i32(keys[(size_t)i * 7 + 0]);
    float z = -1.0f, ur = -1.0f;
    // a pixel outside the image is undefined behaviour in the reference (Mat::at does not check in a release build): here -1,
    // the one stated deviation
    if ((unsigned)r < (unsigned)P.rows && (unsigned)c < (unsigned)P.cols) {
      const float d = depth_at(img, P.depth_type, P.row_stride, r, c, P.factor);
      if (d > 0) {                                      // :1097-1101; NaN fails, +inf gives depth inf and uRight = kpU.pt.x
        z = d;
        ur = keys_un[(size_t)i * 7 + 0] - P.mbf / d;
        mine++;
      }
    }
    depth[i] = z;
    uRight[i] = ur;
  }
  if (P.nstereo) {
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
    if (tid == 0) P.nstereo[f] = s_n;
  }
}

// ---- close points ----------------------------------------------------------------------------------------------------------------

#define CLOSE_THREADS 512

struct CloseParams {
  const float *depth;                            // [nframes][cap] mvDepth
  const int32_t *counts; int count_stride, cap;
  float th_depth; int max_point;                 // mThDepth; maxPoint (100 in both loops, Tracking.cc:2856, :3341-3343)
  const uint8_t *tracked;                        // [nframes][cap] mvpMapPoints[i] && !mvbOutlier[i], or NULL = none
  int32_t *order, *nvisit, *close;               // [nframes][cap], [nframes], [nframes][2] or NULL
  const float *keys_un; float cx, cy, invfx, invfy;
  float *x3Dc; const float *pose; float *x3Dw;   // [nframes][cap][3] or NULL; pose [nframes][12] = [Rwc | Ow] row-major
};

// sort(vDepthIdx) orders pair<float, int> by z, then by i.  z > 0 here, and positive floats (+inf included) order as their bit
// patterns, so the pair orders as this integer; keypoints without depth get the largest key and sort behind every pair.
// The keys are unique, so any correct sort gives the reference's order: a bitonic sort in LDS (orb_sort.h), padded to a power of two.  Measured
// against rank-by-counting (each keypoint counts the keys below its own) on 256 frames of 1205 keypoints: 0.033 ms against
// 0.060 ms for this kernel (profiles/rgbd_batch_sort_choice.txt), and the count grows with N * N.
__device__ __forceinline__ uint64_t close_key(float z, int i) {
  return z > 0 ? ((uint64_t)__float_as_uint(z) << 32) | (uint32_t)i : ~0ull;
}

__global__ __launch_bounds__(CLOSE_THREADS) void k_close_points(CloseParams P) {
  __shared__ uint64_t s_key[ORBX_CLOSE_MAX_KEYPOINTS];
  __shared__ int s_cnt[4];   // m = #{z > 0}, c = #{0 < z <= th_depth}, nTrackedClose, nNonTrackedClose
  const int f = blockIdx.x, tid = threadIdx.x;
  const int n = depth_live(P.counts, P.count_stride, f, P.cap);
  const float *depth = P.depth + (size_t)f * P.cap;
  if (tid < 4) s_cnt[tid] = 0;
  __syncthreads();
  int m = 0, c = 0, nt = 0, nn = 0;
  for (int i = tid; i < n; i += CLOSE_THREADS) {
    const float z = depth[i];
    s_key[i] = close_key(z, i);
    if (z > 0) {
      m++;
      c += !(z > P.th_depth);                           // the complement of the break's `first > mThDepth` (:2856, :3412)
      if (z < P.th_depth) {                             // :3192
        const bool tr = P.tracked && P.tracked[(size_t)f * P.cap + i];
        nt += tr; nn += !tr;
      }
      if (P.x3Dc) {                                     // Frame::UnprojectStereo, Frame.cc:1107-1115
        const float *ku = P.keys_un + ((size_t)f * P.cap + i) * 7;
        const float u = ku[0], v = ku[1];
        const float x3Dc[3] = {(u - P.cx) * z * P.invfx, (v - P.cy) * z * P.invfy, z};
        float *o = P.x3Dc + ((size_t)f * P.cap + i) * 3;
        o[0] = x3Dc[0]; o[1] = x3Dc[1]; o[2] = x3Dc[2];
        if (P.x3Dw) {
          const float *T = P.pose + (size_t)f * 12;
          const float Ow[3] = {T[3], T[7], T[11]};
          float x3Dw[3];
          mat3_mul_add(T, x3Dc, Ow, x3Dw);              // mRwc * x3Dc + mOw
          float *w = P.x3Dw + ((size_t)f * P.cap + i) * 3;
          w[0] = x3Dw[0]; w[1] = x3Dw[1]; w[2] = x3Dw[2];
        }
      }
    }
  }
  if (m) atomicAdd(&s_cnt[0], m);
  if (c) atomicAdd(&s_cnt[1], c);
  if (nt) atomicAdd(&s_cnt[2], nt);
  if (nn) atomicAdd(&s_cnt[3], nn);
  const int p2 = sort_p2(n);
  for (int i = n + tid; i < p2; i += CLOSE_THREADS) s_key[i] = ~0ull;
  __syncthreads();
  m = s_cnt[0]; c = s_cnt[1];
  // `if (first > mThDepth && nPoints > maxPoint) break` with nPoints = position + 1 on every iteration (:2849-2859, :3405-3415):
  // the break comes at position max(c, maxPoint), after that point has been visited
  const int last = max(c, P.max_point);
  const int nvisit = last >= m ? m : last + 1;
  int32_t *order = P.order + (size_t)f * P.cap;
  bitonic_sort_lds<CLOSE_THREADS>(s_key, p2, tid);
  for (int t = tid; t < nvisit; t += CLOSE_THREADS) order[t] = (int32_t)(uint32_t)s_key[t];
  if (tid == 0) {
    P.nvisit[f] = nvisit;
    if (P.close) { P.close[2 * f] = s_cnt[2]; P.close[2 * f + 1] = s_cnt[3]; }
  }
}
