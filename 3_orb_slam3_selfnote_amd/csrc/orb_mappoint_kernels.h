// orb_mappoint_kernels.h -- MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:350-436) and MapPoint::UpdateNormalAndDepth
// (MapPoint.cc:467-547) for all map points of one call (orbm_update_map_points; LocalMapping.cc:1040-1053): one wavefront per map point,
// four per workgroup, the layout of k_distinctive.  The descriptor choice is integer work; every floating-point operation is a function
// of orb_ref_mappoint.h, the host's own definition - the kernel holds no arithmetic of its own.
#pragma once
#include "orb_match_kernels.h"
#include "orb_ref_mappoint.h"

struct MapPointUpdateParams {
  const uint32_t *desc;       // [nobs][8]
  const int32_t *start;       // [nmp + 1]
  const float *centre;        // [nobs][3]
  const uint8_t *in_desc;     // [nobs]
  const float *pos, *ref_centre, *ref_scale, *ref_max_scale;
  int nmp;
  int32_t *best;              // [nmp]
  float *normal, *min_dist, *max_dist;   // [nmp][3], [nmp], [nmp]; not written for a point without entries
};

__device__ __forceinline__ uint32_t mp_lane_read(uint32_t v, int src) { return (uint32_t)__builtin_amdgcn_readlane((int)v, src); }
__device__ __forceinline__ float mp_lane_read(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }

// smallest v with #{lanes : d <= v} >= need, by bisection on ballot counts (d = 0x7fff is never counted)
__device__ __forceinline__ int mp_kth_distance(int d, int need) {
  int lo = 0, hi = 256;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (__popcll(__ballot(d <= mid)) >= need) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_update_map_points(MapPointUpdateParams P) {
  const int lane = threadIdx.x & 63;
  const int mp = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (mp >= P.nmp) return;
  const int s0 = P.start[mp], N = P.start[mp + 1] - s0;
  if (N <= 0) { if (lane == 0) P.best[mp] = -1; return; }      // observations.empty(), :365 / :483: nothing else is written
  int bestMedian = 0x7fffffff, bestIdx = -1;                    // -1: no flagged entry, vDescriptors.empty() (:389)
  if (N <= 64) {
    // lane j holds entry j's descriptor; row i reaches the lanes by a lane read of these registers
    uint32_t r[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    bool flagged = false;
    if (lane < N) {
      const uint4 *row = (const uint4 *)(P.desc + (size_t)(s0 + lane) * 8);
      const uint4 a = row[0], b = row[1];
      r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
      flagged = P.in_desc[(size_t)s0 + lane] != 0;             // !pKF->isBad(), :375
    }
    unsigned long long rows = __ballot(flagged);
    const int need = (int)(0.5 * (double)(__popcll(rows) - 1)) + 1;   // vDists[0.5*(N-1)], :419, over the flagged entries
    while (rows) {
      const int i = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(rows));
      rows &= rows - 1;
      int dist = 0;
#pragma unroll
      for (int w = 0; w < 8; w++) dist += __popc(mp_lane_read(r[w], i) ^ r[w]);
      const int median = mp_kth_distance(flagged ? dist : 0x7fff, need);
      if (median < bestMedian) { bestMedian = median; bestIdx = i; }   // :422-426, strict: the first row wins
    }
  } else {
    // k_distinctive's tiled form (entry j = lane + 64 t), restricted to the flagged entries
    const int nt = (N + 63) >> 6;
    uint32_t fl = 0;                                            // bit t: entry lane + 64 t is flagged
    int nflag = 0;
#pragma unroll
    for (int t = 0; t < DISTINCT_MAXT; t++) {
      const int j = lane + 64 * t;
      const bool f = t < nt && j < N && P.in_desc[(size_t)s0 + j] != 0;
      fl |= (uint32_t)f << t;
      nflag += __popcll(__ballot(f));
    }
    const int need = (int)(0.5 * (double)(nflag - 1)) + 1;
    for (int i = 0; i < N; i++) {
      if (!((mp_lane_read(fl, i & 63) >> (i >> 6)) & 1u)) continue;
      uint32_t di[8];
#pragma unroll
      for (int w = 0; w < 8; w++) di[w] = P.desc[(size_t)(s0 + i) * 8 + w];
      int d[DISTINCT_MAXT];
#pragma unroll
      for (int t = 0; t < DISTINCT_MAXT; t++) {
        d[t] = 0x7fff;
        if ((fl >> t) & 1u) {
          int dist = 0;
#pragma unroll
          for (int w = 0; w < 8; w++) dist += __popc(di[w] ^ P.desc[(size_t)(s0 + lane + 64 * t) * 8 + w]);
          d[t] = dist;
        }
      }
      int lo = 0, hi = 256;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int cnt = 0;
#pragma unroll
        for (int t = 0; t < DISTINCT_MAXT; t++)
          if (t < nt) cnt += __popcll(__ballot(d[t] <= mid));
        if (cnt >= need) hi = mid; else lo = mid + 1;
      }
      if (lo < bestMedian) { bestMedian = lo; bestIdx = i; }
    }
  }
  // :486-511: lane j forms its entry's term, the sum runs in entry order over wave-uniform lane reads (every entry, flagged or not)
  const float pos[3] = {P.pos[3 * (size_t)mp], P.pos[3 * (size_t)mp + 1], P.pos[3 * (size_t)mp + 2]};
  float sum[3] = {0.f, 0.f, 0.f};
  for (int base = 0; base < N; base += 64) {
    const int cnt = min(64, N - base);
    float term[3] = {0.f, 0.f, 0.f};
    if (lane < cnt) mp_normal_term(pos, P.centre + 3 * ((size_t)s0 + base + lane), term);
    for (int e = 0; e < cnt; e++) {
      const float te[3] = {mp_lane_read(term[0], e), mp_lane_read(term[1], e), mp_lane_read(term[2], e)};
      mp_normal_add(sum, te);
    }
  }
  if (lane == 0) {
    P.best[mp] = bestIdx;
    mp_finish(sum, N, pos, P.ref_centre + 3 * (size_t)mp, P.ref_scale[mp], P.ref_max_scale[mp], P.normal + 3 * (size_t)mp, P.min_dist + mp,
              P.max_dist + mp);
  }
}
