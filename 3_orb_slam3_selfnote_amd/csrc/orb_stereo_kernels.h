// orb_stereo_kernels.h -- Frame::ComputeStereoMatches (Frame.cc:901-1079), rectified stereo: the whole stereo path.  Included by
// orbhip.hip after orb_match_kernels.h (wave helpers, ORBM_TH_*).  Two forms share the arithmetic that decides results - the row range
// of a right keypoint, the candidate gates and key, the window test, the sub-pixel fit (the stereo_* device functions below, each
// stated once) - and differ in who looks at what:
//  host arrays, one frame pair (orbx_compute_stereo_matches):
//   k_stereo_match   one wavefront per LEFT keypoint.  Lanes over all right keypoints: row range, octave window, disparity window,
//                    Hamming; wave minimum of (dist << 16 | iR) = first minimum in iR order (:966).  Then the 11x11 SAD at 11
//                    horizontal offsets on the two level images (lanes over the 121 pixels, global reads, DPP wave sums).  The median
//                    filter over the accepted matches (:1060-1073) needs a sort of <= N pairs and stays on the host.
//  a batch of frame pairs resident in HBM (orbx_compute_stereo_matches_batch_device):
//   k_stereo_rows    the reference's row table (vRowIndices, :911-928) as a CSR table of STEREO_BAND-row bands, one workgroup per
//                    frame pair.  A record is 16 bytes (u, the exact row range, octave | index): a candidate is rejected without
//                    touching its 28-byte keypoint or its descriptor.  Order inside a band is whatever the LDS atomics give: the
//                    search takes a minimum over (dist << 16 | iR), which is the reference's "first minimum in iR order" (:978).
//   k_stereo_search  8 left keypoints per wavefront, 8 lanes each, over the band of the keypoint's row (exact row test repeated
//                    per record); then, per accepted keypoint, the whole wavefront on the 11 SAD windows: the 11 x 21 strip of
//                    the right level is staged once in LDS, the 11 sums travel through the DPP reduction two to a register.
//   k_stereo_median  the median filter (:1065-1078) as an order statistic: rank nDI / 2 of the accepted SADs by two 256-bin
//                    histogram passes (a SAD is at most 121 * 510 = 61710 < 2^16), one workgroup per frame pair.
#pragma once

#define STEREO_BAND 8          // rows per band of the row table
#define STEREO_BAND_SHIFT 3
#define STEREO_MAX_BANDS 512   // orbx_configure takes images up to 4096 rows
#define STEREO_KPW 8           // left keypoints per wavefront in the search phase (8 lanes each)
#define STEREO_KPB (4 * STEREO_KPW)   // ... per workgroup of 256 threads

struct StereoRec { float u; int32_t minr, maxr; uint32_t octIdx; };   // octIdx = octave << 16 | iR

struct StereoBatchParams {
  const uint8_t *imgL0, *imgR0; size_t strideL0, strideR0, fsL0, fsR0;   // level 0 in place: frame f at img + f * fs
  const uint8_t *pyrL, *pyrR; size_t pyrFsL, pyrFsR;                      // pyramid blocks (levels >= 1), frame stride
  int w[ORB_MAXL], h[ORB_MAXL], pitch[ORB_MAXL]; size_t off[ORB_MAXL];
  float sf[ORB_MAXL], invsf[ORB_MAXL];
  int nlevels, rows, nbands;
  const float *kpL, *kpR;                                                 // [nframes][cap] keypoints, 7 floats each
  const uint32_t *descL, *descR;                                          // [nframes][cap][8]
  const int32_t *countsL, *countsR;                                       // [nframes][2]
  int cap, recCap;                                                        // recCap: records per frame in `recs`
  float mb, mbf;
  StereoRec *recs; int32_t *bandStart;                                    // [nframes][recCap], [nframes][nbands + 1]
  float *uRight, *depth; int32_t *sad, *nstereo;                          // [nframes][cap]; sad = -1: no match; nstereo may be NULL
};

__device__ __forceinline__ int stereo_live(const int32_t *counts, int f, int cap) { return clamp_count(counts[2 * f], cap); }

#define STEREO_W 5   // half width of the SAD window (w, :991)
#define STEREO_L 5   // half width of the sliding range (L, :998)

// The rows a right keypoint is a candidate for (:916-918).  maxOct bounds the index into sf: k_stereo_match passes ORB_MAXL - 1,
// k_stereo_rows nlevels - 1; the two differ only for octaves no extractor produces, and each kernel keeps its own.
__device__ __forceinline__ void stereo_row_range(const float *sf, int maxOct, float yR, int oR, int *minr, int *maxr) {
  const float r = 2.0f * sf[min(max(oR, 0), maxOct)];                       // :916
  *maxr = (int)ceilf(yR + r); *minr = (int)floorf(yR - r);                  // :917-918
}

// The two gates of a right keypoint in the left keypoint's row: the octave window (:954) and the disparity window (:959)
__device__ __forceinline__ bool stereo_octave_outside(int oR, int levelL) { return oR < levelL - 1 || oR > levelL + 1; }
__device__ __forceinline__ bool stereo_u_outside(float uR, float minU, float maxU) { return !(uR >= minU && uR <= maxU); }
// bestDist starts at TH_HIGH and is replaced on strict <; the minimum of dist << 16 | iR is the first best in iR order (:966-978)
__device__ __forceinline__ uint32_t stereo_take_best(uint32_t best, int dist, int iR) {
  return dist < ORBM_TH_HIGH ? min(best, ((uint32_t)dist << 16) | (uint32_t)iR) : best;
}

// The left window and the sliding range of the right one lie inside the lw x lh level image.  cv::Mat::rowRange / colRange throw
// outside the matrix: such keypoints are skipped (same rule in the test oracle).
__device__ __forceinline__ bool stereo_window_inside(int cuL, int cvL, int cuR, float scaleduR0, int lw, int lh) {
  constexpr int w = STEREO_W, L = STEREO_L;
  const float iniu = scaleduR0 + L - w, endu = scaleduR0 + L + w + 1;
  return cvL - w >= 0 && cvL + w + 1 <= lh && cuL - w >= 0 && cuL + w + 1 <= lw && !(iniu < 0 || endu >= (float)lw) && cuR - L - w >= 0;
}

// SAD argmin over the 2L + 1 offsets, parabola fit, disparity and depth in the reference's fp32 expressions (:1006-1047).  The outputs
// are written only for an accepted match.
__device__ __forceinline__ void stereo_subpixel(const int *sadv, float uL, float scaleduR0, float sfLevel, float minD, float maxD, float mbf,
                                                float *outU, float *outD, int *outSad) {
  constexpr int L = STEREO_L;
  int bestSad = 0x7fffffff, bestincR = 0;
#pragma unroll
  for (int k = 0; k <= 2 * L; k++)
    if ((float)sadv[k] < (float)bestSad) { bestSad = sadv[k]; bestincR = k - L; }       // :1006
  if (bestincR == -L || bestincR == L) return;
  float dist1 = 0.f, dist2 = 0.f, dist3 = 0.f;
#pragma unroll
  for (int k = 1; k < 2 * L; k++)
    if (k == bestincR + L) { dist1 = (float)sadv[k - 1]; dist2 = (float)sadv[k]; dist3 = (float)sadv[k + 1]; }
  const float deltaR = (dist1 - dist3) / (2.0f * (dist1 + dist3 - 2.0f * dist2));      // :1024
  if (deltaR < -1 || deltaR > 1) return;
  float bestuR = sfLevel * ((float)scaleduR0 + (float)bestincR + deltaR);               // :1030
  float disparity = uL - bestuR;
  if (disparity >= minD && disparity < maxD) {
    if (disparity <= 0) { disparity = (float)0.01; bestuR = (float)((double)uL - 0.01); }
    *outD = mbf / disparity;
    *outU = bestuR;
    *outSad = bestSad;
  }
}

struct StereoParams {
  const uint8_t *imgL0, *imgR0; size_t strideL0, strideR0;   // level 0 of the chosen frames
  const uint8_t *pyrL, *pyrR;                                 // pyramid blocks of the chosen frames (levels >= 1)
  int w[ORB_MAXL], h[ORB_MAXL], pitch[ORB_MAXL]; size_t off[ORB_MAXL];
  float sf[ORB_MAXL], invsf[ORB_MAXL];
  int nlevels, rows;
  const float *kpL, *kpR;                                     // 7 floats per keypoint (mvKeys / mvKeysRight)
  const uint32_t *descL, *descR;
  int nL, nR;
  float mb, mbf;
  float *uRight, *depth; int32_t *sad;                        // per left keypoint; sad = -1: no match
};

__global__ __launch_bounds__(256) void k_stereo_match(StereoParams S) {
  const int lane = threadIdx.x & 63;
  const int iL = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (iL >= S.nL) return;
  const float uL = S.kpL[(size_t)iL * 7], vL = S.kpL[(size_t)iL * 7 + 1];
  const int levelL = __float_as_int(S.kpL[(size_t)iL * 7 + 5]);
  float outU = -1.0f, outD = -1.0f;
  int outSad = -1;
  const float minD = 0.f, maxD = S.mbf / S.mb;                // :933-935
  const float minU = uL - maxD, maxU = uL - minD;
  const int row = (int)vL;
  uint32_t best = 0xffffffffu;
  if (row >= 0 && row < S.rows && !(maxU < 0) && levelL >= 0 && levelL < S.nlevels) {
    uint32_t dl[8];
#pragma unroll
    for (int t = 0; t < 8; t++) dl[t] = S.descL[(size_t)iL * 8 + t];
    for (int iR = lane; iR < S.nR; iR += 64) {
      const float uR = S.kpR[(size_t)iR * 7], yR = S.kpR[(size_t)iR * 7 + 1];
      const int oR = __float_as_int(S.kpR[(size_t)iR * 7 + 5]);
      int minr, maxr;
      stereo_row_range(S.sf, ORB_MAXL - 1, yR, oR, &minr, &maxr);
      if (row < minr || row > maxr) continue;
      if (stereo_octave_outside(oR, levelL)) continue;
      if (stereo_u_outside(uR, minU, maxU)) continue;
      int dist = 0;
#pragma unroll
      for (int t = 0; t < 8; t++) dist += __popc(dl[t] ^ S.descR[(size_t)iR * 8 + t]);
      best = stereo_take_best(best, dist, iR);
    }
  }
  best = wave_min_key(best);
  const int thOrbDist = (ORBM_TH_HIGH + ORBM_TH_LOW) / 2;
  if (best != 0xffffffffu && (int)(best >> 16) < thOrbDist) {
    const int bestIdxR = (int)(best & 0xffffu);
    const float uR0 = S.kpR[(size_t)bestIdxR * 7];
    const float scaleFactor = S.invsf[levelL];
    const float scaleduL = roundf(uL * scaleFactor), scaledvL = roundf(vL * scaleFactor), scaleduR0 = roundf(uR0 * scaleFactor);
    constexpr int w = STEREO_W, L = STEREO_L;
    const int lw = S.w[levelL], lh = S.h[levelL];
    const int cuL = (int)scaleduL, cvL = (int)scaledvL, cuR = (int)scaleduR0;
    if (stereo_window_inside(cuL, cvL, cuR, scaleduR0, lw, lh)) {
      const uint8_t *IL, *IR;
      int pL, pR;
      if (levelL == 0) { IL = S.imgL0; IR = S.imgR0; pL = (int)S.strideL0; pR = (int)S.strideR0; }
      else { IL = S.pyrL + S.off[levelL]; IR = S.pyrR + S.off[levelL]; pL = pR = S.pitch[levelL]; }
      const int cL = IL[(size_t)cvL * pL + cuL];
      // my pixels of the 11x11 window: p = lane and lane + 64
      const int p0 = lane, p1 = lane + 64;
      const int y0 = p0 / 11 - w, x0 = p0 % 11 - w, y1 = p1 / 11 - w, x1 = p1 % 11 - w;
      const bool has1 = p1 < 121;
      const int a0 = (int)IL[(size_t)(cvL + y0) * pL + cuL + x0] - cL;
      const int a1 = has1 ? (int)IL[(size_t)(cvL + y1) * pL + cuL + x1] - cL : 0;
      int sadv[2 * L + 1];
#pragma unroll
      for (int k = 0; k <= 2 * L; k++) {
        const int incR = k - L;
        const int cR = IR[(size_t)cvL * pR + cuR + incR];
        const int b0 = (int)IR[(size_t)(cvL + y0) * pR + cuR + incR + x0] - cR;
        const int b1 = has1 ? (int)IR[(size_t)(cvL + y1) * pR + cuR + incR + x1] - cR : 0;
        sadv[k] = wave_sum_i32(abs(a0 - b0) + (has1 ? abs(a1 - b1) : 0));
      }
      stereo_subpixel(sadv, uL, scaleduR0, S.sf[levelL], minD, maxD, S.mbf, &outU, &outD, &outSad);
    }
  }
  if (lane == 0) { S.uRight[iL] = outU; S.depth[iL] = outD; S.sad[iL] = outSad; }
}

__global__ __launch_bounds__(256) void k_stereo_rows(StereoBatchParams S) {
  __shared__ uint32_t sCnt[STEREO_MAX_BANDS];
  __shared__ uint32_t sFill[STEREO_MAX_BANDS];
  __shared__ uint32_t sw[8];
  const int f = blockIdx.x, tid = threadIdx.x;
  const int nR = stereo_live(S.countsR, f, S.cap);
  const float *kp = S.kpR + (size_t)f * S.cap * 7;
  for (int b = tid; b < S.nbands; b += 256) { sCnt[b] = 0; sFill[b] = 0; }
  __syncthreads();
  for (int iR = tid; iR < nR; iR += 256) {
    const float yR = kp[(size_t)iR * 7 + 1];
    const int oR = __float_as_int(kp[(size_t)iR * 7 + 5]);
    int minr, maxr;
    stereo_row_range(S.sf, S.nlevels - 1, yR, oR, &minr, &maxr);
    const int lo = max(minr, 0), hi = min(maxr, S.rows - 1);
    if (lo <= hi)
      for (int b = lo >> STEREO_BAND_SHIFT; b <= (hi >> STEREO_BAND_SHIFT); b++) atomicAdd(&sCnt[b], 1u);
  }
  __syncthreads();
  const uint32_t total = lds_excl_scan<256>(sCnt, S.nbands, sw);
  __syncthreads();
  int32_t *bs = S.bandStart + (size_t)f * (S.nbands + 1);
  for (int b = tid; b < S.nbands; b += 256) bs[b] = (int32_t)min(sCnt[b], (uint32_t)S.recCap);
  if (tid == 0) bs[S.nbands] = (int32_t)min(total, (uint32_t)S.recCap);
  StereoRec *recs = S.recs + (size_t)f * S.recCap;
  for (int iR = tid; iR < nR; iR += 256) {
    const float uR = kp[(size_t)iR * 7], yR = kp[(size_t)iR * 7 + 1];
    const int oR = __float_as_int(kp[(size_t)iR * 7 + 5]);
    int minr, maxr;
    stereo_row_range(S.sf, S.nlevels - 1, yR, oR, &minr, &maxr);
    const int lo = max(minr, 0), hi = min(maxr, S.rows - 1);
    if (lo > hi) continue;
    StereoRec rec;
    rec.u = uR; rec.minr = minr; rec.maxr = maxr; rec.octIdx = ((uint32_t)oR << 16) | (uint32_t)iR;
    for (int b = lo >> STEREO_BAND_SHIFT; b <= (hi >> STEREO_BAND_SHIFT); b++) {
      const uint32_t pos = sCnt[b] + atomicAdd(&sFill[b], 1u);
      if (pos < (uint32_t)S.recCap) recs[pos] = rec;     // (recCap is the host's bound for valid octaves: never reached by extractor output)
    }
  }
}

__global__ __launch_bounds__(256) void k_stereo_search(StereoBatchParams S) {
  __shared__ uint8_t sStrip[4][256];                     // per wavefront: 11 rows x 21 columns of the right level, row-major
  const int f = blockIdx.y;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int nL = stereo_live(S.countsL, f, S.cap);
  const int base = blockIdx.x * STEREO_KPB + wid * STEREO_KPW;
  if (base >= nL) return;                                // wave-uniform: no workgroup barrier below
  const int grp = lane >> 3, sub = lane & 7;
  const int iL = base + grp;
  const bool live = iL < nL;
  const float *kpL = S.kpL + (size_t)f * S.cap * 7, *kpR = S.kpR + (size_t)f * S.cap * 7;
  const uint32_t *descL = S.descL + (size_t)f * S.cap * 8, *descR = S.descR + (size_t)f * S.cap * 8;
  const float uL = live ? kpL[(size_t)iL * 7] : 0.f, vL = live ? kpL[(size_t)iL * 7 + 1] : 0.f;
  const int levelL = live ? __float_as_int(kpL[(size_t)iL * 7 + 5]) : 0;
  const float minD = 0.f, maxD = S.mbf / S.mb;            // :933-935
  const float minU = uL - maxD, maxU = uL - minD;
  const int row = (int)vL;
  uint32_t best = 0xffffffffu;
  if (live && row >= 0 && row < S.rows && !(maxU < 0) && levelL >= 0 && levelL < S.nlevels) {
    uint32_t dl[8];
#pragma unroll
    for (int t = 0; t < 8; t++) dl[t] = descL[(size_t)iL * 8 + t];
    const int32_t *bs = S.bandStart + (size_t)f * (S.nbands + 1) + (row >> STEREO_BAND_SHIFT);
    const int e0 = bs[0], e1 = bs[1];
    const uint4 *recs = (const uint4 *)(S.recs + (size_t)f * S.recCap);
    for (int e = e0 + sub; e < e1; e += 8) {
      const uint4 rc = recs[e];
      if (row < (int)rc.y || row > (int)rc.z) continue;       // the exact row test of the table (:919-920)
      if (stereo_octave_outside((int)rc.w >> 16, levelL)) continue;
      if (stereo_u_outside(__uint_as_float(rc.x), minU, maxU)) continue;
      const int iR = (int)(rc.w & 0xffffu);
      int dist = 0;
#pragma unroll
      for (int t = 0; t < 8; t++) dist += __popc(dl[t] ^ descR[(size_t)iR * 8 + t]);
      best = stereo_take_best(best, dist, iR);
    }
  }
  best = min(best, (uint32_t)__shfl_xor((int)best, 1));
  best = min(best, (uint32_t)__shfl_xor((int)best, 2));
  best = min(best, (uint32_t)__shfl_xor((int)best, 4));
  const int thOrbDist = (ORBM_TH_HIGH + ORBM_TH_LOW) / 2;
  const bool accepted = best != 0xffffffffu && (int)(best >> 16) < thOrbDist;
  float resU = -1.0f, resD = -1.0f;
  int resSad = -1;
  unsigned long long todo = __builtin_amdgcn_ballot_w64(accepted && sub == 0);
  uint8_t *strip = sStrip[wid];
  while (todo) {
    const int src = __builtin_amdgcn_readfirstlane((int)__ffsll((long long)todo) - 1);
    todo &= todo - 1;
    const float quL = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(uL), src));
    const float qvL = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(vL), src));
    const int qlevel = __builtin_amdgcn_readlane(levelL, src);
    const int bestIdxR = (int)((uint32_t)__builtin_amdgcn_readlane((int)best, src) & 0xffffu);
    float outU = -1.0f, outD = -1.0f;
    int outSad = -1;
    const float uR0 = kpR[(size_t)bestIdxR * 7];
    const float scaleFactor = S.invsf[qlevel];
    const float scaleduL = roundf(quL * scaleFactor), scaledvL = roundf(qvL * scaleFactor), scaleduR0 = roundf(uR0 * scaleFactor);
    constexpr int w = STEREO_W, L = STEREO_L;
    const int lw = S.w[qlevel], lh = S.h[qlevel];
    const int cuL = (int)scaleduL, cvL = (int)scaledvL, cuR = (int)scaleduR0;
    if (stereo_window_inside(cuL, cvL, cuR, scaleduR0, lw, lh)) {   // wave-uniform
      const uint8_t *IL, *IR;
      int pL, pR;
      if (qlevel == 0) { IL = S.imgL0 + (size_t)f * S.fsL0; IR = S.imgR0 + (size_t)f * S.fsR0; pL = (int)S.strideL0; pR = (int)S.strideR0; }
      else { IL = S.pyrL + (size_t)f * S.pyrFsL + S.off[qlevel]; IR = S.pyrR + (size_t)f * S.pyrFsR + S.off[qlevel]; pL = pR = S.pitch[qlevel]; }
      // the strip rows cvL-5 .. cvL+5, columns cuR-10 .. cuR+10 (inside the level by the test above): 231 bytes, 4 per lane
      __builtin_amdgcn_wave_barrier();                        // the previous keypoint's reads are done
#pragma unroll
      for (int t = lane; t < 231; t += 64) strip[t] = IR[(size_t)(cvL - w + t / 21) * pR + cuR - L - w + t % 21];
      __builtin_amdgcn_wave_barrier();                        // same-wavefront LDS traffic is ordered
      const int cL = IL[(size_t)cvL * pL + cuL];
      // my pixels of the 11x11 window: p = lane and lane + 64
      const int p0 = lane, p1 = lane + 64;
      const int y0 = p0 / 11, x0 = p0 % 11, y1 = p1 / 11, x1 = p1 % 11;
      const bool has1 = p1 < 121;
      const int a0 = (int)IL[(size_t)(cvL + y0 - w) * pL + cuL + x0 - w] - cL;
      const int a1 = has1 ? (int)IL[(size_t)(cvL + y1 - w) * pL + cuL + x1 - w] - cL : 0;
      const uint8_t *s0 = strip + y0 * 21 + x0, *s1 = strip + (has1 ? y1 * 21 + x1 : 0), *sc = strip + w * 21 + w;
      int part[2 * L + 1];
#pragma unroll
      for (int k = 0; k <= 2 * L; k++) {
        const int cR = sc[k];
        const int b0 = (int)s0[k] - cR;
        const int b1 = (int)s1[k] - cR;
        part[k] = abs(a0 - b0) + (has1 ? abs(a1 - b1) : 0);
      }
      // a SAD is at most 121 * 510 < 2^16: two of them share one register through the reduction
      int sadv[2 * L + 2];
#pragma unroll
      for (int k = 0; k <= 2 * L; k += 2) {
        const int packed = wave_sum_i32(part[k] | (k + 1 <= 2 * L ? part[k + 1] << 16 : 0));
        sadv[k] = packed & 0xffff;
        sadv[k + 1] = (int)((uint32_t)packed >> 16);
      }
      stereo_subpixel(sadv, quL, scaleduR0, S.sf[qlevel], minD, maxD, S.mbf, &outU, &outD, &outSad);
    }
    if (lane == src) { resU = outU; resD = outD; resSad = outSad; }
  }
  if (live && sub == 0) {
    const size_t o = (size_t)f * S.cap + iL;
    S.uRight[o] = resU; S.depth[o] = resD; S.sad[o] = resSad;
  }
}

// Wavefront 0: the bin of `hist` (256 bins) that holds rank `rank` and the rank inside it.  All 64 lanes active.
__device__ __forceinline__ void stereo_select(const uint32_t *hist, int rank, int *sel) {
  const int lane = threadIdx.x;
  uint32_t c[4];
#pragma unroll
  for (int j = 0; j < 4; j++) c[j] = hist[4 * lane + j];
  const uint32_t s = c[0] + c[1] + c[2] + c[3];
  const uint32_t incl = wave_incl_scan(s);
  uint32_t below = incl - s;
  if ((uint32_t)rank >= below && (uint32_t)rank < incl) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if ((uint32_t)rank < below + c[j]) { sel[0] = 4 * lane + j; sel[1] = rank - (int)below; break; }
      below += c[j];
    }
  }
}

__global__ __launch_bounds__(256) void k_stereo_median(StereoBatchParams S) {
  __shared__ uint32_t sHist[256];
  __shared__ int sSel[2];
  __shared__ uint32_t sKept;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int nL = stereo_live(S.countsL, f, S.cap);
  const int32_t *sad = S.sad + (size_t)f * S.cap;
  float *uRight = S.uRight + (size_t)f * S.cap, *depth = S.depth + (size_t)f * S.cap;
  sHist[tid] = 0;
  if (tid == 0) { sKept = 0; sSel[0] = 0; sSel[1] = 0; }
  __syncthreads();
  for (int i = tid; i < nL; i += 256) {
    const int s = sad[i];
    if (s >= 0) atomicAdd(&sHist[(s >> 8) & 255], 1u);
  }
  __syncthreads();
  // nDI: every thread sums the same 256 counters of its wavefront's view (4 per lane, wave sum)
  const int lane = tid & 63;
  const int nDI = wave_sum_i32((int)(sHist[4 * lane] + sHist[4 * lane + 1] + sHist[4 * lane + 2] + sHist[4 * lane + 3]));
  if (nDI == 0) {                                         // an empty set: nothing to do (the oracle's and the host form's rule)
    if (tid == 0 && S.nstereo) S.nstereo[f] = 0;
    return;
  }
  if (tid < 64) stereo_select(sHist, nDI / 2, sSel);      // :1066
  __syncthreads();
  const int hiBin = sSel[0], rank2 = sSel[1];
  __syncthreads();
  sHist[tid] = 0;
  __syncthreads();
  for (int i = tid; i < nL; i += 256) {
    const int s = sad[i];
    if (s >= 0 && ((s >> 8) & 255) == hiBin) atomicAdd(&sHist[s & 255], 1u);
  }
  __syncthreads();
  if (tid < 64) stereo_select(sHist, rank2, sSel);
  __syncthreads();
  const float median = (float)((hiBin << 8) | sSel[0]);
  const float thDist = 1.5f * 1.4f * median;              // :1067
  uint32_t kept = 0;
  for (int i = tid; i < nL; i += 256) {
    const int s = sad[i];
    if (s < 0) continue;
    if ((float)s >= thDist) { uRight[i] = -1; depth[i] = -1; }   // :1069-1077: the descending loop stops at the first sad < thDist
    else kept++;
  }
  if (S.nstereo) {
    if (kept) atomicAdd(&sKept, kept);
    __syncthreads();
    if (tid == 0) S.nstereo[f] = (int32_t)sKept;
  }
}
