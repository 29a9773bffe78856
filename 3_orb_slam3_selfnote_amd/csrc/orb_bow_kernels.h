// orb_bow_kernels.h -- ORBmatcher::SearchByBoW of ONE frame or keyframe against ALL candidates of a call: the loops of
// Tracking::Relocalization (Tracking.cc:3796-3816, K candidate keyframes against the current frame) and of
// LoopClosing::DetectCommonRegionsFromBoW (LoopClosing.cc:724-739, the current keyframe against a candidate and its covisibles).
//
// k_bow_match_candidates has the semantics of k_bow_match (orb_match_kernels.h) line for line - the walk order of the node's first-operand
// keypoints, best / second as two wave minima of (dist << 16 | position) with strict `<`, the `taken` bits, `strict` / hasmp of the
// keyframe form, the right-image branch of a fisheye-stereo frame - over the (candidate, shared node) items of every candidate at once:
// one wavefront per item, four items per workgroup, no LDS, no barrier.  What differs between candidates - where their arrays lie in
// the call's staged block, Frame::Nleft - stands in a table in device memory, one BowCand per candidate (TriNb's arrangement).
// Two things differ from k_bow_match:
//   - the node's first 64 second-operand members are each lane's own: index, map-point flag and the eight descriptor words are loaded
//     once per item and stay in registers across the walk (k_bow_match reads them again for every walked keypoint); positions >= 64
//     keep reading memory;
//   - the walked keypoint - index, map-point flag, descriptor - is the same in every lane: it is fetched through the scalar data cache
//     into scalar registers, and keypoint k + 1's descriptor and flag (and keypoint k + 2's index) are in flight while k is reduced.
//     Those arrays are written by the host alone, never by a kernel, so the constant address space is theirs.
// k_bow_prune_candidates then does per candidate what RotHist does on the host for the per-pair entries: histogram of the rotation
// between the matched keypoints (rot_bin), ComputeThreeMaxima (three_maxima), the pruning, and the count.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "orb_common.h"
#include "orb_ref_geometry.h"
#include "orb_match_kernels.h"

// One work item: vocabulary node shared by candidate `cand`'s pair.  W = the operand whose keypoints are walked (the keyframe of
// SearchByBoW(pKF, F), pKF1 of SearchByBoW(pKF1, pKF2)), S = the second operand, whose keypoints are taken.  32 bytes: one scalar load.
struct BowCandItem { int32_t cand, startW, lenW, startS, lenS, pad_[3]; };

// One candidate: byte offsets of its pair's arrays in the staged block (the base moves when the block grows, the offsets do not).
// The fixed operand's offsets are the same in every record.  hasmpS = BOW_NO_HASMP: every keypoint of S may be taken (the frame form).
#define BOW_NO_HASMP (~(unsigned long long)0)
struct BowCand {
  unsigned long long descW, hasmpW, node_idxW, descS;   // words 0..7
  unsigned long long hasmpS, node_idxS;                 // words 8..11
  unsigned long long angW, angS;                        // words 12..15: keypoint angles [n] (k_bow_prune_candidates, checkOri only)
  int32_t n_left;                                       // word 16: Frame::Nleft of S, 0x7fffffff when it has no right image
  int32_t pad_[3];
};

struct BowCandParams {
  const uint8_t *block;            // the staged block
  const BowCand *cands;            // [K]; a candidate without work has an all-zero record and an all -1 row
  const BowCandItem *items; int nitems;
  int nout;                        // row length: S's keypoints (frame form), W's keypoints (keyframe form)
  float nnratio;
  int kf_kf;                       // SearchByBoW(KeyFrame*, KeyFrame*): strict threshold (:923), rows indexed by W's keypoint (:927)
  int checkOri;
  int32_t *rows;                   // [K][nout], pre-filled with -1
  int32_t *nmatches;               // [K]
};

// 0: the kernel described above.  1, for measurements only: k_bow_match's own body over the same flat item list - nothing
// lane-held, the walked keypoint through ordinary loads - to tell what the two changes are worth apart from the fuller grid.
#ifndef BOW_CAND_BODY
#define BOW_CAND_BODY 0
#endif

typedef uint32_t bow_u8_t __attribute__((ext_vector_type(8)));
typedef uint32_t bow_u4_t __attribute__((ext_vector_type(4)));
// A wave-uniform read of host-written memory: through the constant address space it is a scalar load wherever it stands
template <class V> __device__ __forceinline__ V bow_uniform_load(const void *p) {
  return *reinterpret_cast<const __attribute__((address_space(4))) V *>((const __attribute__((address_space(4))) void *)p);
}
__device__ __forceinline__ unsigned long long bow_u64(uint32_t lo, uint32_t hi) { return ((unsigned long long)hi << 32) | lo; }

__device__ __forceinline__ void bow_best2(uint32_t key, bool left, uint32_t &b1, uint32_t &b2, uint32_t &r1) {
  if (left) {                                                        // :326-335 resp. :347-354
    if (key < b1) { b2 = b1; b1 = key; }
    else if (key < b2) b2 = key;
  } else {
    r1 = key < r1 ? key : r1;                                        // :356-363 (the right second-best is never used, :407)
  }
}

__global__ __launch_bounds__(256) void k_bow_match_candidates(BowCandParams B) {
  const int lane = threadIdx.x & 63;
  const int it = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (it >= B.nitems) return;
  const bow_u8_t I = bow_uniform_load<bow_u8_t>(B.items + it);
  const int cand = (int)I[0], startW = (int)I[1], lenW = (int)I[2], startS = (int)I[3], lenS = (int)I[4];
  const uint8_t *rec = (const uint8_t *)(B.cands + cand);
  const bow_u8_t r0 = bow_uniform_load<bow_u8_t>(rec);
  const bow_u4_t r1_ = bow_uniform_load<bow_u4_t>(rec + 32);
  const int nleftS = (int)bow_uniform_load<uint32_t>(rec + 64);
  const uint32_t *descW = (const uint32_t *)(B.block + bow_u64(r0[0], r0[1]));
  const uint8_t *hasmpW = B.block + bow_u64(r0[2], r0[3]);
  const int32_t *node_idxW = (const int32_t *)(B.block + bow_u64(r0[4], r0[5])) + startW;
  const uint32_t *descS = (const uint32_t *)(B.block + bow_u64(r0[6], r0[7]));
  const unsigned long long hasmpS_off = bow_u64(r1_[0], r1_[1]);
  const uint8_t *hasmpS = hasmpS_off == BOW_NO_HASMP ? nullptr : B.block + hasmpS_off;   // :896-903
  const int32_t *node_idxS = (const int32_t *)(B.block + bow_u64(r1_[2], r1_[3])) + startS;
  int32_t *row = B.rows + (size_t)cand * (size_t)B.nout;
  const bool stereoS = nleftS != 0x7fffffff;
  const int nt = (lenS + 63) >> 6;          // <= 32 (larger nodes are refused on the host)

  // the lane's own member of the node (position = lane): loaded once, held across the walk
  const bool own = lane < lenS;
  const int idxS0 = own ? node_idxS[lane] : 0;
  bool ok0 = own && BOW_CAND_BODY == 0;
  if (ok0 && hasmpS) ok0 = hasmpS[idxS0] != 0;
  uint4 sa = make_uint4(0, 0, 0, 0), sb = sa;
  if (ok0) {
    const uint4 *p = reinterpret_cast<const uint4 *>(descS + (size_t)idxS0 * 8);
    sa = p[0]; sb = p[1];
  }
  const bool left0 = idxS0 < nleftS;

#if BOW_CAND_BODY == 1
  uint32_t taken = 0;
  for (int k = 0; k < lenW; k++) {
    const int idxW = node_idxW[k];
    const uint32_t has = hasmpW[idxW];
    const uint32_t *pw = descW + (size_t)idxW * 8;
    const uint32_t d0 = pw[0], d1 = pw[1], d2 = pw[2], d3 = pw[3], d4 = pw[4], d5 = pw[5], d6 = pw[6], d7 = pw[7];
#else
  // the walked keypoint through the scalar path, two stages ahead: index of k + 2, flag and descriptor of k + 1
  auto walk_idx = [&](int k) { return (int)bow_uniform_load<uint32_t>(node_idxW + k); };
  auto walk_has = [&](int idx) { return bow_uniform_load<uint32_t>(hasmpW + (idx & ~3)); };   // the word that holds the flag: shifted where it is used
  auto walk_desc = [&](int idx) { return bow_uniform_load<bow_u8_t>(descW + (size_t)idx * 8); };
  int idxN = walk_idx(0);
  int idxNN = lenW > 1 ? walk_idx(1) : 0;
  bow_u8_t dN = walk_desc(idxN);
  uint32_t hasN = walk_has(idxN);
  uint32_t taken = 0;
  for (int k = 0; k < lenW; k++) {
    int idxW = idxN;
    uint32_t has = (hasN >> (8 * (idxW & 3))) & 0xffu, d0 = dN[0], d1 = dN[1], d2 = dN[2], d3 = dN[3], d4 = dN[4], d5 = dN[5], d6 = dN[6], d7 = dN[7];
    // keypoint k's values are complete here, in front of the loads for k + 1: nothing below waits for those
    asm volatile("" : "+s"(idxW), "+s"(has), "+s"(d0), "+s"(d1), "+s"(d2), "+s"(d3), "+s"(d4), "+s"(d5), "+s"(d6), "+s"(d7));
    idxN = idxNN;
    if (k + 1 < lenW) { dN = walk_desc(idxN); hasN = walk_has(idxN); }
    if (k + 2 < lenW) idxNN = walk_idx(k + 2);
#endif
    if (!has) continue;                                              // :307-313
    uint32_t b1 = 0xffffffffu, b2 = 0xffffffffu, r1 = 0xffffffffu;
    if (ok0 && !(taken & 1u)) {                                      // :321, position = lane
      const int dist = __popc(d0 ^ sa.x) + __popc(d1 ^ sa.y) + __popc(d2 ^ sa.z) + __popc(d3 ^ sa.w) + __popc(d4 ^ sb.x) +
                       __popc(d5 ^ sb.y) + __popc(d6 ^ sb.z) + __popc(d7 ^ sb.w);
      bow_best2(((uint32_t)dist << 16) | (uint32_t)lane, left0, b1, b2, r1);
    }
    for (int t = BOW_CAND_BODY == 1 ? 0 : 1; t < nt; t++) {
      const int pos = lane + 64 * t;
      if (pos < lenS && !((taken >> t) & 1u)) {                      // :321
        const int idxS = node_idxS[pos];
        if (hasmpS && !hasmpS[idxS]) continue;                       // :896-903
        const uint4 *p = reinterpret_cast<const uint4 *>(descS + (size_t)idxS * 8);
        const uint4 a = p[0], b = p[1];
        const int dist = __popc(d0 ^ a.x) + __popc(d1 ^ a.y) + __popc(d2 ^ a.z) + __popc(d3 ^ a.w) + __popc(d4 ^ b.x) + __popc(d5 ^ b.y) +
                         __popc(d6 ^ b.z) + __popc(d7 ^ b.w);
        bow_best2(((uint32_t)dist << 16) | (uint32_t)pos, idxS < nleftS, b1, b2, r1);
      }
    }
    const uint32_t g1 = wave_min_key(b1);
    const uint32_t g2 = wave_min_key(b1 == g1 ? b2 : b1);
    const int bestDist1 = g1 != 0xffffffffu ? (int)(g1 >> 16) : 256, bestDist2 = g2 != 0xffffffffu ? (int)(g2 >> 16) : 256;
    const bool within = B.kf_kf ? bestDist1 < ORBM_TH_LOW : bestDist1 <= ORBM_TH_LOW;
    if (within && (float)bestDist1 < B.nnratio * (float)bestDist2) {   // :385-387
      const int pos = (int)(g1 & 0xffffu);
      if (lane == (pos & 63)) {
        taken |= 1u << (pos >> 6);
        const int idxS = BOW_CAND_BODY == 0 && pos < 64 ? idxS0 : node_idxS[pos];
        if (B.kf_kf) row[idxW] = idxS;                                 // :927
        else row[idxS] = idxW;                                         // :389
      }
    }
    if (stereoS && within) {                                           // :405-436, inside `if(bestDist1<=TH_LOW)`
      const uint32_t gr = wave_min_key(r1);
      if (gr != 0xffffffffu && (int)(gr >> 16) <= ORBM_TH_LOW) {
        const int pos = (int)(gr & 0xffffu);
        if (lane == (pos & 63)) {
          taken |= 1u << (pos >> 6);
          row[BOW_CAND_BODY == 0 && pos < 64 ? idxS0 : node_idxS[pos]] = idxW;   // :409
        }
      }
    }
  }
}

// The rotation-consistency check of both members on the device (:391-404, :451-466 resp. :929-939, :960-975), one workgroup per
// candidate: the bins only need their sizes (integer LDS atomics, as k_rot_prune); a match whose bin lies outside the histogram is in
// no bin and is never pruned (RotHist::add).  Writes the pruned row and nmatches[j]; with checkOri == 0 it only counts.
__global__ __launch_bounds__(256) void k_bow_prune_candidates(BowCandParams B) {
  __shared__ int hist[32];
  __shared__ int keep[3];
  __shared__ int count;
  const int j = blockIdx.x, t = threadIdx.x;
  int32_t *row = B.rows + (size_t)j * (size_t)B.nout;
  if (t < 32) hist[t] = 0;
  if (t == 0) count = 0;
  __syncthreads();
  int mine = 0;
  if (B.checkOri) {
    const BowCand &C = B.cands[j];
    const float *angW = (const float *)(B.block + C.angW), *angS = (const float *)(B.block + C.angS);
    auto bin_of = [&](int i, int v) { return B.kf_kf ? rot_bin(angW[i] - angS[v]) : rot_bin(angW[v] - angS[i]); };
    for (int i = t; i < B.nout; i += 256) {
      const int v = row[i];
      if (v < 0) continue;
      const int bin = bin_of(i, v);
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
    for (int i = t; i < B.nout; i += 256) {
      const int v = row[i];
      if (v < 0) continue;
      const int bin = bin_of(i, v);
      if (bin < 0 || bin >= ORBM_HISTO_LENGTH || bin == k0 || bin == k1 || bin == k2) mine++;
      else row[i] = -1;
    }
  } else {
    for (int i = t; i < B.nout; i += 256) mine += row[i] >= 0 ? 1 : 0;
  }
  if (mine) atomicAdd(&count, mine);
  __syncthreads();
  if (t == 0) B.nmatches[j] = count;
}
