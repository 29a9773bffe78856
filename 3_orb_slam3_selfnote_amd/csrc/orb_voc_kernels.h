// orb_voc_kernels.h -- Frame::ComputeBoW / KeyFrame::ComputeBoW on the device: the statement of orb_ref_voc.h for `nframes` frames
// per launch.  Included by orbhip.hip after orb_common.h (LiveCount).
//   k_voc_descend  the descent of every descriptor: terminal entry, word id and the node at level m_L - levelsup
//   k_voc_collect  one workgroup per frame: FeatureVector as the CSR orbm_keyframe_t reads, BowVector as ascending (id, value) pairs
#pragma once
#include "orb_ref_voc.h"
#include "orb_sort.h"

// ---- descent -----------------------------------------------------------------------------------------------------------------------

struct VocDescendParams {
  const uint32_t *desc; const VocRec *rec;       // the re-laid tree
  const uint8_t *q;                              // [nframes][cap][32], 16-byte aligned
  LiveCount n; int cap;
  int nid_level;                                 // m_L - levelsup
  int32_t *entry; uint32_t *word, *node;         // [nframes][cap]
};

// the smallest key of a 16-lane row, in every lane of the row: two quad permutes, row_half_mirror, row_mirror.  Every source lane is
// in the reader's own row, and a row is wholly active or wholly inactive here, so no lane reads a disabled one.
__device__ __forceinline__ uint32_t voc_row_min(uint32_t v) {
  uint32_t t;
  t = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xb1, 0xf, 0xf, false); v = t < v ? t : v;    // quad_perm [1,0,3,2]
  t = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4e, 0xf, 0xf, false); v = t < v ? t : v;    // quad_perm [2,3,0,1]
  t = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xf, 0xf, false); v = t < v ? t : v;   // row_half_mirror
  t = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xf, 0xf, false); v = t < v ? t : v;   // row_mirror
  return v;
}

// One 16-lane row per descriptor, four descriptors per wavefront, sixteen per workgroup.  The query's eight dwords stay in registers;
// lane r of the row takes child base + r of the current node: two 16-byte loads, xor, popcount, key = voc_key(distance, r).  The row's
// smallest key is the first minimum among those sixteen, and voc_take holds it against the rounds before (children beyond sixteen: the
// table decides the count, not k).  No LDS: below the levels that fit the caches every level is a dependent miss, so the kernel lives
// on the number of rows in flight.
__global__ __launch_bounds__(256) void k_voc_descend(VocDescendParams P) {
  const int p = blockIdx.y, r = threadIdx.x & 15;
  const int n = P.n.at(p, P.cap);
  const int i = blockIdx.x * 16 + (threadIdx.x >> 4);
  if (i >= n) return;
  const size_t at = (size_t)p * P.cap + i;
  const uint4 *qp = reinterpret_cast<const uint4 *>(P.q + at * 32);
  const uint4 qa = qp[0], qb = qp[1];
  const uint32_t q[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
  int cur = 0, level = 0;
  uint32_t node = 0;
  VocRec rec = P.rec[0];
  while (rec.count > 0) {
    ++level;
    uint32_t best_d = VOC_NO_CHILD;
    int best_pos = 0;
    for (int base = 0; base < rec.count; base += 16) {
      uint32_t key = VOC_NO_CHILD;
      if (base + r < rec.count) {
        const uint4 *cp = reinterpret_cast<const uint4 *>(P.desc + 8 * (size_t)(rec.first + base + r));
        const uint4 ca = cp[0], cb = cp[1];
        const uint32_t c[8] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
        key = voc_key(voc_distance(q, c), r);
      }
      voc_take(voc_row_min(key), base, &best_d, &best_pos);
    }
    cur = rec.first + best_pos;
    rec = P.rec[cur];
    if (level == P.nid_level) node = rec.node;
  }
  if (r == 0) {
    P.entry[at] = cur;
    P.word[at] = rec.word;
    P.node[at] = node;
  }
}

// The alternative measured beside it (tools/bow_transform_bench.py): one lane per descriptor, voc_descend as it is.
__global__ __launch_bounds__(256) void k_voc_descend_lane(VocDescendParams P) {
  const int p = blockIdx.y;
  const int n = P.n.at(p, P.cap);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t at = (size_t)p * P.cap + i;
  const uint4 *qp = reinterpret_cast<const uint4 *>(P.q + at * 32);
  const uint4 qa = qp[0], qb = qp[1];
  const uint32_t q[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
  int32_t entry; uint32_t node;
  voc_descend(P.desc, P.rec, q, P.nid_level, &entry, &node);
  P.entry[at] = entry;
  P.word[at] = P.rec[entry].word;
  P.node[at] = node;
}

// ---- assembly ----------------------------------------------------------------------------------------------------------------------

#define VOC_THREADS 1024

struct VocCollectParams {
  const VocRec *rec; const double *weight;
  LiveCount n; int cap;
  int weighting, scoring;
  const int32_t *entry; const uint32_t *node;    // [nframes][cap] from k_voc_descend
  uint32_t *bow_id; double *bow_val; int32_t *n_bow;          // [nframes][cap], [nframes]
  uint32_t *fv_node_id; int32_t *fv_start, *fv_idx, *n_fv;    // [nframes][cap], [nframes][cap + 1], [nframes][cap], [nframes]
};

// exclusive prefix sum of one int per lane over the workgroup; *total = the sum.  s_scan has VOC_THREADS ints.
__device__ __forceinline__ int voc_block_scan(int v, int *s_scan, int tid, int *total) {
  s_scan[tid] = v;
  __syncthreads();
  for (int d = 1; d < VOC_THREADS; d <<= 1) {
    const int t = tid >= d ? s_scan[tid - d] : 0;
    __syncthreads();
    s_scan[tid] += t;
    __syncthreads();
  }
  const int incl = s_scan[tid];
  *total = s_scan[VOC_THREADS - 1];
  __syncthreads();
  return incl - v;
}

// The two std::maps are fixed by their keys' order and, per key, by ascending feature order; sorting the unique keys
// (node << 32 | i) and (word << 32 | i) gives both at once.  Stopped features (w > 0 fails, :1157 / :1185) get the padding key.
// Per word the value is built by ONE lane, feature after feature (voc_add), since k sequential adds of w are not k * w; the L1 sum
// is walked by ONE lane in ascending word order (voc_l1_step), since its order is part of the result; then all lanes divide.
__global__ __launch_bounds__(VOC_THREADS) void k_voc_collect(VocCollectParams P) {
  extern __shared__ __align__(16) uint8_t smem_vkey[];
  uint64_t *s_vkey = SortCarve::of(P.cap).keys.in(smem_vkey);   // afterwards the values as doubles
  __shared__ int s_scan[VOC_THREADS];
  __shared__ int s_live;
  __shared__ double s_norm;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n = P.n.at(p, P.cap);
  const size_t at = (size_t)p * P.cap;
  const int32_t *entry = P.entry + at;
  const uint32_t *node = P.node + at;
  const int p2 = sort_p2(n);
  const int per = p2 > VOC_THREADS ? p2 / VOC_THREADS : 1;   // consecutive sorted positions per lane
  const bool adds = voc_adds_weight(P.weighting);

  // FeatureVector (FeatureVector.cpp:31-45)
  if (tid == 0) s_live = 0;
  __syncthreads();
  int mine = 0;
  for (int i = tid; i < p2; i += VOC_THREADS) {
    uint64_t key = ~0ull;
    if (i < n && P.weight[entry[i]] > 0) { key = ((uint64_t)node[i] << 32) | (uint32_t)i; mine++; }
    s_vkey[i] = key;
  }
  if (mine) atomicAdd(&s_live, mine);
  __syncthreads();
  const int m = s_live;   // features that enter the containers
  bitonic_sort_lds<VOC_THREADS>(s_vkey, p2, tid);
  const int lo = min(tid * per, m), hi = min(lo + per, m);
  {
    int starts = 0;
    for (int t = lo; t < hi; t++) starts += t == 0 || (uint32_t)(s_vkey[t] >> 32) != (uint32_t)(s_vkey[t - 1] >> 32);
    int total;
    int rank = voc_block_scan(starts, s_scan, tid, &total);
    uint32_t *fv_node_id = P.fv_node_id + at;
    int32_t *fv_start = P.fv_start + (size_t)p * (P.cap + 1), *fv_idx = P.fv_idx + at;
    for (int t = lo; t < hi; t++) {
      const uint64_t key = s_vkey[t];
      fv_idx[t] = (int32_t)(uint32_t)key;
      if (t == 0 || (uint32_t)(key >> 32) != (uint32_t)(s_vkey[t - 1] >> 32)) { fv_node_id[rank] = (uint32_t)(key >> 32); fv_start[rank] = t; rank++; }
    }
    if (tid == 0) { fv_start[total] = m; P.n_fv[p] = total; }
  }
  __syncthreads();

  // BowVector (BowVector.cpp:34-58)
  for (int i = tid; i < p2; i += VOC_THREADS) {
    uint64_t key = ~0ull;
    if (i < n) {
      const int e = entry[i];
      if (P.weight[e] > 0) key = ((uint64_t)P.rec[e].word << 32) | (uint32_t)i;
    }
    s_vkey[i] = key;
  }
  __syncthreads();
  bitonic_sort_lds<VOC_THREADS>(s_vkey, p2, tid);
  int starts = 0;
  for (int t = lo; t < hi; t++) starts += t == 0 || (uint32_t)(s_vkey[t] >> 32) != (uint32_t)(s_vkey[t - 1] >> 32);
  int nb;
  int rank = voc_block_scan(starts, s_scan, tid, &nb);
  uint32_t *bow_id = P.bow_id + at;
  double *bow_val = P.bow_val + at;
  for (int t = lo; t < hi; t++) {
    const uint32_t word = (uint32_t)(s_vkey[t] >> 32);
    if (t != 0 && word == (uint32_t)(s_vkey[t - 1] >> 32)) continue;
    double second = 0.0;
    for (int u = t; u < m; u++) {                 // the features of this word in ascending order
      const uint64_t key = s_vkey[u];
      if ((uint32_t)(key >> 32) != word) break;
      voc_add(&second, P.weight[entry[(uint32_t)key]], u == t, adds);
      if (!adds) break;                           // addIfNotExist: the later features change nothing
    }
    bow_id[rank] = word;
    bow_val[rank] = second;
    rank++;
  }
  if (tid == 0) P.n_bow[p] = nb;
  const bool must = voc_must_normalize(P.scoring);
  if (!must && !adds) return;                     // IDF / BINARY under DOT_PRODUCT: the values stay
  __syncthreads();                                // the keys are dead, this workgroup's stores to bow_val are visible to it
  double *s_val = reinterpret_cast<double *>(s_vkey);
  for (int t = tid; t < nb; t += VOC_THREADS) s_val[t] = bow_val[t];
  __syncthreads();
  if (tid == 0) {
    double norm = 0.0;
    if (must) for (int t = 0; t < nb; t++) voc_l1_step(&norm, s_val[t]);
    else norm = (double)nb;                       // :1167
    s_norm = norm;
  }
  __syncthreads();
  const double by = s_norm;
  if (must && !(by > 0.0)) return;                // BowVector.cpp:79
  for (int t = tid; t < nb; t += VOC_THREADS) bow_val[t] = voc_div(s_val[t], by);
}
