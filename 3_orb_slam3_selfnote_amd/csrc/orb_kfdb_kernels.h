// orb_kfdb_kernels.h -- the heavy part of KeyFrameDatabase::DetectRelocalizationCandidates (KeyFrameDatabase.cc:816-871) and
// KeyFrameDatabase::DetectNBestCandidates (KeyFrameDatabase.cc:627-711) for gfx950: common-word counts per keyframe, the 0.8f gate,
// L1Scoring::score (ScoringObject.cpp:23-68) of every keyframe that passes, and the list in the reference's order.  Every expression
// comes from orb_ref_kfdb.h; the kernels only decide which lane evaluates it and in which order the results meet.
//
// The database is a CSR over "slots" in add order (erased slots are tombstones): ids[off .. off + n) ascending, val[] the doubles.
// One launch sequence serves `nq` queries (gridDim.y, or one block per query): the single-query entries run it with nq = 1.
//   k_kfdb_mark    sets the query's words in a bitmap over the vocabulary (n_words bits per query) and zeroes the query's header
//   k_kfdb_count   one wavefront per (slot, query): 64 keyframe words per step, membership from the bitmap, the ballot's popcount is
//                  the step's common-word count, the first hit of the first step that has one is the smallest shared word (ids ascend);
//                  atomicMax gives maxCommonWords over the listable slots (an integer maximum: no order in it)
//   k_kfdb_order   one workgroup per query: sorts the unique keys kfdb_order_key(first shared word, slot) of the listed slots
//                  (ORDER RULE), applies the gate in that order and writes the passing slots, compacted, in list order
//   k_kfdb_score   one wavefront per passing keyframe: per step each hit lane finds the query's value by a binary search in the
//                  query's ascending ids and forms the term; the terms are then added to the wave's running double in ASCENDING LANE
//                  order, one kfdb_l1_add per hit, by walking the ballot - a lane without a hit adds nothing, so the sum is the
//                  reference's sequence of `+=` and no other
//   k_kfdb_unmark  clears the bitmap by walking the query again (the single-query entries; the batch entry gets a fresh bitmap)
// No kernel stores through a pointer it did not bound: slot indices are < n_slots, word indices < off + n (the host keeps
// off + n <= pool size), bitmap words are addressed only for ids < n_words, outputs are [nq][n_slots].
#pragma once
#include <stdint.h>
#include "orb_ref_kfdb.h"
#include "orb_sort.h"

struct alignas(16) KfdbSlot {   // 32 bytes
  uint32_t off;      // first word of the keyframe in ids[] / val[]
  int32_t n;         // its words; -1 = erased
  uint64_t tag;      // the caller's name
  uint64_t rq;       // mnRelocQuery as the handle holds it (read by the batch form only)
  uint32_t seq_pad[2];
};

#define KFDB_HDR 4   // ints per query: maxCommonWords, minCommonWords, keyframes scored (= listed in lScoreAndMatch), keyframes in lKFsSharingWords
#define KFDB_H_MAX 0
#define KFDB_H_MIN 1
#define KFDB_H_SCORED 2
#define KFDB_H_LISTED 3

struct KfdbParams {
  const KfdbSlot *slot; int n_slots;
  const uint32_t *ids; const double *val;     // the pool
  int n_words; int bm_stride;                 // bitmap: bm_stride dwords per query
  uint32_t *bitmap;
  const uint32_t *q_id; const double *q_val;  // [nq][cap]
  const int32_t *q_n; int cap;                // live words of query q: min(max(q_n[q], 0), cap)
  const uint8_t *listable;                    // [n_slots] single-query form: stored query id differs, not connected; NULL = batch form
  const uint64_t *query_id;                   // [nq] batch form: listable = alive && slot.rq != query_id[q]
  int32_t *hdr;                               // [nq][KFDB_HDR]
  int32_t *cnt; uint32_t *first;              // [nq][n_slots]
  int32_t *out_slot; float *out_score;        // [nq][out_stride] compact, list order
  uint64_t *out_tag;                          // [nq][out_stride] or NULL
  int out_stride;
};

__device__ __forceinline__ int kfdb_qn(const KfdbParams &P, int q) { return min(max(P.q_n[q], 0), P.cap); }

__global__ __launch_bounds__(256) void k_kfdb_mark(KfdbParams P) {
  const int q = blockIdx.y, n = kfdb_qn(P, q);
  const uint32_t *qid = P.q_id + (size_t)q * P.cap;
  uint32_t *bm = P.bitmap + (size_t)q * P.bm_stride;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < KFDB_HDR) P.hdr[q * KFDB_HDR + i] = 0;
  if (i < n) {
    const uint32_t w = qid[i];
    if (w < (uint32_t)P.n_words) atomicOr(&bm[w >> 5], 1u << (w & 31));
  }
}

__global__ __launch_bounds__(256) void k_kfdb_unmark(KfdbParams P) {
  const int q = blockIdx.y, n = kfdb_qn(P, q);
  const uint32_t *qid = P.q_id + (size_t)q * P.cap;
  uint32_t *bm = P.bitmap + (size_t)q * P.bm_stride;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const uint32_t w = qid[i];
    if (w < (uint32_t)P.n_words) bm[w >> 5] = 0;   // every lane that shares the dword stores the same 0
  }
}

__device__ __forceinline__ bool kfdb_listable(const KfdbParams &P, int q, int s, const KfdbSlot &sl) {
  if (sl.n < 0) return false;
  return P.listable ? P.listable[s] != 0 : sl.rq != P.query_id[q];
}

__global__ __launch_bounds__(256) void k_kfdb_count(KfdbParams P) {
  const int q = blockIdx.y, lane = threadIdx.x & 63;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);   // wave-uniform
  if (s >= P.n_slots) return;
  const KfdbSlot sl = P.slot[s];
  const size_t at = (size_t)q * P.n_slots + s;
  int words = 0;
  uint32_t first = 0xffffffffu;
  if (kfdb_listable(P, q, s, sl)) {
    const uint32_t *bm = P.bitmap + (size_t)q * P.bm_stride;
    const uint32_t *ids = P.ids + sl.off;
    for (int c = 0; c < sl.n; c += 64) {
      const int i = c + lane;
      uint32_t w = 0;
      bool hit = false;
      if (i < sl.n) {
        w = ids[i];
        hit = w < (uint32_t)P.n_words && ((bm[w >> 5] >> (w & 31)) & 1u);
      }
      const unsigned long long b = __ballot(hit);
      if (b) {
        if (words == 0) first = (uint32_t)__shfl((int)w, __ffsll((long long)b) - 1);
        words += __popcll(b);
      }
    }
  }
  if (lane == 0) {
    P.cnt[at] = words;
    P.first[at] = first;
    if (words > 0) atomicMax(&P.hdr[q * KFDB_HDR + KFDB_H_MAX], words);
  }
}

#define KFDB_THREADS 1024

// exclusive prefix sum of one int per lane over the workgroup; *total = the sum
__device__ __forceinline__ int kfdb_block_scan(int v, int *s_scan, int tid, int *total) {
  s_scan[tid] = v;
  __syncthreads();
  for (int d = 1; d < KFDB_THREADS; d <<= 1) {
    const int t = tid >= d ? s_scan[tid - d] : 0;
    __syncthreads();
    s_scan[tid] += t;
    __syncthreads();
  }
  const int incl = s_scan[tid];
  *total = s_scan[KFDB_THREADS - 1];
  __syncthreads();
  return incl - v;
}

// dynamic LDS: SortCarve::of(n_slots)
__global__ __launch_bounds__(KFDB_THREADS) void k_kfdb_order(KfdbParams P) {
  extern __shared__ __align__(16) uint8_t smem_kkey[];
  uint64_t *s_kkey = SortCarve::of(P.n_slots).keys.in(smem_kkey);
  __shared__ int s_scan[KFDB_THREADS];
  const int q = blockIdx.x, tid = threadIdx.x;
  const size_t at = (size_t)q * P.n_slots;
  const int32_t *cnt = P.cnt + at;
  const int p2 = sort_p2(P.n_slots);
  const int per = p2 > KFDB_THREADS ? p2 / KFDB_THREADS : 1;   // consecutive sorted positions per lane
  int mine = 0;
  for (int i = tid; i < p2; i += KFDB_THREADS) {
    uint64_t key = KFDB_NOT_LISTED;
    if (i < P.n_slots && cnt[i] > 0) { key = kfdb_order_key(P.first[at + i], (uint32_t)i); mine++; }
    s_kkey[i] = key;
  }
  __syncthreads();
  int listed;
  (void)kfdb_block_scan(mine, s_scan, tid, &listed);
  bitonic_sort_lds<KFDB_THREADS>(s_kkey, p2, tid);
  const int max_common = P.hdr[q * KFDB_HDR + KFDB_H_MAX];
  const int min_common = kfdb_min_common(max_common);
  const int lo = min(tid * per, listed), hi = min(lo + per, listed);
  int pass = 0;
  for (int t = lo; t < hi; t++) pass += kfdb_passes(cnt[(uint32_t)s_kkey[t]], min_common);
  int scored;
  int rank = kfdb_block_scan(pass, s_scan, tid, &scored);
  int32_t *out = P.out_slot + (size_t)q * P.out_stride;
  for (int t = lo; t < hi; t++) {
    const int s = (int)(uint32_t)s_kkey[t];
    if (kfdb_passes(cnt[s], min_common) && rank < P.out_stride) out[rank++] = s;
  }
  if (tid == 0) {
    P.hdr[q * KFDB_HDR + KFDB_H_MIN] = min_common;
    P.hdr[q * KFDB_HDR + KFDB_H_LISTED] = listed;
    P.hdr[q * KFDB_HDR + KFDB_H_SCORED] = min(scored, P.out_stride);
  }
}

__global__ __launch_bounds__(256) void k_kfdb_score(KfdbParams P) {
  const int q = blockIdx.y, lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);   // wave-uniform: position in the scored list
  if (r >= P.hdr[q * KFDB_HDR + KFDB_H_SCORED]) return;
  const size_t o = (size_t)q * P.out_stride + r;
  const int s = P.out_slot[o];
  const KfdbSlot sl = P.slot[s];
  const uint32_t *bm = P.bitmap + (size_t)q * P.bm_stride;
  const uint32_t *ids = P.ids + sl.off;
  const double *val = P.val + sl.off;
  const uint32_t *qid = P.q_id + (size_t)q * P.cap;
  const double *qval = P.q_val + (size_t)q * P.cap;
  const int qn = kfdb_qn(P, q);
  double score = 0;   // ScoringObject.cpp:32; every lane carries the same value
  for (int c = 0; c < sl.n; c += 64) {
    const int i = c + lane;
    bool hit = false;
    double term = 0;
    if (i < sl.n) {
      const uint32_t w = ids[i];
      if (w < (uint32_t)P.n_words && ((bm[w >> 5] >> (w & 31)) & 1u)) {
        int a = 0, b = qn;   // the first query position with id >= w; the bitmap says it holds w
        while (a < b) {
          const int m = (a + b) >> 1;
          if (qid[m] < w) a = m + 1; else b = m;
        }
        if (a < qn && qid[a] == w) { hit = true; term = kfdb_l1_term(qval[a], val[i]); }
      }
    }
    unsigned long long b = __ballot(hit);
    while (b) {   // ascending lane = ascending word id; only hits add
      const int l = __ffsll((long long)b) - 1;
      kfdb_l1_add(&score, __shfl(term, l));
      b &= b - 1;
    }
  }
  if (lane == 0) {
    P.out_score[o] = kfdb_l1_finish(score);
    if (P.out_tag) P.out_tag[o] = sl.tag;
  }
}
