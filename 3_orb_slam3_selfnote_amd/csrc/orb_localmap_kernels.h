// orb_localmap_kernels.h -- Tracking::UpdateLocalMap (Tracking.cc:3542-3762) and the counter and lists of KeyFrame::UpdateConnections
// (KeyFrame.cc:407-492) on the device: orbm_update_local_map*, orbm_update_connections, orbm_gather_local_map_device.  Every compare is a
// function of orb_ref_localmap.h, the host's own statement.
//
//   k_covis_vote      grid (tiles of 256 rows, target): one vote per (row, entry of the row's point) into count[target][G].  Tracking: the
//                     rows are the frame's slots, one target, no filter, slot_bad written.  UpdateConnections: the rows of target t with
//                     the self / bad / other-map filter.  The votes of a workgroup are summed in an LDS table of LM_HIST slots (open
//                     addressing on the keyframe) and leave as one global atomic per keyframe the workgroup met; a vote that finds no
//                     slot within LM_PROBES goes to global memory at once.  A lane walks its own row's list while it has at most 64
//                     entries; longer lists are taken by the whole wavefront in 64-entry tiles, so there is no cap on the entries.
//   k_local_kf_walk   one workgroup: the voted keyframes compacted and sorted by rank (orb_sort.h), the first list and kf_max by a scan
//                     and a maximum, then the expansion and the temporal tail by wavefront 0, one trip after the other.  The marks
//                     (mnTrackReferenceForFrame) are a bit per keyframe in LDS.
//   k_lp_first        the first occurrence of every live point in the reversed walk: an atomic maximum over the complement of
//                     lm_point_key (the scratch is cleared to zero, and zero is "never seen").
//   k_lp_count        one workgroup per local keyframe: the rows that are first occurrences.
//   k_lp_write        one workgroup per local keyframe: its offset is the sum of the counts in front of it; its rows in row order.
//   k_conn_walk       one workgroup per target: compaction, rank sort, kf_max / nmax, threshold or fallback, (weight, rank) sort.
//   k_conn_pack       the targets' lists moved behind each other (conn_start / ord_start), clamped at the capacity.
//   k_gather_mark / k_gather_local_map   the arrays of an orbm_local_map_t from the local-point list and the per-point tables.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "orb_ref_localmap.h"
#include "orb_sort.h"

#define LM_WALK_THREADS 1024
#define LM_HIST 2048            // slots of k_covis_vote's LDS table
#define LM_PROBES 8
#define LM_TILES_X 8            // k_lp_first: tiles of 256 rows in flight per keyframe
#define LM_KF_BLOCKS 128        // k_lp_*: workgroups striding over the local keyframes
#define LM_HDR 4                // scratch header: [0] local keyframes, [1] local points

struct LmTables {   // orbm_map_graph_t on the device
  int G;
  const int32_t *kf_rank; const uint8_t *kf_bad; const int32_t *kf_map, *kf_row_start, *row_point, *kf_best, *kf_child_start, *kf_child, *kf_parent, *kf_prev;
  int P;
  const uint8_t *pt_bad; const int32_t *obs_start, *obs_kf;
};

struct VoteParams {
  LmTables M;
  int n_rows;                  // tracking: N frame slots; connections: unused
  const int32_t *rows;         // tracking: frame_point [N]; connections: NULL (the rows of the target)
  const int32_t *targets;      // connections: [T]; tracking: NULL
  uint8_t *slot_bad;           // tracking: [N]
  int32_t *count;              // [T][G], zero on entry
  int form;                    // 0: LDS table; 1: one global atomic per vote (measurements)
};

// one vote for keyframe k: into the workgroup's table, or straight to global memory
__device__ __forceinline__ void lm_vote(int k, int32_t *s_key, int32_t *s_cnt, int32_t *count, int form) {
  if (form == 0) {
    unsigned h = ((unsigned)k * 2654435761u) >> 21;   // 11 bits
#pragma unroll 1
    for (int i = 0; i < LM_PROBES; i++) {
      const int old = atomicCAS(&s_key[h], -1, k);
      if (old == -1 || old == k) { atomicAdd(&s_cnt[h], 1); return; }
      h = (h + 1) & (LM_HIST - 1);
    }
  }
  atomicAdd(count + k, 1);
}

__global__ __launch_bounds__(256) void k_covis_vote(VoteParams V) {
  __shared__ int32_t s_key[LM_HIST], s_cnt[LM_HIST];
  const LmTables &M = V.M;
  const int lane = threadIdx.x & 63;
  int r0, r1, t = -1, t_map = 0;
  if (V.targets) {
    t = V.targets[blockIdx.y];
    r0 = M.kf_row_start[t]; r1 = M.kf_row_start[t + 1]; t_map = M.kf_map[t];
  } else { r0 = 0; r1 = V.n_rows; }
  if (r0 + (int)blockIdx.x * 256 >= r1) return;                                   // block-uniform
  for (int i = threadIdx.x; i < LM_HIST; i += 256) { s_key[i] = -1; s_cnt[i] = 0; }
  __syncthreads();
  int32_t *count = V.count + (size_t)blockIdx.y * M.G;
  const int i = r0 + blockIdx.x * 256 + threadIdx.x;
  int s0 = 0, s1 = 0;
  bool is_long = false;
  if (i < r1) {
    int p = V.targets ? M.row_point[i] : V.rows[i];
    if (p >= M.P) p = -1;                                                         // the device form cannot look at its tables beforehand
    const bool bad = p >= 0 && M.pt_bad[p] != 0;
    if (V.slot_bad) V.slot_bad[i] = lm_slot_nulled(p, bad);
    if (lm_point_votes(p, bad)) {
      s0 = M.obs_start[p]; s1 = M.obs_start[p + 1];
      if (s1 - s0 > 64) is_long = true;
      else
        for (int e = s0; e < s1; e++) {
          const int k = M.obs_kf[e];
          if ((unsigned)k >= (unsigned)M.G) continue;
          if (t < 0 || conn_entry_counts(k, t, M.kf_bad[k] != 0, M.kf_map[k], t_map)) lm_vote(k, s_key, s_cnt, count, V.form);
        }
    }
  }
  unsigned long long longs = __ballot(is_long);
  while (longs) {
    const int src = (int)__builtin_ctzll(longs);
    longs &= longs - 1;
    const int b0 = __builtin_amdgcn_readlane(s0, src), b1 = __builtin_amdgcn_readlane(s1, src);
    for (int e = b0 + lane; e < b1; e += 64) {
      const int k = M.obs_kf[e];
      if ((unsigned)k >= (unsigned)M.G) continue;
      if (t < 0 || conn_entry_counts(k, t, M.kf_bad[k] != 0, M.kf_map[k], t_map)) lm_vote(k, s_key, s_cnt, count, V.form);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < LM_HIST; j += 256)
    if (s_cnt[j] > 0) atomicAdd(count + s_key[j], s_cnt[j]);
}

// The keyframes with count > 0 as keys (rank, slot) sorted ascending in s_key[0 .. n); returns n.  s_n is one LDS int.
__device__ __forceinline__ int lm_voted_in_rank_order(const LmTables &M, const int32_t *count, uint64_t *s_key, int *s_n) {
  const int tid = threadIdx.x;
  if (tid == 0) *s_n = 0;
  __syncthreads();
  for (int g = tid; g < M.G; g += LM_WALK_THREADS)
    if (count[g] > 0) s_key[atomicAdd(s_n, 1)] = lm_rank_key(M.kf_rank[g], g);
  __syncthreads();
  const int n = *s_n;
  const int p2 = sort_p2(n);
  for (int i = n + tid; i < p2; i += LM_WALK_THREADS) s_key[i] = ~0ull;
  __syncthreads();
  bitonic_sort_lds<LM_WALK_THREADS>(s_key, p2, tid);
  return n;
}

// exclusive scan of one value per lane of the workgroup; *total = the sum.  s_scan has LM_WALK_THREADS ints.
__device__ __forceinline__ int lm_block_scan(int mine, int *s_scan, int *total) {
  const int tid = threadIdx.x;
  s_scan[tid] = mine;
  __syncthreads();
  for (int d = 1; d < LM_WALK_THREADS; d <<= 1) {
    const int v = tid >= d ? s_scan[tid - d] : 0;
    __syncthreads();
    s_scan[tid] += v;
    __syncthreads();
  }
  const int incl = s_scan[tid];
  *total = s_scan[LM_WALK_THREADS - 1];
  __syncthreads();
  return incl - mine;
}

struct WalkParams {
  LmTables M;
  const int32_t *count;         // [G]
  int inertial, last_kf, cap_kf;
  int32_t *list;                // scratch [G + 24]: the whole list, whatever cap_kf
  int32_t *hdr;                 // scratch [LM_HDR]
  int32_t *local_kf;            // [cap_kf]
  int32_t *n_local_kf, *kf_max, *max_votes, *n_local_point;
};

// dynamic LDS: SortCarve::of(G)
__global__ __launch_bounds__(LM_WALK_THREADS) void k_local_kf_walk(WalkParams W) {
  extern __shared__ __align__(16) uint8_t smem_lkey[];
  uint64_t *s_lkey = SortCarve::of(W.M.G).keys.in(smem_lkey);
  __shared__ int s_scan[LM_WALK_THREADS];
  __shared__ uint32_t s_mark[512];                                               // a bit per keyframe, G <= 16384
  __shared__ unsigned long long s_best;
  __shared__ int s_n;
  const LmTables &M = W.M;
  const int tid = threadIdx.x;
  if (tid < 512) s_mark[tid] = 0;
  if (tid == 0) s_best = 0;
  const int n = lm_voted_in_rank_order(M, W.count, s_lkey, &s_n);
  // the first list (:3658-3675): the voted keyframes that are not bad, in rank order; kf_max the first with the largest count
  const int per = (n + LM_WALK_THREADS - 1) / LM_WALK_THREADS;
  const int lo = min(tid * per, n), hi = min(lo + per, n);
  int mine = 0;
  for (int i = lo; i < hi; i++) mine += M.kf_bad[(int)(uint32_t)s_lkey[i]] == 0;
  int first;
  int at = lm_block_scan(mine, s_scan, &first);
  for (int i = lo; i < hi; i++) {
    const int g = (int)(uint32_t)s_lkey[i];
    if (M.kf_bad[g]) continue;
    W.list[at] = g;
    if (at < W.cap_kf) W.local_kf[at] = g;
    atomicOr(&s_mark[g >> 5], 1u << (g & 31));
    // lm_beats is strict: among equal counts the smallest place wins
    atomicMax(&s_best, ((unsigned long long)(uint32_t)W.count[g] << 32) | (uint32_t)(0x7fffffff - at));
    at++;
  }
  __syncthreads();
  if (tid >= 64) return;
  // the expansion (:3680-3733) and the tail (:3737-3754) by one wavefront: every trip depends on the marks of the one before
  const int lane = tid;
  int size = first;
  volatile uint32_t *mark = s_mark;                                               // lane 0 writes, every lane reads: LDS accesses of one wavefront stay in order
  auto marked = [&](int g) { return (mark[g >> 5] >> (g & 31)) & 1u; };
  auto append = [&](int g) {                                                      // wave-uniform g
    if (lane == 0) {
      W.list[size] = g;
      if (size < W.cap_kf) W.local_kf[size] = g;
      mark[g >> 5] = mark[g >> 5] | (1u << (g & 31));
    }
    __builtin_amdgcn_wave_barrier();
    size++;
  };
  for (int i = 0; i < first; i++) {
    if (lm_expansion_stops(size)) break;
    const int g = (int)(uint32_t)__builtin_amdgcn_readfirstlane(i < first ? W.list[i] : 0);   // list[i], i < first: written before the barrier
    {                                                                             // :3693-3705
      const int nb = lane < LM_BEST ? M.kf_best[(size_t)g * LM_BEST + lane] : -1;
      const unsigned long long ended = __ballot(lane < LM_BEST && nb < 0);        // the vector ends at the first -1
      const int len = ended ? (int)__builtin_ctzll(ended) : LM_BEST;
      const bool take = lane < len && !M.kf_bad[nb] && !marked(nb);
      const unsigned long long b = __ballot(take);
      if (b) append(__builtin_amdgcn_readlane(nb, (int)__builtin_ctzll(b)));
    }
    const int c0 = M.kf_child_start[g], c1 = M.kf_child_start[g + 1];             // :3708-3720
    for (int base = c0; base < c1; base += 64) {
      const int c = base + lane;
      const int ch = c < c1 ? M.kf_child[c] : -1;
      const bool take = ch >= 0 && !M.kf_bad[ch] && !marked(ch);
      const unsigned long long b = __ballot(take);
      if (b) { append(__builtin_amdgcn_readlane(ch, (int)__builtin_ctzll(b))); break; }
    }
    const int par = M.kf_parent[g];                                               // :3723-3732
    if (par >= 0 && !marked(par)) { append(par); break; }
  }
  if (lm_tail_runs(W.inertial != 0, size)) {
    int t = W.last_kf;
    for (int i = 0; i < LM_TAIL_TRIPS; i++) {
      if (t < 0) break;
      if (marked(t)) break;                                                       // the reference does not advance: the other trips change nothing
      append(t);
      t = M.kf_prev[t];
    }
  }
  if (lane == 0) {
    const unsigned long long best = s_best;
    const int best_at = 0x7fffffff - (int)(uint32_t)best;
    *W.max_votes = (int)(best >> 32);
    *W.kf_max = best ? W.list[best_at] : -1;
    *W.n_local_kf = size;
    W.hdr[0] = size;
    if (size == 0) { *W.n_local_point = 0; W.hdr[1] = 0; }
  }
}

struct LpParams {
  LmTables M;
  const int32_t *list, *hdr;
  uint32_t *pt_word;            // [P], zero on entry: the complement of the smallest key
  int32_t *kf_count;            // [G + 24] by reversed position
  int cap_pts;
  int32_t *local_point, *n_local_point;
};

// rows of the keyframe at reversed position j: at most LM_MAX_ROWS are walked (the host forms refuse more; the device form cannot look)
__device__ __forceinline__ void lp_rows(const LpParams &L, int n_kf, int j, int &r0, int &nr) {
  const int g = L.list[n_kf - 1 - j];
  r0 = L.M.kf_row_start[g];
  nr = min(L.M.kf_row_start[g + 1] - r0, LM_MAX_ROWS);
}

__global__ __launch_bounds__(256) void k_lp_first(LpParams L) {
  const int n_kf = L.hdr[0];
  for (int j = blockIdx.y; j < n_kf; j += gridDim.y) {
    int r0, nr;
    lp_rows(L, n_kf, j, r0, nr);
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nr; i += 256 * LM_TILES_X) {
      const int p = L.M.row_point[r0 + i];
      if (p >= 0 && !L.M.pt_bad[p]) atomicMax(L.pt_word + p, ~lm_point_key(j, i));
    }
  }
}

// the rows of this lane's tile position that are first occurrences; returns the workgroup's exclusive rank and the tile's total
__device__ __forceinline__ bool lp_is_first(const LpParams &L, int j, int r0, int i, int nr, int &p) {
  p = i < nr ? L.M.row_point[r0 + i] : -1;
  return p >= 0 && !L.M.pt_bad[p] && L.pt_word[p] == ~lm_point_key(j, i);
}

__global__ __launch_bounds__(256) void k_lp_count(LpParams L) {
  __shared__ int s_sum;
  const int n_kf = L.hdr[0];
  for (int j = blockIdx.x; j < n_kf; j += gridDim.x) {
    int r0, nr, p, mine = 0;
    lp_rows(L, n_kf, j, r0, nr);
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < nr; i += 256) mine += lp_is_first(L, j, r0, i, nr, p);
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_sum, mine);
    __syncthreads();
    if (threadIdx.x == 0) L.kf_count[j] = s_sum;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_lp_write(LpParams L) {
  __shared__ int s_sum, s_wave[4];
  const int n_kf = L.hdr[0], lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = blockIdx.x; j < n_kf; j += gridDim.x) {
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    int before = 0;
    for (int q = threadIdx.x; q < j; q += 256) before += L.kf_count[q];
    for (int d = 32; d > 0; d >>= 1) before += __shfl_down(before, d);
    if (lane == 0 && before) atomicAdd(&s_sum, before);
    __syncthreads();
    int at = s_sum;                                                               // the points of the keyframes walked before this one
    if (j == n_kf - 1 && threadIdx.x == 0) { *L.n_local_point = at + L.kf_count[j]; ((int32_t *)L.hdr)[1] = at + L.kf_count[j]; }
    int r0, nr;
    lp_rows(L, n_kf, j, r0, nr);
    for (int base = 0; base < nr; base += 256) {                                  // tiles in row order
      int p;
      const bool first = lp_is_first(L, j, r0, base + (int)threadIdx.x, nr, p);
      const unsigned long long b = __ballot(first);
      if (lane == 0) s_wave[wave] = __popcll(b);
      __syncthreads();
      int off = at;
      for (int w = 0; w < wave; w++) off += s_wave[w];
      off += __popcll(b & ((1ull << lane) - 1));
      if (first && off < L.cap_pts) L.local_point[off] = p;
      at += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
      __syncthreads();
    }
    __syncthreads();                                                              // all have read s_sum before the next keyframe clears it
  }
}

struct ConnParams {
  LmTables M;
  const int32_t *count;         // [T][G]
  const int32_t *targets;       // [T]
  int T, th, cap;
  // per target at stride G (scratch)
  int32_t *w_conn_kf, *w_conn_w, *w_ord_kf, *w_ord_w;
  int32_t *n_conn, *n_ord;      // [T] (scratch)
  // outputs
  int32_t *conn_start, *conn_kf, *conn_w, *ord_start, *ord_kf, *ord_w;   // [T+1], [cap], [cap], [T+1], [cap], [cap]
  int32_t *kf_max, *nmax;       // [T]
};

// dynamic LDS: SortCarve::of(G)
__global__ __launch_bounds__(LM_WALK_THREADS) void k_conn_walk(ConnParams C) {
  extern __shared__ __align__(16) uint8_t smem_ckey[];
  uint64_t *s_ckey = SortCarve::of(C.M.G).keys.in(smem_ckey);
  __shared__ unsigned long long s_best;
  __shared__ int s_n, s_pairs;
  const LmTables &M = C.M;
  const int tid = threadIdx.x, t = blockIdx.x;
  const int32_t *count = C.count + (size_t)t * M.G;
  int32_t *ckf = C.w_conn_kf + (size_t)t * M.G, *cw = C.w_conn_w + (size_t)t * M.G, *okf = C.w_ord_kf + (size_t)t * M.G, *ow = C.w_ord_w + (size_t)t * M.G;
  if (tid == 0) { s_best = 0; s_pairs = 0; }
  const int n = lm_voted_in_rank_order(M, count, s_ckey, &s_n);                   // KFcounter in iteration order
  for (int i = tid; i < n; i += LM_WALK_THREADS) {
    const int g = (int)(uint32_t)s_ckey[i], w = count[g];
    ckf[i] = g; cw[i] = w;
    atomicMax(&s_best, ((unsigned long long)(uint32_t)w << 32) | (uint32_t)(0x7fffffff - i));
  }
  __syncthreads();                                                                // the keys have been read; ckf / cw are visible to the workgroup
  const unsigned long long best = s_best;
  const int best_at = 0x7fffffff - (int)(uint32_t)best, nmax = (int)(best >> 32);
  // vPairs (:464-475) as keys that sort ascending into the reversed order of sort(vPairs): weight descending, then rank descending
  for (int i = tid; i < n; i += LM_WALK_THREADS)
    if (conn_is_pair(cw[i], C.th)) s_ckey[atomicAdd(&s_pairs, 1)] = ((uint64_t)(uint32_t)(0x7fffffff - cw[i]) << 32) | (uint32_t)(0x7fffffff - i);
  __syncthreads();
  if (n > 0 && s_pairs == 0 && tid == 0) { s_ckey[0] = ((uint64_t)(uint32_t)(0x7fffffff - nmax) << 32) | (uint32_t)(0x7fffffff - best_at); s_pairs = 1; }
  __syncthreads();
  const int np = s_pairs;
  const int p2 = sort_p2(np);
  for (int i = np + tid; i < p2; i += LM_WALK_THREADS) s_ckey[i] = ~0ull;
  __syncthreads();
  bitonic_sort_lds<LM_WALK_THREADS>(s_ckey, p2, tid);
  for (int i = tid; i < np; i += LM_WALK_THREADS) {
    const int at = 0x7fffffff - (int)(uint32_t)s_ckey[i];
    okf[i] = ckf[at]; ow[i] = 0x7fffffff - (int)(uint32_t)(s_ckey[i] >> 32);
  }
  if (tid == 0) { C.n_conn[t] = n; C.n_ord[t] = np; C.kf_max[t] = n > 0 ? ckf[best_at] : -1; C.nmax[t] = nmax; }
}

__global__ __launch_bounds__(256) void k_conn_pack(ConnParams C) {
  __shared__ int s_a, s_b;
  const int t = blockIdx.x, lane = threadIdx.x & 63, G = C.M.G;
  if (threadIdx.x == 0) { s_a = 0; s_b = 0; }
  __syncthreads();
  int a = 0, b = 0;
  for (int q = threadIdx.x; q < t; q += 256) { a += C.n_conn[q]; b += C.n_ord[q]; }
  for (int d = 32; d > 0; d >>= 1) { a += __shfl_down(a, d); b += __shfl_down(b, d); }
  if (lane == 0) { if (a) atomicAdd(&s_a, a); if (b) atomicAdd(&s_b, b); }
  __syncthreads();
  const int a0 = s_a, b0 = s_b, na = C.n_conn[t], nb = C.n_ord[t];
  if (threadIdx.x == 0) {
    C.conn_start[t] = a0; C.ord_start[t] = b0;
    if (t == C.T - 1) { C.conn_start[C.T] = a0 + na; C.ord_start[C.T] = b0 + nb; }
  }
  for (int i = threadIdx.x; i < na; i += 256)
    if (a0 + i < C.cap) { C.conn_kf[a0 + i] = C.w_conn_kf[(size_t)t * G + i]; C.conn_w[a0 + i] = C.w_conn_w[(size_t)t * G + i]; }
  for (int i = threadIdx.x; i < nb; i += 256)
    if (b0 + i < C.cap) { C.ord_kf[b0 + i] = C.w_ord_kf[(size_t)t * G + i]; C.ord_w[b0 + i] = C.w_ord_w[(size_t)t * G + i]; }
}

struct GatherParams {
  int P, N, cap;
  const int32_t *frame_point;   // [N]
  const int32_t *local_point, *n_local_point;
  const uint8_t *pt_bad;
  const float *Xw, *normal, *max_dist, *min_dist; const uint8_t *mpdesc, *obs;   // per point; obs may be NULL
  uint8_t *in_frame;            // scratch [P], zero on entry
  uint8_t *o_eligible; float *o_Xw, *o_normal, *o_max_dist, *o_min_dist; uint8_t *o_mpdesc, *o_obs;   // o_obs may be NULL
  int32_t *map_n;
};

__global__ __launch_bounds__(256) void k_gather_mark(GatherParams A) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= A.N) return;
  const int p = A.frame_point[s];
  if (p >= 0 && p < A.P) A.in_frame[p] = 1;
}

// eight lanes per point: each moves four bytes of the descriptor, the first seven one float of Xw / normal / the distances
__global__ __launch_bounds__(256) void k_gather_local_map(GatherParams A) {
  const int n = min(max(*A.n_local_point, 0), A.cap);
  if (blockIdx.x == 0 && threadIdx.x == 0) *A.map_n = n;
  const int i = blockIdx.x * 32 + (threadIdx.x >> 3), part = threadIdx.x & 7;
  if (i >= n) return;
  const int p = A.local_point[i];
  ((uint32_t *)A.o_mpdesc)[(size_t)i * 8 + part] = ((const uint32_t *)A.mpdesc)[(size_t)p * 8 + part];
  if (part < 3) A.o_Xw[(size_t)i * 3 + part] = A.Xw[(size_t)p * 3 + part];
  else if (part < 6) A.o_normal[(size_t)i * 3 + part - 3] = A.normal[(size_t)p * 3 + part - 3];
  else if (part == 6) { A.o_max_dist[i] = A.max_dist[p]; A.o_min_dist[i] = A.min_dist[p]; }
  else {
    A.o_eligible[i] = !A.pt_bad[p] && !A.in_frame[p];                             // Tracking.cc:3453-3471, :3483-3487
    if (A.o_obs) A.o_obs[i] = A.obs ? A.obs[p] : 1;
  }
}
