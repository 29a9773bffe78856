// orb_sort.h -- the sort that k_close_points (orb_depth_kernels.h) and k_voc_collect (orb_voc_kernels.h) share: a bitonic sort of
// 64-bit keys in LDS by one workgroup of THREADS lanes.  p2 is a power of two >= 2 and s_key[0 .. p2) is filled (padding = ~0ull,
// which sorts last) and made visible by a barrier before the call; the sorted keys are visible to every lane on return.  The network
// is oblivious of the data, so with UNIQUE keys any two correct sorts give the same array: callers put the element's index into the
// low bits and get a stable order by construction.
#pragma once
#include <stdint.h>
#include "orb_lds.h"

// The sort's length for n keys: the power of two >= max(n, 2).  The one definition, for the kernels and for the host.
__host__ __device__ constexpr int sort_p2(int n) { int p2 = 2; while (p2 < n) p2 <<= 1; return p2; }

// Dynamic LDS of a kernel that sorts up to `cap` keys in it (k_local_kf_walk, k_conn_walk, k_voc_collect, k_kfdb_order): the keys.
// cap <= 16384 in all four (128 KiB), beside at most 3 KiB of static LDS.
struct SortCarve {
  LdsRegion<uint64_t> keys;
  int bytes;
  __host__ __device__ static constexpr SortCarve of(int cap) {
    LdsCarver c;
    SortCarve s{c.take<uint64_t>(sort_p2(cap)), 0};
    s.bytes = c.at;
    return s;
  }
};

template <int THREADS>
__device__ __forceinline__ void bitonic_sort_lds(uint64_t *s_key, int p2, int tid) {
  for (int k = 2; k <= p2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (p2 >> 1); t += THREADS) {
        const int lo = 2 * t - (t & (j - 1)), hi = lo + j;
        const uint64_t a = s_key[lo], b = s_key[hi];
        if ((a > b) == ((lo & k) == 0)) { s_key[lo] = b; s_key[hi] = a; }
      }
      __syncthreads();
    }
}
