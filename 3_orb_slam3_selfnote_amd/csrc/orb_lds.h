// orb_lds.h -- the two pieces every dynamic-LDS layout ("carve") of liborbhip is written with.  A kernel that takes dynamic LDS has a
// carve type beside it in its kernel header: one LdsRegion member per array and `bytes`, made by ONE function `of(...)` of values that
// both the kernel and the host have.  The kernel takes its pointers from it, the host launches with its `bytes`; nobody else adds up
// offsets or sizes (tests/test_lds_carves.py prints and checks every carve, DESIGN.md "LDS carves").
// A kernel that is not given a count the host has (the most table entries of any tile, the most cells of any level, the batch's maxn)
// passes 0 or its own smaller count for it.  That is right only because such a count sizes the LAST region of its carve (or the only
// one): a count changes nothing in front of its own region.  Whoever adds a region behind one of these gives the kernel the count.
#pragma once
#include <stdint.h>
#include <stddef.h>

// gfx950 has 160 KiB of LDS per CU; a workgroup's static __shared__ and its dynamic carve share it.
#define ORB_LDS_LIMIT (160 * 1024)

// `count` elements of T at byte `off` of the dynamic LDS block, aligned to `align`.  over = the region deliberately lies over earlier
// ones (its carve says which, and why the two are never live together); every other region starts where the one before it ends.
template <typename T>
struct LdsRegion {
  int off, count, align;
  bool over;
  // lds + off, taken as whole elements and a remainder (0 unless T is a record whose size is no power of two): an element index is
  // what the kernels' own pointer arithmetic gave the compiler
  __host__ __device__ T *in(void *lds) const { return reinterpret_cast<T *>(static_cast<uint8_t *>(lds) + off % (int)sizeof(T)) + off / (int)sizeof(T); }
  __host__ __device__ constexpr int size() const { return count * (int)sizeof(T); }
  __host__ __device__ constexpr int end() const { return off + size(); }
};

struct LdsCarver {
  int at = 0;
  template <typename T>
  __host__ __device__ constexpr LdsRegion<T> take(int count, int align = alignof(T)) {
    const int off = (at + align - 1) & ~(align - 1);
    at = off + count * (int)sizeof(T);
    return {off, count, align, false};
  }
  template <typename T>
  __host__ __device__ static constexpr LdsRegion<T> over(int off, int count, int align = alignof(T)) { return {off, count, align, true}; }
};
