// orb_kernels.h -- hand-written gfx950 kernels of the ORB extractor (included once, by orbhip.hip).
//
// Kernel inventory (roofline per kernel in DESIGN.md):
//   k_resize    K1  cv::resize INTER_LINEAR 8U, one pyramid level of every frame per launch
//   k_pyramid_chain K1  the same planes in ONE launch for single-frame calls (a tile recomputes the levels below it in LDS)
//   k_fast      K2  FAST-9/16 score + per-cell NMS, cell detected at iniThFAST and again at minThFAST if empty, one wavefront per 30-px cell
//   k_octree    K3  DistributeOctTree, one workgroup per (frame, level), node list in LDS
//   k_blur      K5  7x7 sigma-2 fixed-point Gaussian as two int8 MFMA products, 128x32 tiles staged through LDS
//   k_describe  K4+K6+K7  IC_Angle + steered BRIEF + lapping-order scatter + frame totals, one wavefront per block of 8 keypoint slots
//                         (one per keypoint in few-frame calls)
// All arithmetic is integer or non-contracted IEEE fp32/fp64 (hipcc -ffp-contract=off) so results are bit-exact
// against the CPU restatement the tests use.  No MFMA: this is byte/bit work bound by HBM, LDS and VALU integer rate.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "orb_common.h"
#include "orb_lds.h"
#include "orb_fast_score.h"
#include "orb_sincos.h"

#define WAVE 64

__constant__ __attribute__((aligned(16))) int8_t c_pattern[1024] = {
#include "../../include/orb_pattern_data.inc"
};

// Offsets (u, v) of the 749 pixels of the radius-15 intensity-centroid disc, rows v = -15..15, u = -umax[|v|]..umax[|v|]
// (ORBextractor.cc:452-467 always yields umax = 15,15,15,15,14,14,14,13,13,12,11,10,9,8,6,3 for HALF_PATCH_SIZE 15;
// orbx_create re-derives umax at run time and refuses to start if it differs).  Padded to 768 with (0,0), which
// contributes u*I = v*I = 0 to the moments.
// Stored per lane: lane L handles disc pixels L, 64+L, ..., 704+L; its twelve u offsets are bytes 0..11 and its twelve
// v offsets bytes 12..23 of w[L][0..5], so one lane fetches its share of the table with two wide loads.
struct DiscTab { uint32_t w[64][6]; };
constexpr int kDiscUmax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
constexpr DiscTab make_disc_tab() {
  DiscTab t{};
  int n = 0;
  for (int v = -15; v <= 15; v++) {
    const int d = kDiscUmax[v < 0 ? -v : v];
    for (int u = -d; u <= d; u++) {
      const int lane = n & 63, k = n >> 6;  // pixel n = k * 64 + lane
      t.w[lane][k >> 2] |= (uint32_t)(uint8_t)(int8_t)u << (8 * (k & 3));
      t.w[lane][3 + (k >> 2)] |= (uint32_t)(uint8_t)(int8_t)v << (8 * (k & 3));
      n++;
    }
  }
  return t;  // pixels 749..767 stay (0, 0)
}
__constant__ __attribute__((aligned(16))) DiscTab c_disc = make_disc_tab();
// the same umax, four bits per row distance |v|: the block form of k_describe derives its per-row weights from it in registers
constexpr uint64_t make_disc_umax_nibbles() {
  uint64_t p = 0;
  for (int v = 0; v < 16; v++) p |= (uint64_t)kDiscUmax[v] << (4 * v);
  return p;
}

// ------------------------------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect101(int p, int n) {
  if (n == 1) return 0;
  while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
  return p;
}

__device__ __forceinline__ const uint8_t *level_plane(const FrameParams &P, int frame, int level, int &pitch) {
  if (level == 0) {
    pitch = (int)P.img0_stride;
    return P.img0 + (size_t)frame * P.img0_frame_stride;
  }
  pitch = P.geom[level].pitch;
  return P.pyr + (size_t)frame * P.pyr_fs + P.geom[level].off;
}

// XCD-aware block -> (frame, item) mapping.  Workgroups are dealt round-robin over the 8 XCDs (block b lands on XCD
// b % 8, MI355X_MICROARCH.md "Workgroup dispatch"), and each XCD has its own 4 MiB L2.  All items of frame f are
// therefore placed on XCD f % 8: neighbouring FAST cells / blur tiles / keypoint patches of one frame share cache
// lines and halo rows, and with this mapping they are fetched into ONE L2 instead of up to eight.  Placement only
// affects speed, never results.  Grid: 1-D, nframes * nitems blocks.
// magic = floor(2^32 / nitems) (host): the quotient estimate is at most one too small, one correction makes it exact.
__device__ __forceinline__ void xcd_map(int nitems, uint32_t magic, int nframes, int &frame, int &item) {
  const unsigned b = blockIdx.x;
  const unsigned full = (unsigned)(nframes & ~7);
  const unsigned nfull = full * (unsigned)nitems;
  const bool inFull = b < nfull;
  const unsigned q = inFull ? (b >> 3) : (b - nfull);
  unsigned g = __umulhi(q, magic);
  unsigned r = q - g * (unsigned)nitems;
  if (r >= (unsigned)nitems) { g++; r -= (unsigned)nitems; }
  frame = (int)(inFull ? (b & 7u) + 8u * g : full + g);
  item = (int)r;
}

// Wave-wide sum through DPP (row_shr 1/2/4/8, row_bcast15, row_bcast31): no LDS traffic; the result is uniform.
// All 64 lanes must be active.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ int dpp_or_zero(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, ROWMASK, 0xf, false); }
// Low 32 bits of a 24 x 24-bit product: v_mul_u32_u24, full rate (v_mul_lo_u32 / v_mul_hi_u32 issue at a quarter of it).
// Inline assembly because the instruction selector only forms it when it can prove both operands 24-bit, which it cannot
// for loop indices bounded by a compare.  mul24(a, u): u wave-uniform (scalar operand).
__device__ __forceinline__ uint32_t mul24(uint32_t a, uint32_t u) {
  uint32_t d;
  asm("v_mul_u32_u24 %0, %1, %2" : "=v"(d) : "s"(u), "v"(a));
  return d;
}
// both operands per lane; the caller guarantees 24 bits
__device__ __forceinline__ uint32_t mul24_vv(uint32_t a, uint32_t b) { return __umul24(a, b); }

__device__ __forceinline__ int wave_sum_i32(int v) {
  v += dpp_or_zero<0x111, 0xf>(v);
  v += dpp_or_zero<0x112, 0xf>(v);
  v += dpp_or_zero<0x114, 0xf>(v);
  v += dpp_or_zero<0x118, 0xf>(v);
  v += dpp_or_zero<0x142, 0xa>(v);
  v += dpp_or_zero<0x143, 0xc>(v);
  return __builtin_amdgcn_readlane(v, 63);
}

// inclusive scan inside a wavefront
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
  // DPP: row_shr 1, 2, 4, 8 scan each row of 16 lanes, row_bcast15 / row_bcast31 carry the row totals on (six vector instructions;
  // the __shfl_up form is six trips through the LDS crossbar)
  int v = (int)x;
  v += dpp_or_zero<0x111, 0xf>(v);
  v += dpp_or_zero<0x112, 0xf>(v);
  v += dpp_or_zero<0x114, 0xf>(v);
  v += dpp_or_zero<0x118, 0xf>(v);
  v += dpp_or_zero<0x142, 0xa>(v);
  v += dpp_or_zero<0x143, 0xc>(v);
  return (uint32_t)v;
}

// Exclusive scan of an LDS array a[0..n) in place using all NT threads (blockDim.x == NT, 1-D block).
// Returns the total.  sw: LDS scratch of NT/64 + 2 words.
template <int NT>
__device__ uint32_t lds_excl_scan(uint32_t *a, int n, uint32_t *sw) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  constexpr int NW = NT / 64;
  uint32_t carry = 0;
  for (int base = 0; base < n; base += NT) {
    int i = base + tid;
    uint32_t v = i < n ? a[i] : 0u;
    uint32_t inc = wave_incl_scan(v);
    if (lane == 63) sw[wid] = inc;
    __syncthreads();
    // the NW wave totals are scanned in registers by every wavefront (one LDS read per lane instead of NW per thread)
    const uint32_t wsum = lane < NW ? sw[lane] : 0u;
    const uint32_t wincl = wave_incl_scan(wsum);
    const int widu = __builtin_amdgcn_readfirstlane(wid);
    const uint32_t woff = (uint32_t)__builtin_amdgcn_readlane((int)(wincl - wsum), widu);
    const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)wincl, NW - 1);
    if (i < n) a[i] = carry + woff + inc - v;
    carry += tot;
    __syncthreads();
  }
  return carry;
}

// ------------------------------------------------------------------------------------------------------------
// K1: cv::resize INTER_LINEAR 8UC1.  Level `level` of every frame from level-1.
// Tables {sx, a0|a1<<16} / {sy, b0|b1<<16} are built on the host (orbx_configure); the result is
//   (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2,   r = S[sy][sx] * a0 + S[sy][sx + 1] * a1   for rows sy, sy + 1.
// Workgroup = G.resizeRows (16 or 8) output rows x full width.
//
// Two-pass form (tPitch > 0, the host's choice whenever a tile's source rows fit the LDS stage): the horizontal interpolation r >> 4
// of a source row is shared by the two output rows that straddle it, so it is evaluated once per (source row, output column) -
// about 1.35 per output pixel for 16-row tiles at scale 1.2 instead of 2 - into a 16-bit LDS plane T, and the vertical pass reads
// four finished values with one 8-byte LDS load (SQ_INSTS_VALU per launch 13.3 M -> 9.8 M against the one-pass gather form).
// One-pass form (tPitch == 0): extreme scale factors, straight from global memory.
// ------------------------------------------------------------------------------------------------------------
// Output rows per workgroup: 16 (late round 3; 8 before) - a tile's source rows come in with ONE HBM round trip, and twice the rows
// behind it is twice the work per wait (the same reasoning as k_blur's 64-row tiles); alone on the chip the kernel is as fast as before,
// beside the other pipelines the step gains 2 % (16: 208-211 k frames/s, 8: 204-207 k, 24: 206 k, 32: 201 k).  Levels whose 16-row stage
// would not fit the LDS (images wider than ~2600 columns) take 8-row tiles (G.resizeRows, decided in orbx_configure).
#define RESIZE_MAXSRC 32   // most source rows per tile the two-pass form stages (16 rows at scale 2: 32)
// Diagnostic builds (-DFAST_STAMPS, -DOCT_STAMPS, -DTILE_STAMPS; tools/fast_stamps.py, octree_stamps.py, tile_stamps.py): cycle stamps of
// thread 0 of every workgroup, eight words per workgroup.
#if defined(FAST_STAMPS) || defined(OCT_STAMPS) || defined(TILE_STAMPS)
__device__ unsigned int *g_fast_stamps;  // [workgroup][8], set by orbx_debug_fast_stamps
#endif
// -DTILE_STAMPS: k_blur's workgroups take rows 0 .. totalTiles * nframes - 1 of the buffer, k_resize's follow level by level.  Words:
// cycles from kernel entry to 0 "tile fetch issued", 1 "tile landed" (behind the barrier), 2 the end;  3: level + 1.
#ifdef TILE_STAMPS
#define TSTAMP_BEGIN() const long long ts0_ = __builtin_readcyclecounter()
#define TSTAMP(i, rowExpr, lvl) do { const long long t_ = __builtin_readcyclecounter(); if (threadIdx.x == 0 && g_fast_stamps) { const size_t r_ = (rowExpr); g_fast_stamps[r_ * 8 + (i)] = (unsigned int)(t_ - ts0_); g_fast_stamps[r_ * 8 + 3] = (unsigned int)((lvl) + 1); } } while (0)
__device__ __forceinline__ size_t resize_stamp_row(const FrameParams &P, int level) {
  size_t row = (size_t)P.totalTiles * P.nframes + blockIdx.x;
  for (int l = 1; l < level; l++) row += (size_t)((P.geom[l].h + P.geom[l].resizeRows - 1) / P.geom[l].resizeRows) * P.nframes;
  return row;
}
#else
#define TSTAMP_BEGIN() do {} while (0)
#define TSTAMP(i, rowExpr, lvl) do {} while (0)
#endif
#define RSTAMP(i) TSTAMP(i, resize_stamp_row(P, level), level)
// k_resize's dynamic LDS.  Two-pass form (tPitch > 0): the tile's source rows, their horizontally interpolated rows, the tile record's
// row part.  One-pass form (tPitch == 0): the level's x table alone.
__host__ __device__ constexpr int resize_row_bytes(int srcW) { return (srcW + 4 + 15) & ~15; }   // a source row and the 4 bytes pass 1 reads past it, in chunks
__host__ __device__ constexpr int resize_t_pitch(int wq) { return (wq * 2 + 7) & ~7; }           // 16 bits per column of the padded level width
struct ResizeCarve {
  LdsRegion<uint8_t> rows;     // [maxSrc][rowBytes]: whole 16-byte chunks land here by LDS-DMA
  LdsRegion<uint8_t> t;        // [maxSrc][tPitch], u16 entries
  LdsRegion<uint4> rowRec;     // [RESIZE_ROWS_MAX], 16-byte aligned for its ds_read_b128 / ds_write_b128 (tPitch is a multiple of 8 only)
  LdsRegion<int2> xtab;        // one-pass: [wq]
  int bytes;
  __host__ __device__ static constexpr ResizeCarve of(int maxSrc, int rowBytes, int tPitch, int wq) {
    LdsCarver c;
    const bool two = tPitch > 0;
    ResizeCarve r{c.take<uint8_t>(two ? maxSrc * rowBytes : 0, 16), c.take<uint8_t>(two ? maxSrc * tPitch : 0),
                  c.take<uint4>(two ? RESIZE_ROWS_MAX : 0, 16), c.take<int2>(two ? 0 : wq), 0};
    r.bytes = c.at;
    return r;
  }
};
#define RESIZE_LDS_MAX (ORB_LDS_LIMIT - 1024)   // either form: leaves 1 KiB for the kernel's static LDS (the one-pass form's y entries, 128 B)
#define RESIZE_STAGE_MAX (64 * 1024)            // a 16-row tile's rows + T rows: two workgroups per CU beside everything else; else 8-row tiles
__global__ __launch_bounds__(256) void k_resize(FrameParams P, int level, int smemRowBytes, int tPitch, int maxSrc) {
  TSTAMP_BEGIN();
  extern __shared__ __align__(16) uint8_t smem_rs[];
  const LevelGeom G = P.geom[level];
  const LevelGeom Gs = P.geom[level - 1];
  const int tid = threadIdx.x;
  int frame, rowTile;
  xcd_map((G.h + G.resizeRows - 1) / G.resizeRows, G.rowTileMagic, P.nframes, frame, rowTile);
  int spitch;
  const uint8_t *src = level_plane(P, frame, level - 1, spitch);
  uint8_t *dstplane = P.pyr + (size_t)frame * P.pyr_fs + G.off;
  const int wq = (G.w + 3) & ~3, qw = wq >> 2;   // the x table is padded to whole output quads with copies of its last entry (host)
  // (taken here, in front of the branch, so that the table's address arrives with the other kernel arguments)
  const uint32_t *tileRec = P.resizeRecs + (size_t)(G.resizeRecBase + rowTile) * RESIZE_REC_WORDS;

  if (tPitch > 0) {
    // The row tile's record (orbx_configure, layout in orb_common.h), built from the y table on the host: the group part is one
    // scalar load that depends on the kernel arguments alone - read through the constant address space, as k_fast reads its
    // records (the host alone writes the table) -, so no vector-memory round trip stands in front of the staging below.
    typedef uint32_t rec4_t __attribute__((ext_vector_type(4)));
    const __attribute__((address_space(4))) uint32_t *rec = (const __attribute__((address_space(4))) uint32_t *)tileRec;
    const rec4_t gr = *reinterpret_cast<const __attribute__((address_space(4))) rec4_t *>(rec);
    const int syFirst = (int)gr[0], nsrc = (int)gr[1], nrows = (int)gr[2];   // source row span of this tile (at most maxSrc rows), its output rows
    const auto lds = ResizeCarve::of(maxSrc, smemRowBytes, tPitch, wq);
    uint8_t *sRows = lds.rows.in(smem_rs), *sT = lds.t.in(smem_rs);
    uint4 *sRowRec = lds.rowRec.in(smem_rs);
    // this thread's first two column pairs of pass 1, loaded ahead of the staging (a level up to 1024 columns wide needs no more)
    const int4 *xtab4 = reinterpret_cast<const int4 *>(P.xtab + G.xtabBase);
    int4 xtPre[2];
#pragma unroll
    for (int k = 0; k < 2; k++) { const int p = tid + 256 * k; xtPre[k] = 2 * p < wq ? xtab4[p] : make_int4(0, 0, 0, 0); }
    // per output row of the tile: where its two T rows start, its coefficient pair, where it goes - the record's row part, 16 bytes
    // per lane by LDS-DMA (lane-linear: row r lands in sRowRec[r]); pass 2 reads it behind the barriers that are there anyway
    if (tid < nrows)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(tileRec + RESIZE_REC_GROUP_WORDS + 4 * tid),
                                       (__attribute__((address_space(3))) void *)sRowRec, 16, 0, 0);
    const bool aligned = ((((uintptr_t)src) | (uintptr_t)spitch) & 3u) == 0;
    // Index arithmetic: 32-bit integer multiplies issue at a quarter of the full rate, so idx / ndw is taken in float --
    // (idx + 0.5) / ndw stays at least 0.5 / ndw >= 2^-11 away from an integer while the rounding error of the product is
    // below 2^-19 for idx < 2^14, so truncation yields the exact quotient -- and offsets use 24-bit multiplies (mul24).
    const uint8_t *src0 = src + (size_t)syFirst * spitch;
    if (aligned) {
      // Full 16-byte chunks of every source row by LDS-DMA (global_load_lds_dwordx4: no register, no ds_write).  The LDS rows
      // are smemRowBytes = 16 * cpr long; the loop runs over all cpr chunk positions so that the LDS image stays lane-linear
      // (destination = wave base + lane * 16), the positions past the last full chunk simply stay inactive.
      const int cpr = smemRowBytes >> 4, nfull = Gs.w >> 4;
      const float inv_cpr = 1.0f / (float)cpr;
      for (int idx = tid; idx < cpr * nsrc; idx += 256) {
        const int r = (int)(((float)idx + 0.5f) * inv_cpr), c = idx - (int)mul24((uint32_t)r, (uint32_t)cpr);
        if (c < nfull)
          __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src0 + (mul24((uint32_t)r, (uint32_t)spitch) + 16u * (uint32_t)c)),
                                           (__attribute__((address_space(3))) void *)(sRows + (size_t)(idx - (tid & 63)) * 16), 16, 0, 0);
      }
      // the tail of every row (< 16 bytes, up to 4 dwords) through registers
      const int ndw = (Gs.w + 3) >> 2, d0 = 4 * nfull, ntail = ndw - d0;   // the last dword may read up to 3 bytes of row padding / next row: inside the plane
      const bool lastRowPartial = (Gs.w & 3) != 0;
      for (int idx = tid; idx < ntail * nsrc; idx += 256) {
        const int r = idx / ntail, d = d0 + (idx - r * ntail);
        const uint8_t *rowp = src0 + mul24((uint32_t)r, (uint32_t)spitch);
        uint32_t v;
        if (lastRowPartial && d == ndw - 1 && syFirst + r == Gs.h - 1 && spitch < 4 * ndw) {
          v = 0;  // very last bytes of the plane: do not read past the allocation
          for (int b = 0; 4 * d + b < Gs.w; b++) v |= (uint32_t)rowp[4 * d + b] << (8 * b);
        } else {
          v = *reinterpret_cast<const uint32_t *>(rowp + 4 * d);
        }
        *reinterpret_cast<uint32_t *>(sRows + mul24((uint32_t)r, (uint32_t)smemRowBytes) + 4 * d) = v;
      }
    } else {
      const float inv_w = 1.0f / (float)Gs.w;
      for (int idx = tid; idx < Gs.w * nsrc; idx += 256) {
        const int r = (int)(((float)idx + 0.5f) * inv_w), c = idx - (int)mul24((uint32_t)r, (uint32_t)Gs.w);
        sRows[mul24((uint32_t)r, (uint32_t)smemRowBytes) + c] = src0[mul24((uint32_t)r, (uint32_t)spitch) + c];
      }
    }
    RSTAMP(0);
    __syncthreads();   // the source rows and the row records have landed
    RSTAMP(1);
    // Pass 1: T[r][c] = (S[r][sx] * a0 + S[r][sx + 1] * a1) >> 4, at most 255 * 2048 / 16 = 32640: 16 bits.  Thread = two neighbouring
    // output columns, loop over the staged source rows.  Per row ONE aligned 8-byte window [base, base + 8), base = sx_A & ~3, holds all
    // four source bytes (sx_B - sx_A <= 3: the host takes this form for horizontal scale factors below 3 only): v_perm_b32 picks each
    // column's byte pair out of it as two 16-bit halves, v_dot2_u32_u16 multiplies by the column's coefficient pair - pre-scaled by 16
    // (a << 4 <= 2^15 still fits its half), which moves the >> 4 to a byte boundary: the product's bytes 1..2 are T - and a third
    // v_perm_b32 packs the two T values into one 32-bit store: five vector instructions per row for two columns, and no byte access
    // that straddles a dword (the straightforward byte-pair read compiles to an unaligned ds_read_u16, which the LDS serialises:
    // measured 25 cycles per LDS instruction, 3x the whole kernel's time).
    // Column sx + 1 = w exists in the LDS rows (they are padded to 16-byte chunks) and is only ever read with weight a1 = 0 (the table
    // clamps sx to w - 1 with fx = 0 there); the window's other bytes may be anything, they are never selected.
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    auto dot2 = [](uint32_t pix, uint32_t coef) -> uint32_t {
      u16x2 x, y;
      __builtin_memcpy(&x, &pix, 4); __builtin_memcpy(&y, &coef, 4);
      return __builtin_amdgcn_udot2(x, y, 0u, false);
    };
    int trip = 0;
    for (int p = tid; 2 * p < wq; p += 256, trip++) {
      const int4 xt = trip == 0 ? xtPre[0] : trip == 1 ? xtPre[1] : xtab4[p];     // {sx_A, coef_A, sx_B, coef_B}
      const uint32_t base = (uint32_t)xt.x & ~3u, oA = (uint32_t)xt.x & 3u, oB = (uint32_t)xt.z - base;
      const uint32_t selA = 0x0c000c00u | oA | ((oA + 1u) << 16), selB = 0x0c000c00u | oB | ((oB + 1u) << 16);
      const uint32_t kA = (uint32_t)xt.y << 4, kB = (uint32_t)xt.w << 4;
      const uint8_t *sp = sRows + base;
      uint8_t *tp = sT + 4 * p;
      // four rows per trip, all loads first: the compiler may not move an LDS load over an LDS store (T and the staged rows could alias
      // for all it knows), and one load -> store chain per row is one LDS latency per row.  The row addresses run (sp, tp advance by
      // four rows per trip, the rows of a trip lie at loop-invariant offsets from them), and the trips are nsrc / 4 full ones with no
      // test on the row count, then one tail trip of nsrc % 4 rows: the scalar unit is left with the trip counter.
      // The two running addresses are LDS byte addresses in one register each, opaque to the compiler: left to itself it keeps them
      // without the stage's constant offset in the LDS and adds that offset again for every row of every trip.
      typedef __attribute__((address_space(3))) const uint32_t lds_cu32;
      typedef __attribute__((address_space(3))) uint32_t lds_u32;
      uint32_t sa = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const uint8_t *)sp;
      uint32_t ta = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t *)tp;
      asm("" : "+v"(sa), "+v"(ta));
      auto rows4 = [&](uint32_t s, uint32_t t, int n) {   // n = 4 in the full trips (a constant there), 1 .. 3 in the tail
        uint32_t lo[4], hi[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          lds_cu32 *q = (lds_cu32 *)(uintptr_t)(s + (uint32_t)(min(k, n - 1) * smemRowBytes));
          lo[k] = q[0]; hi[k] = q[1];
        }
#pragma unroll
        for (int k = 0; k < 4; k++)
          if (k < n) {
            const uint32_t vA = dot2(__builtin_amdgcn_perm(hi[k], lo[k], selA), kA), vB = dot2(__builtin_amdgcn_perm(hi[k], lo[k], selB), kB);
            *(lds_u32 *)(uintptr_t)(t + (uint32_t)(k * tPitch)) = __builtin_amdgcn_perm(vB, vA, 0x06050201u);
          }
      };
      for (int i = nsrc >> 2; i > 0; i--, sa += 4 * smemRowBytes, ta += 4 * tPitch) rows4(sa, ta, 4);
      if (nsrc & 3) rows4(sa, ta, nsrc & 3);
    }
    __syncthreads();
    // Pass 2: 32 threads per output row, eight rows at a time, each 4 consecutive output pixels per trip: everything that
    // depends on the row alone is read once, a trip is two 8-byte LDS loads, the arithmetic and one 32-bit store.  No saturate_cast
    // needed: the coefficients are non-negative and each pair sums to 2048, so v is a convex combination of four bytes, rounded
    // down-ish: always inside [0, 255].
    // A row is G.w / 4 whole quads and, for a width that is no multiple of 4, one more of G.w % 4 bytes.  The 32 lanes of a row take
    // 32 whole quads per trip for (G.w / 4) / 32 trips - a count that is the same for every lane, so the loop is a scalar counter
    // and three running addresses, with no lane mask and no test on the column - and then one last trip, in which the lanes below
    // (G.w / 4) % 32 store a whole quad and the next lane the row's tail bytes.
    auto quad = [](const uint8_t *T0q, const uint8_t *T1q, uint32_t b0, uint32_t b1) -> uint32_t {
      const uint2 t0 = *reinterpret_cast<const uint2 *>(T0q), t1 = *reinterpret_cast<const uint2 *>(T1q);
      const uint32_t u0[4] = {t0.x & 0xffffu, t0.x >> 16, t0.y & 0xffffu, t0.y >> 16};
      const uint32_t u1[4] = {t1.x & 0xffffu, t1.x >> 16, t1.y & 0xffffu, t1.y >> 16};
      uint32_t packed = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t v = ((mul24_vv(b0, u0[j]) >> 16) + (mul24_vv(b1, u1[j]) >> 16) + 2) >> 2;
        packed |= v << (8 * j);
      }
      return packed;
    };
    const int nfq = G.w >> 2, lx = tid & 31, remq = nfq & 31, tailBytes = G.w & 3;
    for (int ry = tid >> 5; ry < nrows; ry += 8) {
      const uint4 rec = sRowRec[ry];
      const uint32_t b0 = rec.z & 0xffffu, b1 = rec.z >> 16;
      const uint8_t *T0 = sT + rec.x + 8 * lx, *T1 = sT + rec.y + 8 * lx;
      uint8_t *dst = dstplane + rec.w + 4 * lx;
      for (int n = nfq >> 5; n > 0; n--, T0 += 8 * 32, T1 += 8 * 32, dst += 4 * 32) *reinterpret_cast<uint32_t *>(dst) = quad(T0, T1, b0, b1);
      const bool whole = lx < remq;
      if (whole || (lx == remq && tailBytes)) {   // the arithmetic once for both kinds of lane
        const uint32_t packed = quad(T0, T1, b0, b1);
        if (whole) *reinterpret_cast<uint32_t *>(dst) = packed;
        else for (int j = 0; j < tailBytes; j++) dst[j] = (uint8_t)(packed >> (8 * j));
      }
    }
    RSTAMP(2);
    return;
  }

  // One-pass form: the x table in LDS, the four source bytes of every output pixel straight from global memory.
  const int dy0 = rowTile * G.resizeRows;
  const int nrows = min(G.resizeRows, G.h - dy0);
  // the tile's y-coefficients go through LDS: the row code below then has no global load in front of it
  __shared__ int2 sY[RESIZE_ROWS_MAX];
  if (tid < nrows) sY[tid] = P.ytab[G.ytabBase + dy0 + tid];
  int2 *sX = ResizeCarve::of(0, 0, 0, wq).xtab.in(smem_rs);
  for (int i = tid; i < wq; i += 256) sX[i] = P.xtab[G.xtabBase + i];
  __syncthreads();
  // q / qw in float: (q + 0.5) / qw is at least 0.5 / qw >= 2^-11 away from an integer, the product's rounding error is
  // below 2^-19 for q < 8 * 1024, so truncation gives the exact quotient (four full-rate operations)
  const float inv_qw = 1.0f / (float)qw;
  for (int q = tid; q < qw * nrows; q += 256) {
    const int ry = (int)(((float)q + 0.5f) * inv_qw), dx0 = (q - (int)mul24((uint32_t)ry, (uint32_t)qw)) * 4, dy = dy0 + ry;
    const int2 yt = sY[ry];
    const int sy0 = min(max(yt.x, 0), Gs.h - 1), sy1 = min(max(yt.x + 1, 0), Gs.h - 1);
    const int b0 = yt.y & 0xffff, b1 = (yt.y >> 16) & 0xffff;
    const uint8_t *S0 = src + mul24((uint32_t)sy0, (uint32_t)spitch), *S1 = src + mul24((uint32_t)sy1, (uint32_t)spitch);
    uint32_t packed = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int2 xt = sX[dx0 + j];            // columns past the row end repeat the last one (padded table); only [0, w) is stored
      const int sx = xt.x, sx1 = min(sx + 1, Gs.w - 1);
      const int a0 = xt.y & 0xffff, a1 = (xt.y >> 16) & 0xffff;
      const int r0 = S0[sx] * a0 + S0[sx1] * a1;
      const int r1 = S1[sx] * a0 + S1[sx1] * a1;
      const int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
      packed |= (uint32_t)v << (8 * j);
    }
    uint8_t *dst = dstplane + mul24((uint32_t)dy, (uint32_t)G.pitch);
    if (dx0 + 3 < G.w) *reinterpret_cast<uint32_t *>(dst + dx0) = packed;
    else for (int j = 0; j < 4 && dx0 + j < G.w; j++) dst[dx0 + j] = (uint8_t)(packed >> (8 * j));
  }
  RSTAMP(2);   // (the one-pass form stages no tile: the end only)
}

// ------------------------------------------------------------------------------------------------------------
// K1, single-frame form.  A frame on its own is latency: seven dependent k_resize launches of a few microseconds each cost more
// in launch-to-launch gaps than in work.  Here ONE launch makes every level: a workgroup owns a 32x32 tile of level L and
// recomputes, in LDS, the rectangles of levels 1..L-1 that tile depends on (sizes grow 1.2x per level down: 141x141 of level 0
// for a level-7 tile), each from the one below with exactly k_resize's arithmetic on exactly its table entries - a level's pixel
// is the same function of the same bytes whoever computes it, so the planes are byte-identical.  About 10x the arithmetic of
// the level-by-level form, on a chip that a single frame leaves empty; batches keep k_resize.
// ------------------------------------------------------------------------------------------------------------
// Dynamic LDS: the two level buffers (even / odd levels; FrameParams::chainBuf0 / chainBuf1 bytes, multiples of 16), then per level
// 1..L the x entries of rect[l] and its y entries - `tab` entries for the tile that has most (the host's count; the kernel, which only
// needs where the table starts, passes 0).
struct ChainCarve {
  LdsRegion<uint8_t> buf0, buf1;
  LdsRegion<int2> tab;
  int bytes;
  __host__ __device__ static constexpr ChainCarve of(int buf0, int buf1, int tab) {
    LdsCarver c;
    ChainCarve r{c.take<uint8_t>(buf0, 16), c.take<uint8_t>(buf1, 16), c.take<int2>(tab), 0};
    r.bytes = c.at;
    return r;
  }
};
#define CHAIN_LDS_MAX (64 * 1024)   // what a kernel gets unasked, and two workgroups per CU; configurations beyond it keep the level-by-level form
__global__ __launch_bounds__(CHAIN_NT) void k_pyramid_chain(FrameParams P) {
  extern __shared__ __align__(16) uint8_t smem_ch[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  constexpr int NW = CHAIN_NT / 64;
  const int ntile = (int)gridDim.x / P.nframes;
  const int frame = (int)blockIdx.x / ntile, tile = (int)blockIdx.x - frame * ntile;
  __shared__ ChainTile T;   // indexed by level at run time: LDS, not registers
  static_assert(sizeof(ChainTile) % 4 == 0 && sizeof(ChainTile) / 4 <= CHAIN_NT, "one dword per thread");
  if (tid < (int)(sizeof(ChainTile) / 4)) reinterpret_cast<uint32_t *>(&T)[tid] = reinterpret_cast<const uint32_t *>(&P.chain[tile])[tid];
  __syncthreads();
  const int L = T.level;
  const auto lds = ChainCarve::of(P.chainBuf0, P.chainBuf1, 0);
  uint8_t *buf[2] = {lds.buf0.in(smem_ch), lds.buf1.in(smem_ch)};
  int2 *sTab = lds.tab.in(smem_ch);
  // table slices of every stage, one memory latency for all of them
  {
    int off = 0;
    for (int l = 1; l <= L; l++) {
      const LevelGeom &G = P.geom[l];
      for (int i = tid; i < T.w[l] + T.h[l]; i += CHAIN_NT)
        sTab[off + i] = i < T.w[l] ? P.xtab[G.xtabBase + T.x[l] + i] : P.ytab[G.ytabBase + T.y[l] + (i - T.w[l])];
      off += T.w[l] + T.h[l];
    }
  }
  // rect[0] of the caller's image -> buffer 0 (rows by wavefront, columns by lane)
  {
    const uint8_t *img = P.img0 + (size_t)frame * P.img0_frame_stride + (size_t)T.y[0] * P.img0_stride + T.x[0];
    const int rw = T.w[0], rh = T.h[0];
    for (int r = wid; r < rh; r += NW)
      for (int c = lane; c < rw; c += 64) buf[0][r * rw + c] = img[(size_t)r * P.img0_stride + c];
  }
  __syncthreads();
  int toff = 0;
  for (int l = 1; l <= L; l++) {
    const LevelGeom &G = P.geom[l];
    const LevelGeom &Gs = P.geom[l - 1];
    const int rw = T.w[l], rh = T.h[l], sw = T.w[l - 1], sx0 = T.x[l - 1], sy0 = T.y[l - 1];
    const uint8_t *S = buf[(l - 1) & 1];
    uint8_t *D = buf[l & 1];
    const int2 *sX = sTab + toff, *sY = sX + rw;
    toff += rw + rh;
    uint8_t *plane = P.pyr + (size_t)frame * P.pyr_fs + G.off + (size_t)T.y[l] * G.pitch + T.x[l];
    const float inv_rw = 1.0f / (float)rw;
    for (int idx = tid; idx < rw * rh; idx += CHAIN_NT) {       // idx < 2^14: (idx + 0.5) / rw truncates to the exact quotient (see k_resize)
      const int ry = (int)(((float)idx + 0.5f) * inv_rw), rx = idx - ry * rw;
      const int2 xt = sX[rx], yt = sY[ry];
      const int sx = xt.x, sx1 = min(sx + 1, Gs.w - 1);
      const int sya = min(max(yt.x, 0), Gs.h - 1), syb = min(max(yt.x + 1, 0), Gs.h - 1);
      const int a0 = xt.y & 0xffff, a1 = (xt.y >> 16) & 0xffff, b0 = yt.y & 0xffff, b1 = (yt.y >> 16) & 0xffff;
      const uint8_t *S0 = S + (sya - sy0) * sw - sx0, *S1 = S + (syb - sy0) * sw - sx0;
      const int r0 = S0[sx] * a0 + S0[sx1] * a1;
      const int r1 = S1[sx] * a0 + S1[sx1] * a1;
      const int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
      if (l == L) plane[(size_t)ry * G.pitch + rx] = (uint8_t)v;
      else D[idx] = (uint8_t)v;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------
// K2: FAST-9/16 per cell (ORBextractor.cc:787-854 + cv::FAST).
//
// Threshold-free formulation.  For a pixel with centre v and circle c_k let
//   S = max( max_arcs min_k (v - c_k), max_arcs min_k (c_k - v) )   over the 16 arcs of 9 contiguous pixels.
// Then "corner at threshold t"  <=>  S > t, and cornerScore = S - 1 for every corner, independent of t.
// A corner survives cv::FAST's 3x3 NMS iff its S is strictly greater than the S of its 8 neighbours inside the
// same cell (neighbours outside the cell's detection interior count as 0), again independent of t.  So one pass
// gives the keypoints for iniThFAST and, if that set is empty, for minThFAST (decided per cell, after NMS).
//
// One 256-thread workgroup per group of up to 2 x 2 cells, one wavefront per cell: tile (<=76x80 B) and score plane in LDS,
// wave ballots for the raster-order compaction.  Output: per-cell slot list, packed (response<<24 | y<<12 | x) in
// detection-rectangle coordinates, raster order inside the cell.
// ------------------------------------------------------------------------------------------------------------
// number of set bits of a wave ballot below this lane (v_mbcnt_lo / v_mbcnt_hi)
__device__ __forceinline__ int lane_rank(unsigned long long b) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}
// fast_score_S: orb_fast_score.h (one host/device definition)

// Necessary condition for "corner at threshold t" on the 4 compass pixels (k = 0, 4, 8, 12): every arc of 9 contiguous
// circle pixels contains two ADJACENT compass pixels, so two adjacent ones must both be darker than v-t or both
// brighter than v+t.  Pixels that fail it at minThFAST have S <= minThFAST and can never be emitted nor suppress a
// neighbour, so their score is left at 0 and the 16-pixel score is only evaluated for the survivors.
__device__ __forceinline__ int fast_compass_sign(const uint8_t *c, int t) {  // negative <=> the pixel passes
  constexpr int Pt = FAST_TILE_PITCH;
  const int v = c[0];
  const uint16_t p0 = c[3 * Pt], p4 = c[3], p8 = c[-3 * Pt], p12 = c[-3];
  // "two ADJACENT compass pixels both darker than v - t": (dark0 | dark8) & (dark4 | dark12), and dark_a | dark_b is
  // min(a, b) < v - t: the whole dark test is max(min(p0, p8), min(p4, p12)) < v - t, the bright one
  // min(max(p0, p8), max(p4, p12)) > v + t.  16-bit min / max issue at the full rate on gfx950 (the 32-bit ones at half,
  // profiles/valu_calib.json); the two comparisons are sign bits of differences, so the caller's ballot is one compare.
  const int D = (int)(uint16_t)max((uint16_t)min(p0, p8), (uint16_t)min(p4, p12));
  const int B = (int)(uint16_t)min((uint16_t)max(p0, p8), (uint16_t)max(p4, p12));
  return (D - (v - t)) | ((v + t) - B);
}

#ifndef FAST_NT
#define FAST_NT 256
#endif
#define FAST_QUEUE 128   // per-wavefront ring of pre-test survivors waiting for the 16-pixel score; a row step adds at most 64 to at most 63
#ifndef FAST_LIST
#define FAST_LIST 384    // per-wavefront list of a detection's corners (S > t) for the NMS; a cell with more takes the full-cell walk
#endif
static_assert(FAST_NT == 4 * WAVE, "k_fast gives each cell of a 2 x 2 group a wavefront of its own");
static_assert(FAST_QUEUE >= 2 * WAVE - 1 && (FAST_QUEUE & (FAST_QUEUE - 1)) == 0, "the queue is looked at after every row step; its indices wrap by a mask");
static_assert(FAST_LIST % WAVE == 0, "pass 3 reads the corner list 64 entries at a time, all inside the list");
static_assert((FAST_TILE_ROWS * FAST_TILE_PITCH) % 16 == 0, "the score plane is cleared in 16-byte stores");
static_assert(FAST_TILE_ROWS * FAST_TILE_PITCH <= 65536, "queue entries are 16-bit tile offsets");
// Diagnostic builds (-DFAST_STAMPS, tools/fast_stamps.py): cycles per section, thread 0 of every workgroup (wavefront 0's cell), as
// [workgroup][8] cycle deltas in g_fast_stamps (above)
#ifdef FAST_STAMPS
#define FSTAMP(i) do { const long long t_ = __builtin_readcyclecounter(); if (threadIdx.x == 0 && g_fast_stamps) g_fast_stamps[(size_t)blockIdx.x * 8 + (i)] = (unsigned int)(t_ - ft0); ft0 = t_; } while (0)
#else
#define FSTAMP(i) do {} while (0)
#endif
// LDS written by some lanes of a wavefront and read by other lanes of the SAME wavefront: the hardware executes one
// wavefront's LDS instructions in order, so only the compiler has to be kept from moving the accesses across each other.
__device__ __forceinline__ void wave_lds_order() {
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}
__global__ __launch_bounds__(FAST_NT) void k_fast(FrameParams P) {
#ifdef FAST_STAMPS
  long long ft0 = __builtin_readcyclecounter();
#endif
  __shared__ __align__(16) uint8_t sTile[FAST_TILE_ROWS * FAST_TILE_PITCH];
  __shared__ __align__(16) uint8_t sS[FAST_TILE_ROWS * FAST_TILE_PITCH];   // the group's score plane, indexed like the tile
  __shared__ uint16_t sQ[4 * FAST_QUEUE];
  __shared__ uint16_t sL[4 * FAST_LIST];   // per-wavefront corner lists (tile offsets, raster order)
  const int tid = threadIdx.x, lane = tid & 63;
  // A workgroup takes a GROUP of up to 2 x 2 neighbouring cells: their windows overlap by six pixels and the 80-byte tile rows carry
  // the right-hand neighbour's columns, so one staged tile - one HBM round trip, one set of address arithmetic - serves four
  // cells.  Wavefront w then detects cell w of the group on its own, with no workgroup barrier after the tile has landed: the
  // reference decides iniThFAST / minThFAST per cell (ORBextractor.cc:820-828), and a cell that needs the second detection
  // holds up no other.
  int groupId, frame;
  xcd_map(P.totalGroups, P.magicGroups, P.nframes, frame, groupId);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform by construction; tells the compiler so (scalar control flow)
  // The group's record (orbx_configure, layout in orb_common.h): the group part and this wavefront's cell part, two scalar loads
  // that depend on the kernel arguments alone and are in flight together, in front of the tile's DMA.  The table is written by
  // the host only, never by a kernel: read through the constant address space the loads stay scalar loads wherever their
  // values are used, and nothing is fetched behind the barrier, where no other memory traffic would hide the round trip.
  typedef uint32_t rec8_t __attribute__((ext_vector_type(8)));
  typedef uint32_t rec4_t __attribute__((ext_vector_type(4)));
  const __attribute__((address_space(4))) uint32_t *rec =
      (const __attribute__((address_space(4))) uint32_t *)P.fastRecs + (size_t)groupId * FAST_REC_WORDS;
  const rec8_t gr = *reinterpret_cast<const __attribute__((address_space(4))) rec8_t *>(rec);
  const rec4_t cr = *reinterpret_cast<const __attribute__((address_space(4))) rec4_t *>(rec + FAST_REC_GROUP_WORDS + FAST_REC_CELL_WORDS * wave);
  const int tileX = (int)(gr[0] & 0xffffu), tileY = (int)(gr[0] >> 16);
  const int gtw = (int)(gr[1] & 0xffu), gth = (int)((gr[1] >> 8) & 0xffu), level = (int)((gr[1] >> 16) & 0xffu);
  const bool gvalid = (gr[1] >> 24) != 0u;
  const int ax = tileX & ~3;                          // tile column 0 = image column ax, tile row 0 = image row tileY
  if (gvalid) {
    int pitch;
    const uint8_t *img;
    if (level == 0) { pitch = (int)P.img0_stride; img = P.img0 + (size_t)frame * P.img0_frame_stride; }   // the caller's image: not in the record
    else { pitch = (int)gr[3]; img = P.pyr + (size_t)frame * P.pyr_fs + (((size_t)gr[5] << 32) | gr[4]); }
    // ---- tile -> LDS.  Aligned path: the columns [tileX & ~3, ...) of the group's rows.
    const bool aligned = ((((uintptr_t)img) | (uintptr_t)pitch) & 3u) == 0;
    if (aligned) {
      // LDS-DMA: one global_load_lds_dwordx4 per lane moves 16 bytes straight into the tile (no register, no ds_write); the
      // tile is lane-linear, chunk idx = 5 * row + chunk-in-row.  Chunks past the group's columns read the bytes that follow
      // in the plane (a cell window ends >= 13 rows above the plane's last row, so they exist) and are never looked at.
      // Index arithmetic in 24-bit multiplies (full rate): idx / 5 as (idx * 13108) >> 16, exact below 5 * FAST_TILE_ROWS.
      const int nch = 5 * gth;
      const uint8_t *img0 = img + mul24((uint32_t)tileY, (uint32_t)pitch) + ax;
      for (int idx = tid; idx < nch; idx += FAST_NT) {
        const uint32_t r = mul24((uint32_t)idx, 13108u) >> 16, c = (uint32_t)idx - 5u * r;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(img0 + (mul24(r, (uint32_t)pitch) + 16u * c)),
                                         (__attribute__((address_space(3))) void *)&sTile[idx * 16], 16, 0, 0);
      }
    } else {
      const uint32_t magic = (1u << 20) / (uint32_t)gtw + 1u;
      const int ox0 = tileX - ax;
      const uint8_t *img0 = img + mul24((uint32_t)tileY, (uint32_t)pitch) + tileX;
      for (int idx = tid; idx < gtw * gth; idx += FAST_NT) {
        const uint32_t r = mul24((uint32_t)idx, magic) >> 20, cc = (uint32_t)idx - mul24(r, (uint32_t)gtw);
        sTile[r * FAST_TILE_PITCH + ox0 + cc] = img0[mul24(r, (uint32_t)pitch) + cc];
      }
    }
  }
  FSTAMP(3);
  // Score 0 everywhere, while the LDS-DMA is in flight: a pixel the pre-test never passes keeps it.  S does not depend on the
  // threshold and the minThFAST survivors include the iniThFAST ones, so a second detection rewrites the same values.
  for (int i = tid; i < FAST_TILE_ROWS * FAST_TILE_PITCH / 16; i += FAST_NT) reinterpret_cast<uint4 *>(sS)[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();   // the only workgroup barrier: the tile has landed (its fence waits for the LDS-DMA), the plane is clear
  FSTAMP(0);
  if (wave >= (int)gr[2]) return;                               // groups at the right / bottom edge of a level: fewer cells
  // this wavefront's cell (ORBextractor.cc:787-803), from the record: registers, no load
  const int iniX = (int)(cr[0] & 0xffffu), iniY = (int)(cr[0] >> 16);
  const int tw = (int)(cr[1] & 0xffu), th = (int)((cr[1] >> 8) & 0xffu), cw = tw - 6, ch = th - 6;
  const uint32_t baseX = (uint32_t)(iniX - ORB_MIN_BORDER), baseY = (uint32_t)(iniY - ORB_MIN_BORDER);  // cj * wCell, ci * hCell
  const uint32_t cellCap = gr[6];
  uint32_t *cellCnt = P.cellCnt + (size_t)frame * P.cell_fs + cr[3];
  if (!(cr[1] >> 24)) {  // cell outside the detection rectangle
    if (lane == 0) *cellCnt = 0;
    return;
  }
  // The reference runs cv::FAST on the cell at iniThFAST and, only if that returns nothing, again at minThFAST
  // (ORBextractor.cc:820-828).  The score S is threshold-free, so "FAST at threshold t with non-maximum suppression" is: S > t
  // and S strictly above the S of the 8 neighbours inside the cell (a neighbour that is no corner at t has S <= t < S and can be
  // left at 0; one outside the cell counts as 0, as on the cell's own Mat).  The kernel follows the same order - detect at
  // iniThFAST, and again at minThFAST when the cell stayed empty - because the compass pre-test at the higher threshold passes
  // far fewer pixels to the 16-pixel score (synthetic EuRoC frames: 81-125 per 30x30 cell instead of 227-360 at minThFAST 7,
  // and 2 % of the cells need the second detection).
  // Lanes form rows of 32 (cells up to 32 interior columns, the usual 30) or 64 and step down the cell, so the per-pixel index
  // arithmetic is one add; a step visits its pixels in raster order.  Cell interiors are disjoint, so the four wavefronts share
  // one score plane; a wavefront reads the plane only inside its own cell.
  const int xsh = cw <= 32 ? 5 : 6;
  const int px = lane & ((1 << xsh) - 1), sub = lane >> xsh, rpi = 64 >> xsh;   // rows per step: 2 or 1
  const bool xin = px < cw;
  const int off0 = (iniY - tileY + 3 + sub) * FAST_TILE_PITCH + (iniX - ax) + 3 + px;   // tile offset of this lane's first pixel
  // validity as a sign bit: row - ch is negative inside the cell; columns outside the cell start from a value that stays positive
  const int yr0 = xin ? sub - ch : 0x40000000;
  const uint32_t yx0 = ((baseY + (uint32_t)sub + 3u) << 12) | (baseX + (uint32_t)px + 3u);   // packed output coordinates
  uint16_t *q = sQ + wave * FAST_QUEUE;
  uint16_t *list = sL + wave * FAST_LIST;
  const int base00 = (iniY - tileY + 3) * FAST_TILE_PITCH + (iniX - ax) + 3;   // tile offset of the interior's first pixel
  uint32_t *slots = P.slots + (size_t)frame * P.slot_fs + cr[2];
  int nkept = 0;
  int t = P.iniTh;
#ifdef FAST_STAMPS
  asm volatile("" ::"v"(off0), "v"(yr0), "v"(yx0), "s"(cellCap), "v"(slots), "v"(cellCnt));   // section 4 ends once all the cell's values are there
#endif
  FSTAMP(4);
  for (int detection = 0;; detection++) {
    // ---- passes 1 + 2: compass pre-test at t; survivors join the wavefront's queue as tile offsets, and every time the queue
    // holds a full wavefront's worth, 64 of them get the 16-pixel score (a second detection recomputes the first one's
    // entries: same values).  Lanes whose score is above t append their offset to the corner list: the queue is filled and
    // drained in raster order, so the list is in raster order too.  A second detection starts a new list.
    const int tt = max(t, 1);   // S > t, and S >= 2: the response S - 1 must be positive
    // queue head and tail (running counts, reduced mod FAST_QUEUE where they index) and the list's length: wave-uniform.  The head is
    // kept as qfull = head + WAVE, the tail at which a full wavefront's worth is waiting: the look at the queue is one compare.
    int qfull = WAVE, qt = 0, nl = 0;
    auto score = [&](bool act) {
      const int o = act ? (int)q[(qfull - WAVE + lane) & (FAST_QUEUE - 1)] : base00;   // idle lanes of the tail: a pixel of the cell
      const int S = fast_score_S(&sTile[o]);
      if (act) sS[o] = (uint8_t)S;
      const bool c = act && S > tt;
      const unsigned long long bc = __builtin_amdgcn_ballot_w64(c);
      const int li = nl + lane_rank(bc);
      if (c && li < FAST_LIST) list[li] = (uint16_t)o;
      nl += __popcll(bc);
    };
    // Two row steps per trip, specialised on the rows per step: the second step's pixels lie at a constant distance from the
    // first one's, so its five byte reads are the first step's addresses with another immediate and all ten are in flight
    // before the first wait; one loop counter and one advance of off / yr serve both steps.  A step past the cell's last row (an
    // odd number of steps) is masked like any row outside the cell: yr + RPI is not negative there.  The queue is still looked at
    // after each step (one compare and a branch that is rarely taken): looked at once per pair it has to hold 63 + 128 entries, and
    // the 1 KB of LDS that costs per workgroup lost more beside the other pipelines than the two instructions cost.
    auto drain = [&]() {
      wave_lds_order();
      score(true);
      qfull += WAVE;
      wave_lds_order();   // these queue entries are free again
    };
    auto pretest = [&](auto rpiC) {
      constexpr int RPI = decltype(rpiC)::value, STEP = RPI * FAST_TILE_PITCH;
      int off = off0, yr = yr0;
      for (int y0 = 0; y0 < ch; y0 += 2 * RPI, off += 2 * STEP, yr += 2 * RPI) {
        // lanes outside the cell read LDS bytes that mean nothing (or zero past the allocation) and are masked out by yr
#ifdef FAST_PAD   // diagnostic builds only (tools/fast_sensitivity.sh): 16 extra instructions of one class per pass-1 trip, results unused
        {
          int pad0 = off, pad1 = yr;
#if FAST_PAD == 1   // full-rate VALU
          asm volatile("v_add_u32 %0, %0, %1\nv_add_u32 %1, %1, %0\nv_add_u32 %0, %0, %1\nv_add_u32 %1, %1, %0\nv_add_u32 %0, %0, %1\nv_add_u32 %1, %1, %0\nv_add_u32 %0, %0, %1\nv_add_u32 %1, %1, %0\n"
                       "v_add_u32 %0, %0, %1\nv_add_u32 %1, %1, %0\nv_add_u32 %0, %0, %1\nv_add_u32 %1, %1, %0\nv_add_u32 %0, %0, %1\nv_add_u32 %1, %1, %0\nv_add_u32 %0, %0, %1\nv_add_u32 %1, %1, %0\n" : "+v"(pad0), "+v"(pad1));
#elif FAST_PAD == 2   // half-rate VALU
          asm volatile("v_pk_max_i16 %0, %0, %1\nv_pk_max_i16 %1, %1, %0\nv_pk_max_i16 %0, %0, %1\nv_pk_max_i16 %1, %1, %0\nv_pk_max_i16 %0, %0, %1\nv_pk_max_i16 %1, %1, %0\nv_pk_max_i16 %0, %0, %1\nv_pk_max_i16 %1, %1, %0\n"
                       "v_pk_max_i16 %0, %0, %1\nv_pk_max_i16 %1, %1, %0\nv_pk_max_i16 %0, %0, %1\nv_pk_max_i16 %1, %1, %0\nv_pk_max_i16 %0, %0, %1\nv_pk_max_i16 %1, %1, %0\nv_pk_max_i16 %0, %0, %1\nv_pk_max_i16 %1, %1, %0\n" : "+v"(pad0), "+v"(pad1));
#elif FAST_PAD == 3   // scalar ALU
          asm volatile("s_add_u32 s40, s40, 1\ns_add_u32 s41, s41, 1\ns_add_u32 s42, s42, 1\ns_add_u32 s43, s43, 1\ns_add_u32 s40, s40, 1\ns_add_u32 s41, s41, 1\ns_add_u32 s42, s42, 1\ns_add_u32 s43, s43, 1\n"
                       "s_add_u32 s40, s40, 1\ns_add_u32 s41, s41, 1\ns_add_u32 s42, s42, 1\ns_add_u32 s43, s43, 1\ns_add_u32 s40, s40, 1\ns_add_u32 s41, s41, 1\ns_add_u32 s42, s42, 1\ns_add_u32 s43, s43, 1\n" ::: "s40", "s41", "s42", "s43", "scc");
#endif
          asm volatile("" ::"v"(pad0), "v"(pad1));
        }
#endif
        const uint8_t *c = &sTile[off];
        const bool passA = (fast_compass_sign(c, t) & yr) < 0, passB = (fast_compass_sign(c + STEP, t) & (yr + RPI)) < 0;
        const unsigned long long bA = __builtin_amdgcn_ballot_w64(passA), bB = __builtin_amdgcn_ballot_w64(passB);
        if (passA) q[(qt + lane_rank(bA)) & (FAST_QUEUE - 1)] = (uint16_t)off;
        qt += __popcll(bA);
        if (__builtin_expect(qt >= qfull, 0)) drain();
        if (passB) q[(qt + lane_rank(bB)) & (FAST_QUEUE - 1)] = (uint16_t)(off + STEP);
        qt += __popcll(bB);
        if (__builtin_expect(qt >= qfull, 0)) drain();
      }
    };
    if (xsh == 5) pretest(std::integral_constant<int, 2>());
    else pretest(std::integral_constant<int, 1>());
    wave_lds_order();
    if (qt > qfull - WAVE) score(lane < qt - (qfull - WAVE));
    wave_lds_order();   // the plane and the list are complete
    FSTAMP(1);
    // ---- pass 3: NMS + emit.  cv::FAST emits rows ascending, x ascending = the order of the corner list, so a kept corner's
    // output slot is the wavefront's running count plus its lane rank: no atomics, no sorting.
    if (nl <= FAST_LIST) {
      // 64 corners per trip: all nine plane reads issued at once, neighbours outside the cell masked to 0 by selects
      for (int i0 = 0; i0 < nl; i0 += WAVE) {
        const bool act = i0 + lane < nl;
        const int o = act ? (int)list[i0 + lane] : FAST_TILE_PITCH + 1;   // idle lanes: any offset whose 3 x 3 lies in the plane
        const uint32_t rel = (uint32_t)(o - base00);
        const int y = (int)(mul24(rel, 52429u) >> 22), x = (int)rel - y * FAST_TILE_PITCH;   // rel / 80, exact for rel < 2^18
        const uint8_t *s = &sS[o];
        const int S = s[0];
        int n0 = s[-FAST_TILE_PITCH - 1], n1 = s[-FAST_TILE_PITCH], n2 = s[-FAST_TILE_PITCH + 1], n3 = s[-1];
        int n4 = s[1], n5 = s[FAST_TILE_PITCH - 1], n6 = s[FAST_TILE_PITCH], n7 = s[FAST_TILE_PITCH + 1];
        asm("" : "+v"(n0), "+v"(n1), "+v"(n2), "+v"(n3), "+v"(n4), "+v"(n5), "+v"(n6), "+v"(n7));   // keeps the reads out of branches
        const bool l = x > 0, r = x < cw - 1, u = y > 0, d = y < ch - 1;   // neighbours outside the cell count as 0
        const int mu = u ? max(max(l ? n0 : 0, n1), r ? n2 : 0) : 0;
        const int md = d ? max(max(l ? n5 : 0, n6), r ? n7 : 0) : 0;
        const int m = max(max(l ? n3 : 0, r ? n4 : 0), max(mu, md));
        const bool keep = act && S > m;
        const unsigned long long bK = __builtin_amdgcn_ballot_w64(keep);
        const uint32_t rank = (uint32_t)nkept + (uint32_t)lane_rank(bK);
        if (keep && rank < cellCap) slots[rank] = ((uint32_t)(S - 1) << 24) | (((baseY + (uint32_t)y + 3u) << 12) | (baseX + (uint32_t)x + 3u));
        nkept += __popcll(bK);
      }
    } else {
      // more corners than the list holds (dense texture or noise): the cell's plane rows in raster order; only lanes with
      // S > t look at their neighbours.  Two row steps per trip, as in the pre-test: both plane reads first, one counter and one
      // advance for the pair; a step past the last row is masked by yr.
      int off = off0, yr = yr0;
      uint32_t yx = yx0;
      const int stepB = rpi * FAST_TILE_PITCH;
      auto walk = [&](bool cand, int S, int o, int y, uint32_t yxv) {
        bool keep = false;
        if (cand) {
          const uint8_t *s = &sS[o];
          const bool l = px > 0, r = px < cw - 1, u = y > 0, d = y < ch - 1;   // neighbours outside the cell count as 0
          const int mu = u ? max(max(l ? (int)s[-FAST_TILE_PITCH - 1] : 0, (int)s[-FAST_TILE_PITCH]), r ? (int)s[-FAST_TILE_PITCH + 1] : 0) : 0;
          const int md = d ? max(max(l ? (int)s[FAST_TILE_PITCH - 1] : 0, (int)s[FAST_TILE_PITCH]), r ? (int)s[FAST_TILE_PITCH + 1] : 0) : 0;
          const int m = max(max(l ? (int)s[-1] : 0, r ? (int)s[1] : 0), max(mu, md));
          keep = S > m;
        }
        const unsigned long long bK = __builtin_amdgcn_ballot_w64(keep);
        const uint32_t rank = (uint32_t)nkept + (uint32_t)lane_rank(bK);
        if (keep && rank < cellCap) slots[rank] = ((uint32_t)(S - 1) << 24) | yxv;
        nkept += __popcll(bK);
      };
      for (int y0 = 0; y0 < ch; y0 += 2 * rpi, off += 2 * stepB, yr += 2 * rpi, yx += (uint32_t)rpi << 13) {
        const int SA = sS[off], SB = sS[off + stepB];
        const bool candA = ((tt - SA) & yr) < 0, candB = ((tt - SB) & (yr + rpi)) < 0;
        const unsigned long long bA = __builtin_amdgcn_ballot_w64(candA), bB = __builtin_amdgcn_ballot_w64(candB);
        if (bA != 0ull) walk(candA, SA, off, y0 + sub, yx);
        if (bB != 0ull) walk(candB, SB, off + stepB, y0 + rpi + sub, yx + ((uint32_t)rpi << 12));
      }
    }
    FSTAMP(2);
    // ORBextractor.cc:825: the second detection runs only if the first returned nothing (with minThFAST >= iniThFAST it could
    // only return a subset of nothing)
    if (nkept > 0 || detection == 1 || P.minTh >= P.iniTh) break;
    t = P.minTh;
    wave_lds_order();   // pass 3 is done with the plane and the list, the queue is empty
  }
  if (lane == 0) *cellCnt = (uint32_t)min(nkept, (int)cellCap);
  FSTAMP(7);
}

// ------------------------------------------------------------------------------------------------------------
// K3: DistributeOctTree (ORBextractor.cc:479-761), one 256-thread workgroup per (frame, level).
//
// Data-parallel restatement (model + proof-by-test in tests/octree_model.py):
//  * the std::list is an array in list order; a round builds the next array with prefix sums:
//      new list = [children of the nodes processed this round, in reverse processing order, each as n4,n3,n2,n1]
//                 ++ [unprocessed nodes in their old order]            (push_front / erase semantics, :619-661)
//  * keys never move: each candidate carries the list position of its node (knode) and is re-labelled per round;
//  * full rounds process every node with >1 key in list order (:598-663); once size + 3*nToExpand > N (:671)
//    rounds process nodes by (size desc, creation order desc) = (size desc, list position asc) and stop at the
//    first prefix that reaches N nodes (:682-729) -- the cut is found with a scan over the ranked child counts;
//  * the winner of a node is max response, first in vKeys order on ties (:745-757) = smallest dense index,
//    taken with a 64-bit LDS atomicMax over (response, ~index).
// Candidates are first compacted from the per-cell slot lists into the reference's vToDistributeKeys order.
// Where the host built the code tables (P.octTab), the rounds touch no key: a key's cell at every depth down to OCT_D follows from
// its column and its row alone (DivideNode's lines depend on the node's bounds only), so one pass codes and counts the keys and the
// rounds read the child counts of a node from a pyramid of sums (model + proof-by-test in tests/octree_codes_model.py).
// ------------------------------------------------------------------------------------------------------------
#ifdef OCT_STAMPS   // diagnostic builds only (tools/octree_stamps.py): cycles per phase, thread 0 of every workgroup, summed over the rounds
#define OSTAMP(i) do { const long long t_ = __builtin_readcyclecounter(); if (threadIdx.x == 0 && g_fast_stamps) g_fast_stamps[(size_t)blockIdx.x * 8 + (i)] += (unsigned int)(t_ - ot0); ot0 = t_; } while (0)
#else
#define OSTAMP(i) do {} while (0)
#endif
struct OctNode { short ulx, urx, uly, bry; };

// k_octree's dynamic LDS for `cap` nodes: a head region of `head` bytes (FrameParams::octHead: a multiple of 16, at least the
// OCT_HEAD_PER_NODE bytes per node of the per-key rounds' child tables), OCT_BODY_PER_NODE bytes per node of node tables, the scan
// scratch of an NT-thread workgroup and, behind it, the level's cell offsets where the host keeps them in LDS (cells > 0).
// Three things lie over others.  best (the winners' 64-bit atomicMax) over chcnt: it is used after the last round.  pyr - the code
// form's counts, leaves first (OCT_PYR_OFF), with the leaf -> list position map over the leaf bins - over the whole head, and codeA /
// codeB (depth << 13 | ix << 5 | iy of a node's cell) over npos: chcnt, chpos and npos are live only while keys are re-labelled per
// round, which the code form does not do.
#define OCT_HEAD_PER_NODE 32   // chcnt + chpos
#define OCT_BODY_PER_NODE 40   // nodeA .. sflag
#define OCT_SCAN_BYTES 128     // what every launch reserves for the scan scratch (NT = 1024 uses 72 bytes of it)
struct OctreeCarve {
  LdsRegion<uint32_t> chcnt;   // 4 per node: keys per child
  LdsRegion<int32_t> chpos;    // 4 per node: list position of each child
  LdsRegion<unsigned long long> best;
  LdsRegion<uint16_t> pyr;
  LdsRegion<OctNode> nodeA, nodeB;
  LdsRegion<uint32_t> cntA, cntB;
  LdsRegion<int32_t> npos, rankOf;
  LdsRegion<uint16_t> codeA, codeB;
  LdsRegion<uint32_t> incl;    // child counts by rank -> inclusive sums
  LdsRegion<uint32_t> sflag;   // unprocessed flags -> exclusive sums
  LdsRegion<uint32_t> sw;      // scan scratch
  LdsRegion<uint32_t> cellOff; // cells + 1 offsets of the level's FAST cells
  int bytes;
  __host__ __device__ static constexpr OctreeCarve of(int cap, int head, int nt, int cells) {
    LdsCarver c;
    OctreeCarve o{};
    o.chcnt = c.take<uint32_t>(4 * cap);
    o.chpos = c.take<int32_t>(4 * cap);
    o.best = LdsCarver::over<unsigned long long>(0, cap);
    o.pyr = LdsCarver::over<uint16_t>(0, head / 2);
    c.at = head;
    o.nodeA = c.take<OctNode>(cap); o.nodeB = c.take<OctNode>(cap);
    o.cntA = c.take<uint32_t>(cap); o.cntB = c.take<uint32_t>(cap);
    o.npos = c.take<int32_t>(cap); o.rankOf = c.take<int32_t>(cap);
    o.codeA = LdsCarver::over<uint16_t>(o.npos.off, cap); o.codeB = LdsCarver::over<uint16_t>(o.codeA.end(), cap);
    o.incl = c.take<uint32_t>(cap); o.sflag = c.take<uint32_t>(cap);
    o.sw = c.take<uint32_t>(nt / 64 + 2);
    o.cellOff = c.take<uint32_t>(cells > 0 ? cells + 1 : 0);
    o.bytes = o.sw.off + OCT_SCAN_BYTES + o.cellOff.size();
    return o;
  }
};
static_assert(OctreeCarve::of(1, OCT_HEAD_PER_NODE, 256, 0).chpos.end() == OCT_HEAD_PER_NODE && OctreeCarve::of(1, OCT_HEAD_PER_NODE, 256, 0).sw.off == OCT_HEAD_PER_NODE + OCT_BODY_PER_NODE,
              "bytes per node");
static_assert(4 * (1024 / 64 + 2) <= OCT_SCAN_BYTES, "scan scratch of the widest workgroup");
// What orbx_configure admits.  The kernel's static LDS is 32 bytes.
#define OCT_LDS_MAX (ORB_LDS_LIMIT - 256)   // node tables and scan scratch: nfeatures beyond it are refused
#define OCT_CELLS_LDS_MAX (96 * 1024)       // the cell offsets join them in LDS while the launch stays within this, which leaves 64 KiB of the CU to other workgroups
#define OCT_GROWN_HEAD_MAX (32 * 1024)      // a head enlarged for the code tables (few nodes): only while the whole state stays this small

#ifndef OCT_REGKEYS
#define OCT_REGKEYS 4096   // keys of a level held in registers (the rest goes through the global cand / knode arrays)
#endif
template <int NT, bool CELLS_LDS>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(4))) void k_octree(   // four workgroups of 256 per CU, as before the code form: no more than 128 registers
FrameParams P, uint32_t *cellOffScratch) {
  extern __shared__ __align__(16) uint8_t smem[];
#ifdef OCT_STAMPS
  long long ot0 = __builtin_readcyclecounter();
#endif
  const int CAP = P.octCap;
  const auto lds = OctreeCarve::of(CAP, P.octHead, NT, 0);   // (the cell count only sizes cellOff)
  unsigned long long *best = lds.best.in(smem);
  uint32_t *chcnt = lds.chcnt.in(smem);
  int32_t *chpos = lds.chpos.in(smem);
  OctNode *nodeA = lds.nodeA.in(smem), *nodeB = lds.nodeB.in(smem);
  uint32_t *cntA = lds.cntA.in(smem), *cntB = lds.cntB.in(smem);
  int32_t *npos = lds.npos.in(smem), *rankOf = lds.rankOf.in(smem);
  uint32_t *incl = lds.incl.in(smem), *sflag = lds.sflag.in(smem), *sw = lds.sw.in(smem);
  __shared__ int shI[8];
  // Code form (P.octTab): every key is looked up once - its leaf of the depth-OCT_D split grid - and counted
  // into a leaf histogram; the counts of the coarser cells are sums, the rounds run on the nodes alone (a node knows its cell and
  // reads its children's counts), and a leaf -> list position map gives the keys their node at the end.  Bins, sums and map take
  // the place of chcnt / chpos, the nodes' cells that of npos: none of those is live while no key is re-labelled.
  uint16_t *pyr = lds.pyr.in(smem), *codeA = lds.codeA.in(smem), *codeB = lds.codeB.in(smem);
  bool codes = P.octTab != nullptr;                              // false from the round that has to split a depth-OCT_D node

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  constexpr int NW = NT / 64;
  // 1-D grid, level-major: workgroups are dealt round-robin over the 8 XCDs by block index, so frame f of every level
  // lands on XCD f % 8 (a (level, frame) 2-D grid put ALL level-0 workgroups, the long ones, on one XCD: 2.2x slower),
  // and the long level-0 workgroups are dispatched first.
  const int level = (int)(blockIdx.x / (unsigned)P.nframes), frame = (int)(blockIdx.x - (unsigned)level * (unsigned)P.nframes);
  const LevelGeom G = P.geom[level];
  int32_t *lcnt = P.lcnt + ((size_t)frame * P.nlevels + level) * 2;
  uint32_t *cand = P.cand + (size_t)frame * P.cand_fs + G.candBase;
  uint16_t *knode = P.knode + (size_t)frame * P.cand_fs + G.candBase;
  // The keys never move and every pass over them uses the same thread <-> key assignment (k = tid + j * NT), so the first 4096 keys
  // of a level - all of them on any frame seen so far (EuRoC: 600 .. 3300 per level) - live in REGISTERS: the packed candidate and its
  // node label, PER of each per thread.  The rounds then touch no memory but the node tables in LDS; the global cand / knode arrays
  // only serve keys beyond 4096 (round 2 re-read and re-wrote both arrays every round: 4.8x the kernel's algorithmic traffic, and a
  // global round trip in front of both key passes of every round).
  constexpr int PER = OCT_REGKEYS / NT, REGN = PER * NT;
  uint32_t rc[PER > 0 ? PER : 1], rk[PER > 0 ? PER : 1];
#pragma unroll
  for (int j = 0; j < PER; j++) { rc[j] = 0u; rk[j] = 0u; }
  // f(k, c, nd): k dense key index, c packed candidate, nd node label (both by reference)
  auto for_keys = [&](int n_, auto f) {
#pragma unroll
    for (int j = 0; j < PER; j++) {
      if (j * NT >= n_) break;
      const int k = tid + j * NT;
      if (k < n_) f(k, rc[j], rk[j]);
    }
    for (int k = REGN + tid; k < n_; k += NT) {
      uint32_t c = cand[k], nd = knode[k];
      f(k, c, nd);
      knode[k] = (uint16_t)nd;
    }
  };

  // ---- A. compact the per-cell slot lists into vToDistributeKeys order (cells row-major, raster inside) ----
  // Cell offsets by a workgroup scan (kept in LDS when they fit: CELLS_LDS), then one thread per candidate finds its
  // cell by bisection and copies its slot: every global access of this phase is independent of the others, so the
  // phase costs a few memory latencies instead of one per cell.
  const int ncell = G.nCols * G.nRows;
  const uint32_t *cellCnt = P.cellCnt + (size_t)frame * P.cell_fs + G.cellBase;
  uint32_t *cellOffG = cellOffScratch + (size_t)frame * P.cell_fs + G.cellBase;
  uint32_t *cellOffL = lds.cellOff.in(smem);        // ncell + 1 words behind the scan scratch (CELLS_LDS only)
  uint32_t carry = 0;
  for (int base = 0; base < ncell; base += NT) {
    int i = base + tid;
    uint32_t v = i < ncell ? cellCnt[i] : 0u;
    uint32_t inc = wave_incl_scan(v);
    if (lane == 63) sw[wid] = inc;
    __syncthreads();
    const uint32_t wsum = lane < NW ? sw[lane] : 0u;       // wave totals scanned in registers, as in lds_excl_scan
    const uint32_t wincl = wave_incl_scan(wsum);
    const uint32_t woff = (uint32_t)__builtin_amdgcn_readlane((int)(wincl - wsum), __builtin_amdgcn_readfirstlane(wid));
    const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)wincl, NW - 1);
    if (i < ncell) { if (CELLS_LDS) cellOffL[i] = carry + woff + inc - v; else cellOffG[i] = carry + woff + inc - v; }
    carry += tot;
    __syncthreads();
  }
  const int n = min((int)carry, G.candCap);
  if (tid == 0) P.candCnt[(size_t)frame * P.nlevels + level] = n;
  if (n == 0) {
    if (tid == 0) { lcnt[0] = 0; lcnt[1] = 0; }
    return;
  }
  __syncthreads();  // cell offsets visible to the whole workgroup
  {
    const uint32_t *slots = P.slots + (size_t)frame * P.slot_fs + G.slotBase;
    if (CELLS_LDS) {
      auto fetch = [&](int k) -> uint32_t {
        int lo = 0, hi = ncell - 1;                  // last cell whose offset is <= k (empty cells share offsets)
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (cellOffL[mid] <= (uint32_t)k) lo = mid; else hi = mid - 1;
        }
        return slots[(size_t)lo * G.cellCap + ((uint32_t)k - cellOffL[lo])];
      };
#pragma unroll
      for (int j = 0; j < PER; j++) {
        if (j * NT >= n) break;
        const int k = tid + j * NT;
        if (k < n) { rc[j] = fetch(k); cand[k] = rc[j]; }   // the global copy is written once and never read back (orbx_debug_candidates, stage parity tests)
      }
      for (int k = REGN + tid; k < n; k += NT) cand[k] = fetch(k);
      __syncthreads();
    } else {
      for (int cidx = wid; cidx < ncell; cidx += NW) {
        uint32_t cnt = cellCnt[cidx], off = cellOffG[cidx];
        for (uint32_t j = lane; j < cnt; j += 64)
          if (off + j < (uint32_t)n) cand[off + j] = slots[(size_t)cidx * G.cellCap + j];
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < PER; j++) {
        if (j * NT >= n) break;
        const int k = tid + j * NT;
        if (k < n) rc[j] = cand[k];
      }
    }
  }
  OSTAMP(0);

  // ---- B. root nodes (ORBextractor.cc:541-585) ----
  const int nIni = G.nIni;
  const float hX = G.hX;
  const int Hrect = G.maxBorderY - ORB_MIN_BORDER;
  if (n > 65535) codes = false;   // the counts are 16 bits wide
  if (codes) {
    // the one pass over the keys: leaf code (root and x bits from the column table, y bits from the row table) and leaf histogram
    uint32_t *bins = reinterpret_cast<uint32_t *>(pyr);   // the carve's pyr, its leaf bins two to a word; no count passes n <= 65535
    for (int i = tid; i < (nIni << (2 * OCT_D - 1)); i += NT) bins[i] = 0u;
    if (tid == 0) shI[5] = 0;
    __syncthreads();
    const uint8_t *tabX = P.octTab + G.octTabX, *tabY = P.octTab + G.octTabY;
    const int Wrect = G.maxBorderX - ORB_MIN_BORDER;
    for_keys(n, [&](int, uint32_t &c, uint32_t &nd) {
      const int x = min((int)(c & 0xfff), Wrect), y = min((int)((c >> 12) & 0xfff), Hrect);
      nd = ((uint32_t)tabX[x] << OCT_D) | (uint32_t)tabY[y];
      atomicAdd(&bins[nd >> 1], 1u << ((nd & 1u) << 4));
    });
    __syncthreads();
    // counts of depths OCT_D - 1 .. 0: a cell's four children are two adjacent pairs of the finer grid
#pragma unroll
    for (int d = OCT_D - 1; d >= 0; d--) {
      const uint16_t *fine = pyr + OCT_PYR_OFF(nIni, d + 1);
      uint16_t *coarse = pyr + OCT_PYR_OFF(nIni, d);
      for (int e = tid; e < (nIni << (2 * d)); e += NT) {
        const int ix = e >> d, iy = e & ((1 << d) - 1);
        const uint32_t w0 = *reinterpret_cast<const uint32_t *>(fine + ((2 * ix) << (d + 1)) + 2 * iy);
        const uint32_t w1 = *reinterpret_cast<const uint32_t *>(fine + ((2 * ix + 1) << (d + 1)) + 2 * iy);
        coarse[e] = (uint16_t)((w0 & 0xffffu) + (w0 >> 16) + (w1 & 0xffffu) + (w1 >> 16));
      }
      __syncthreads();
    }
  } else {
  for (int i = tid; i < nIni; i += NT) chcnt[i] = 0;
  __syncthreads();
  for_keys(n, [&](int, uint32_t &c, uint32_t &nd) {
    int r = (int)((float)(c & 0xfff) / hX);  // vpIniNodes[kp.pt.x/hX], :567
    r = min(max(r, 0), nIni - 1);
    nd = (uint32_t)r;
    atomicAdd(&chcnt[r], 1u);
  });
  __syncthreads();
  }
  if (tid == 0) {
    int L = 0;
    for (int r = 0; r < nIni; r++) {
      uint32_t cn = codes ? (uint32_t)pyr[OCT_PYR_OFF(nIni, 0) + r] : chcnt[r];
      if (cn > 0) {
        OctNode nd;
        nd.ulx = (short)(int)(hX * (float)r);
        nd.urx = (short)(int)(hX * (float)(r + 1));
        nd.uly = 0;
        nd.bry = (short)Hrect;
        nodeA[L] = nd;
        cntA[L] = cn;
        if (codes) codeA[L] = (uint16_t)(r << 5); else chpos[r] = L;
        L++;
      }
    }
    shI[0] = L;
  }
  __syncthreads();
  if (!codes) for_keys(n, [&](int, uint32_t &, uint32_t &nd) { nd = (uint32_t)chpos[nd]; });
  int L = shI[0];
  __syncthreads();
  OSTAMP(1);

  // ---- C. rounds ----
  const int N = G.N;
  bool careful = false;
  OctNode *nodes = nodeA, *nodesN = nodeB;
  uint32_t *cnts = cntA, *cntsN = cntB;
  uint16_t *ncode = codeA, *ncodeN = codeB;
  // code form: every node of the list writes its list position over its leaves (each leaf once; leaves without keys belong to no
  // node and are not read), then the keys exchange their leaf code for the position
  auto label_keys = [&]() {
    for (int w = tid; w < 4 * L; w += NT) {
      const int i = w >> 2, part = w & 3;
      const uint32_t code = ncode[i];
      const int up = OCT_D - (int)(code >> 13), side = 1 << up;
      const int x0 = (int)((code >> 5) & 255u) << up, y0 = (int)(code & 31u) << up;
      if (up == 0) { if (part == 0) pyr[(x0 << OCT_D) + y0] = (uint16_t)i; }
      else
        for (int cx = part; cx < side; cx += 4) {
          uint32_t *col = reinterpret_cast<uint32_t *>(pyr + ((x0 + cx) << OCT_D) + y0);
          for (int j = 0; j < side / 2; j++) col[j] = (uint32_t)i * 0x10001u;
        }
    }
    __syncthreads();
    for_keys(n, [&](int, uint32_t &, uint32_t &nd) { nd = (uint32_t)pyr[nd]; });
    __syncthreads();
  };
  // key counts of node i's four children: the finer grid's cells in the code form, else what this round's key pass counted
  auto child_counts = [&](int i, uint32_t &c0, uint32_t &c1, uint32_t &c2, uint32_t &c3) {
    if (codes) {
      const uint32_t code = ncode[i];
      const int d = min((int)(code >> 13), OCT_D - 1), ix = (int)((code >> 5) & 255u), iy = (int)(code & 31u);
      const uint16_t *fine = pyr + OCT_PYR_OFF(nIni, d + 1);
      const uint32_t w0 = *reinterpret_cast<const uint32_t *>(fine + ((2 * ix) << (d + 1)) + 2 * iy);
      const uint32_t w1 = *reinterpret_cast<const uint32_t *>(fine + ((2 * ix + 1) << (d + 1)) + 2 * iy);
      c0 = w0 & 0xffffu; c1 = w1 & 0xffffu; c2 = w0 >> 16; c3 = w1 >> 16;
    } else {
      c0 = chcnt[i * 4]; c1 = chcnt[i * 4 + 1]; c2 = chcnt[i * 4 + 2]; c3 = chcnt[i * 4 + 3];
    }
  };
  auto child_nodes = [&](int i) -> uint32_t {
    uint32_t c0, c1, c2, c3;
    child_counts(i, c0, c1, c2, c3);
    return (c0 > 0) + (c1 > 0) + (c2 > 0) + (c3 > 0);
  };
  for (int guard = 0; guard < 64; guard++) {
    const int prevSize = L;
    // deeper than OCT_D: some node with more than one key is a leaf of the grid (shI[5], set when the node was made), so this round
    // and the ones after it count and re-label per key
    if (codes && shI[5] != 0) { label_keys(); codes = false; }
    if (!codes) for (int i = tid; i < 4 * L; i += NT) chcnt[i] = 0;
    if (tid == 0) { shI[1] = 0; shI[2] = 0x7fffffff; }
    __syncthreads();
    // child key counts of every expandable node
    if (!codes) for_keys(n, [&](int, uint32_t &c, uint32_t &nd) {
      if (cnts[nd] > 1) {
        OctNode o = nodes[nd];
        int x = c & 0xfff, y = (c >> 12) & 0xfff;
        int hx = (o.urx - o.ulx + 1) >> 1, hy = (o.bry - o.uly + 1) >> 1;  // ceil(/2), :481-482
        int q = (x < o.ulx + hx ? 0 : 1) + (y < o.uly + hy ? 0 : 2);
        atomicAdd(&chcnt[nd * 4 + q], 1u);
      }
    });
    __syncthreads();
    OSTAMP(2);
    // A full round (every node with more than one key is split, in list order: rank order = list order) needs three prefix sums
    // over the list - expandable nodes before me, their children before me, unprocessed nodes before me - and gets them from ONE
    // scan of packed counters (10 + 12 + 10 bits: lists below 1024 nodes); careful rounds, which rank by size, keep three scans.
    int mstar, Eproc, Lnew;
    const bool fusedScan = !careful && L < 1024;
    if (fusedScan) {
      for (int i = tid; i < L; i += NT) {
        const bool e = cnts[i] > 1;
        const uint32_t c = e ? child_nodes(i) : 0u;
        sflag[i] = (e ? 1u : 0u) | (c << 10) | ((e ? 0u : 1u) << 22);
      }
      __syncthreads();
      const uint32_t tot = lds_excl_scan<NT>(sflag, L, sw);
      mstar = (int)(tot & 1023u) - 1;
      Eproc = (int)((tot >> 10) & 4095u);
      Lnew = Eproc + (int)(tot >> 22);
    } else {
    // rank of the expandable nodes in processing order
    if (!careful) {
      for (int i = tid; i < L; i += NT) sflag[i] = cnts[i] > 1 ? 1u : 0u;
      __syncthreads();
      uint32_t nX = lds_excl_scan<NT>(sflag, L, sw);
      for (int i = tid; i < L; i += NT) rankOf[i] = cnts[i] > 1 ? (int)sflag[i] : -1;
      if (tid == 0) shI[3] = (int)nX;
    } else {
      // rank by (size descending, list position ascending) = the number of expandable nodes that go first: four adjacent lanes
      // per node, each counting over a quarter of the list, summed across the quad (DPP)
      uint32_t myX = 0;
      for (int i0 = 0; i0 < L; i0 += NT / 4) {
        const int i = i0 + (tid >> 2), part = tid & 3;
        const uint32_t ci = i < L ? cnts[i] : 0u;
        int r = 0;
        if (ci > 1)
          for (int j = part; j < L; j += 4) {
            const uint32_t cj = cnts[j];
            r += (cj > 1 && (cj > ci || (cj == ci && j < i))) ? 1 : 0;
          }
        r += __builtin_amdgcn_update_dpp(0, r, 0xb1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]
        r += __builtin_amdgcn_update_dpp(0, r, 0x4e, 0xf, 0xf, true);   // quad_perm [2,3,0,1]
        if (i < L && part == 0) {
          rankOf[i] = ci > 1 ? r : -1;
          if (ci > 1) myX++;
        }
      }
      myX = (uint32_t)wave_sum_i32((int)myX);
      if (lane == 0 && myX) atomicAdd(&shI[1], (int)myX);
      __syncthreads();
      if (tid == 0) { shI[3] = shI[1]; shI[1] = 0; }
    }
    __syncthreads();
    const int nX = shI[3];
    // child counts in rank order -> inclusive sums
    for (int i = tid; i < L; i += NT) {
      int r = rankOf[i];
      if (r >= 0) {
        uint32_t c = child_nodes(i);
        incl[r] = c;
      }
    }
    __syncthreads();
    lds_excl_scan<NT>(incl, nX, sw);  // exclusive; inclusive = excl + c, recomputed below
    // cut of a careful round: first rank r with L + incl(r) - (r+1) >= N  (:728)
    if (careful) {
      for (int i = tid; i < L; i += NT) {
        int r = rankOf[i];
        if (r >= 0) {
          uint32_t c = child_nodes(i);
          int after = L + (int)(incl[r] + c) - (r + 1);
          if (after >= N) atomicMin(&shI[2], r);
        }
      }
    }
    __syncthreads();
    mstar = nX - 1;
    if (careful && shI[2] != 0x7fffffff) mstar = shI[2];
    // Eproc = inclusive sum at mstar; unprocessed flags
    for (int i = tid; i < L; i += NT) {
      int r = rankOf[i];
      bool proc = r >= 0 && r <= mstar;
      sflag[i] = proc ? 0u : 1u;
      if (r == mstar && r >= 0) {
        uint32_t c = child_nodes(i);
        shI[4] = (int)(incl[r] + c);
      }
    }
    if (tid == 0 && nX == 0) shI[4] = 0;
    __syncthreads();
    Eproc = shI[4];
    uint32_t nUnproc = lds_excl_scan<NT>(sflag, L, sw);
    Lnew = Eproc + (int)nUnproc;
    }
    OSTAMP(3);
    // build the next list
    for (int i = tid; i < L; i += NT) {
      OctNode o = nodes[i];
      bool proc;
      uint32_t childrenBefore, unprocBefore;
      if (fusedScan) {
        const uint32_t pk = sflag[i];
        proc = cnts[i] > 1; childrenBefore = (pk >> 10) & 4095u; unprocBefore = pk >> 22;
      } else {
        const int r = rankOf[i];
        proc = r >= 0 && r <= mstar; childrenBefore = proc ? incl[r] : 0u; unprocBefore = sflag[i];
      }
      if (proc) {
        uint32_t c0, c1, c2, c3;
        child_counts(i, c0, c1, c2, c3);
        uint32_t c = (c0 > 0) + (c1 > 0) + (c2 > 0) + (c3 > 0);
        const uint32_t code = codes ? (uint32_t)ncode[i] : 0u;
        const uint32_t dN = (code >> 13) + 1u, ixN = 2u * ((code >> 5) & 255u), iyN = 2u * (code & 31u);   // the children's depth, first cell
        int pos = Eproc - (int)(childrenBefore + c);  // block start; inside the block n4,n3,n2,n1
        int hx = (o.urx - o.ulx + 1) >> 1, hy = (o.bry - o.uly + 1) >> 1;
        int nexp = 0;
        uint32_t cc[4] = {c0, c1, c2, c3};
#pragma unroll
        for (int q = 3; q >= 0; q--) {
          if (cc[q] > 0) {
            OctNode ch;
            ch.ulx = (short)((q & 1) ? o.ulx + hx : o.ulx);
            ch.urx = (short)((q & 1) ? o.urx : o.ulx + hx);
            ch.uly = (short)((q & 2) ? o.uly + hy : o.uly);
            ch.bry = (short)((q & 2) ? o.bry : o.uly + hy);
            if (pos < CAP) { nodesN[pos] = ch; cntsN[pos] = cc[q]; }
            if (codes) { if (pos < CAP) ncodeN[pos] = (uint16_t)((dN << 13) | ((ixN + (q & 1)) << 5) | (iyN + (q >> 1))); }
            else chpos[i * 4 + q] = pos;
            nexp += cc[q] > 1 ? 1 : 0;
            pos++;
          } else {
            if (!codes) chpos[i * 4 + q] = -1;
          }
        }
        if (nexp) atomicAdd(&shI[1], nexp);
        if (codes) { if (nexp && dN == OCT_D) shI[5] = 1; }
        else npos[i] = -1;
      } else {
        int pos = Eproc + (int)unprocBefore;
        if (pos < CAP) { nodesN[pos] = o; cntsN[pos] = cnts[i]; }
        if (codes) { if (pos < CAP) ncodeN[pos] = ncode[i]; }
        else npos[i] = pos;
      }
    }
    __syncthreads();
    OSTAMP(4);
    // re-label the keys
    if (!codes) for_keys(n, [&](int, uint32_t &c, uint32_t &nd) {
      int np = npos[nd];
      if (np < 0) {
        OctNode o = nodes[nd];
        int x = c & 0xfff, y = (c >> 12) & 0xfff;
        int hx = (o.urx - o.ulx + 1) >> 1, hy = (o.bry - o.uly + 1) >> 1;
        int q = (x < o.ulx + hx ? 0 : 1) + (y < o.uly + hy ? 0 : 2);
        np = chpos[nd * 4 + q];
      }
      nd = (uint32_t)(uint16_t)np;
    });
    const int nToExpand = shI[1];
    __syncthreads();
    OSTAMP(5);
    { OctNode *t = nodes; nodes = nodesN; nodesN = t; }
    { uint32_t *t = cnts; cnts = cntsN; cntsN = t; }
    { uint16_t *t = ncode; ncode = ncodeN; ncodeN = t; }
    L = min(Lnew, CAP);
    if (Lnew >= N || Lnew == prevSize) break;                      // :667, :731
    if (!careful && Lnew + nToExpand * 3 > N) careful = true;      // :671
  }

  if (codes) label_keys();
  // ---- D. best key per node, list order out, lapping ranks (ORBextractor.cc:742-758, :1169-1178) ----
  for (int i = tid; i < L; i += NT) best[i] = 0ull;
  __syncthreads();
  for_keys(n, [&](int k, uint32_t &c, uint32_t &nd) {
    const unsigned long long key = ((unsigned long long)(c >> 24) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)k);
    atomicMax(&best[nd], key);
  });
  __syncthreads();
  uint32_t *lkp = P.lkp + (size_t)frame * P.lkp_fs + G.kpBase;
  uint16_t *lrank = P.lrank + (size_t)frame * P.lkp_fs + G.kpBase;
  const int Lout = min(L, G.kpCap);
  // every node holds at least one key and exactly one key equals its maximum: that key's thread writes the node's keypoint
  for_keys(n, [&](int k, uint32_t &c, uint32_t &nd) {
    const unsigned long long key = ((unsigned long long)(c >> 24) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)k);
    if ((int)nd < Lout && best[nd] == key) {
      lkp[nd] = c;
      float xs = (float)((int)(c & 0xfff) + ORB_MIN_BORDER);
      if (level != 0) xs = xs * G.scale;  // keypoint->pt *= scale, :1164-1166
      const bool lap = xs >= (float)P.lap0 && xs <= (float)P.lap1;
      sflag[nd] = lap ? 1u : 0u;
    }
  });
  __syncthreads();
  // sflag was read as packed flags; keep a copy of the flag in incl before the scan overwrites it
  for (int i = tid; i < Lout; i += NT) incl[i] = sflag[i];
  __syncthreads();
  uint32_t nLap = lds_excl_scan<NT>(sflag, Lout, sw);
  for (int i = tid; i < Lout; i += NT) {
    uint32_t f = incl[i];
    uint32_t rank = f ? sflag[i] : (uint32_t)i - sflag[i];
    lrank[i] = (uint16_t)((f << 15) | (rank & 0x7fff));
  }
  if (tid == 0) { lcnt[0] = Lout; lcnt[1] = (int)nLap; }
  OSTAMP(6);
}

// ------------------------------------------------------------------------------------------------------------
// K5: cv::GaussianBlur 7x7 sigma 2 BORDER_REFLECT_101, 8U fixed point: taps {18,34,49,55,49,34,18} - on the matrix pipe.
// The 8-bit GaussianBlur is an exact integer computation - row sums of at most 257 * 255 (16 bits, no rounding), then
// (sum of 7 weighted row sums + 32768) >> 16 - i.e. two products with banded constant matrices:
//     T = I H      (H[k][x] = tap[k - x - 13]: 64 input columns -> 32 output columns)
//     O = V T      (V[y][k] = tap[k - y]:      64 rows of T     -> 32 output rows)
// v_mfma_i32_32x32x32_i8 takes SIGNED bytes, so pixels enter as I - 128 (one xor per dword) with the correction 128 * 257 in the
// accumulator seed, and the 16-bit row sums are split into their high and low byte (again minus 128) for the second product:
//     sum V T = 256 (sum V hi' ) + (sum V lo') + 257 * 128 * 257.
// The accumulator of the first product (row index in the registers, column on the lane) IS the B operand of the second one - the
// guide's "accumulator tile as the next MFMA's operand": element j of lane half h is row (j & 3) + 8 (j >> 2) + 4 h, and V's
// fragments are laid out in that order - so nothing moves between the passes but the byte split.  Per 32 x 32 outputs: 4 + 4
// MFMAs and about 130 vector instructions per wavefront for the arithmetic (the v_dot4 / v_dot2 form of rounds 1-2: 220), and with
// the border tiles loaded by LDS-DMA like the interior ones (half of all tiles touch an edge; their byte-wise loops were a third
// of the old kernel's instructions) 0.247 -> 0.172 ms per 256 frames, byte for byte the same planes.
// Workgroup = the same 128 x 32 tile as before, wavefront w its columns 32 w .. 32 w + 31; the results go through a 4 KB LDS
// image so that the stores are 16-byte row segments.
// ------------------------------------------------------------------------------------------------------------
// per lane (column / row n = lane & 31, half h = lane >> 5): H fragments of K-steps 0, 1, then V fragments of K-steps 0, 1
struct BlurTab { uint32_t v[64][16]; };
constexpr uint32_t blur_tap(int d) { return d == 0 || d == 6 ? 18u : d == 1 || d == 5 ? 34u : d == 2 || d == 4 ? 49u : d == 3 ? 55u : 0u; }
constexpr BlurTab make_blur_tab() {
  BlurTab t{};
  for (int lane = 0; lane < 64; lane++) {
    const int n = lane & 31, h = lane >> 5;
    for (int s = 0; s < 2; s++)
      for (int d = 0; d < 4; d++) {
        uint32_t hv = 0, vv = 0;
        for (int b = 0; b < 4; b++) {
          const int j = 4 * d + b;
          hv |= blur_tap(32 * s + 16 * h + j - n - 13) << (8 * b);                       // H[k = 32 s + 16 h + j][n]: input column k -> output column n
          vv |= blur_tap(32 * s + (j & 3) + 8 * (j >> 2) + 4 * h - n) << (8 * b);        // V[m = n][k = 32 s + rho(h, j)]: row sum k -> output row m
        }
        t.v[lane][4 * s + d] = hv;
        t.v[lane][8 + 4 * s + d] = vv;
      }
  }
  return t;
}
__device__ const BlurTab g_blurTab = make_blur_tab();

#define BLUR_TX 128
#ifndef BLUR_TY
#define BLUR_TY 64               // output rows per workgroup: 32-row products, neighbours share a block of row sums
#endif
#define BLUR_ROWS_IN (BLUR_TY + 6)
#define BLURM_PITCH 176          // bytes per input tile row: 160 used (columns x0 - 16 .. x0 + 143) + one 16-byte chunk of padding
                                 // (44 dwords: 16 consecutive rows start in 16 different 4-bank groups, the A fragments read conflict-free)
#define BLURM_OPITCH 144         // bytes per output staging row
// Workgroup = 128 x 64 outputs (late round 3; 128 x 32 before): input rows y0 - 3 .. y0 + 66 form three 32-row blocks of row sums
// T0, T1, T2 (rows 70 .. 95 of the third only meet zero taps), output rows 0 .. 31 = V (T0, T1), rows 32 .. 63 = V (T1, T2): 6 + 8
// products per 64 rows instead of 8 + 8, one block of row sums and byte splits less, and - what the kernel's time is made of - one HBM
// round trip in front of twice the work.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7, 7))) void k_blur(FrameParams P) {   // seven workgroups per CU by LDS (21.5 KB each): no more than 72 registers
#define BSTAMP(i) TSTAMP(i, (size_t)blockIdx.x, level)
  TSTAMP_BEGIN();
  typedef int v4i __attribute__((ext_vector_type(4)));
  typedef int v16i __attribute__((ext_vector_type(16)));
  // input rows 0 .. 69, then the output staging rows: the A fragments of the third block read "rows" 70 .. 95, i.e. into the staging
  // area - any bytes will do there, they are multiplied by zero taps
  __shared__ __align__(16) uint8_t sLds[BLUR_ROWS_IN * BLURM_PITCH + BLUR_TY * BLURM_OPITCH];
  static_assert(BLUR_TY % 32 == 0 && (BLUR_TY + 32) * BLURM_PITCH <= BLUR_ROWS_IN * BLURM_PITCH + BLUR_TY * BLURM_OPITCH, "the last block's rows must stay inside the allocation");
  uint8_t *sIn = sLds, *sOut = sLds + BLUR_ROWS_IN * BLURM_PITCH;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int tile, frame;
  xcd_map(P.totalTiles, P.magicTiles, P.nframes, frame, tile);
  const uint4 t0 = reinterpret_cast<const uint4 *>(P.tiles)[2 * tile], t1 = reinterpret_cast<const uint4 *>(P.tiles)[2 * tile + 1];
  const int x0 = (int)(t0.x & 0xffffu), y0 = (int)(t0.x >> 16), level = (int)(t0.y & 0xffu);
  // the host's view of the tile (orbx_configure): nothing of its 70 x 176-byte window is reflected, clamped or synthesised; every
  // 16-byte store of its outputs lies inside the blurred plane's rows
  const bool interior = (t0.y & BLUR_TILE_INTERIOR) != 0u, wholeStores = (t0.y & BLUR_TILE_WHOLE_STORES) != 0u;
  struct { int w, h, bpitch; size_t boff; } G;
  G.w = (int)(t0.z & 0xffffu); G.h = (int)(t0.z >> 16); G.bpitch = (int)(t0.w >> 16);
  G.boff = ((size_t)t1.w << 32) | t1.z;
  int pitch;
  const uint8_t *img;
  if (level == 0) { pitch = (int)P.img0_stride; img = P.img0 + (size_t)frame * P.img0_frame_stride; }
  else { pitch = (int)(t0.w & 0xffffu); img = P.pyr + (size_t)frame * P.pyr_fs + (((size_t)t1.y << 32) | t1.x); }
  const bool aligned = ((((uintptr_t)img) | (uintptr_t)pitch) & 3u) == 0;
  // ---- input tile: 70 rows x 11 chunks of 16 bytes from column x0 - 16, by LDS-DMA for EVERY tile of a level that is larger than
  // the halo: BORDER_REFLECT_101 across the top / bottom edge is a source ROW (an address), across the left / right edge it is at
  // most three bytes per row, which a few threads copy inside the tile once the DMA has landed.  Chunks that would start outside
  // the row's memory are fetched from a clamped address (their bytes never meet a non-zero tap of a stored output, except the
  // reflected ones); the same holds for rows more than three below the image (clamped).  Tiny levels and unaligned level-0 images
  // take the byte-wise loop.
  const int wlim = level == 0 ? G.w : pitch;                 // bytes of a row that may be read (level 0 is the caller's image: not past its rows)
  const bool dma = aligned && G.w >= 160 && G.h >= 40 && (wlim & 15) == 0;
  const bool edgeL = x0 == 0, edgeR = x0 + 131 >= G.w;       // some stored output of this tile needs a column left of 0 / right of w - 1
  // ---- constant operands of this lane: H (B of the first product), V (A of the second), in the operands' element order (g_blurTab).
  // Requested in front of the tile, so that no path fetches them behind a barrier, where nothing else would hide the round trip.
  const int n = lane & 31, hh = lane >> 5;
  v4i Hb[2], Va[2];
  {
    const uint4 *tab = reinterpret_cast<const uint4 *>(g_blurTab.v[lane]);
    const uint4 q0 = tab[0], q1 = tab[1], q2 = tab[2], q3 = tab[3];
    Hb[0] = v4i{(int)q0.x, (int)q0.y, (int)q0.z, (int)q0.w}; Hb[1] = v4i{(int)q1.x, (int)q1.y, (int)q1.z, (int)q1.w};
    Va[0] = v4i{(int)q2.x, (int)q2.y, (int)q2.z, (int)q2.w}; Va[1] = v4i{(int)q3.x, (int)q3.y, (int)q3.z, (int)q3.w};
  }
  if (dma && interior) {
    // Interior tiles: chunk idx = 11 r + c comes from img + (y0 - 3 + r) * pitch + x0 - 16 + 16 c as it is.  A lane's chunk of the next
    // trip is idx + 256 = idx + 23 * 11 + 3, i.e. (r + 23, c + 3) or, past the row's end, (r + 24, c - 8): one add per trip for the
    // address, no divide, no reflection, no clamp.
    const uint8_t *tile0 = img + ((uint32_t)(y0 - 3) * (uint32_t)pitch + (uint32_t)(x0 - 16));   // uniform: scalar arithmetic
    const uint32_t r0 = mul24((uint32_t)tid, 5958u) >> 16;     // tid / 11
    uint32_t c = (uint32_t)tid - 11u * r0, off = mul24(r0, (uint32_t)pitch) + 16u * c;
    const uint32_t step = 23u * (uint32_t)pitch + 48u, stepWrap = 24u * (uint32_t)pitch - 128u;
#pragma unroll
    for (int k = 0; k < (BLUR_ROWS_IN * 11 + 255) / 256; k++) {
      if (256 * (k + 1) <= BLUR_ROWS_IN * 11 || tid + 256 * k < BLUR_ROWS_IN * 11)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(tile0 + off),
                                         (__attribute__((address_space(3))) void *)(sIn + (tid + 256 * k) * 16), 16, 0, 0);
      const bool wrap = c >= 8u;
      c = wrap ? c - 8u : c + 3u;
      off += wrap ? stepWrap : step;
    }
    BSTAMP(0);
  } else if (dma) {
    for (int idx = tid; idx < BLUR_ROWS_IN * 11; idx += 256) {
      const uint32_t r = mul24((uint32_t)idx, 5958u) >> 16, c = (uint32_t)idx - 11u * r;      // idx / 11, exact below 770
      int yy = y0 - 3 + (int)r;
      yy = yy < 0 ? -yy : yy;
      yy = yy >= G.h ? 2 * (G.h - 1) - yy : yy;
      yy = max(yy, 0);
      int xb = x0 - 16 + 16 * (int)c;
      xb = min(max(xb, 0), wlim - 16);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(img + (mul24((uint32_t)yy, (uint32_t)pitch) + (uint32_t)xb)),
                                       (__attribute__((address_space(3))) void *)(sIn + idx * 16), 16, 0, 0);
    }
    BSTAMP(0);
    if (edgeL || edgeR) {
      __syncthreads();                                        // the tile has landed (the compiler drains the DMA in front of the barrier)
      for (int i = tid; i < BLUR_ROWS_IN * 6; i += 256) {
        const int r = (int)(mul24((uint32_t)i, 10923u) >> 16), k = i - 6 * r;      // i / 6, exact below 420
        const int x = k < 3 ? -1 - k : G.w + (k - 3);         // the column to synthesise
        const int xs = k < 3 ? 1 + k : G.w - 2 - (k - 3);     // its BORDER_REFLECT_101 source
        const bool need = k < 3 ? edgeL : (edgeR && x - (x0 - 16) < 160);
        if (need) sIn[r * BLURM_PITCH + (x - (x0 - 16))] = sIn[r * BLURM_PITCH + (xs - (x0 - 16))];
      }
    }
  } else {
    // byte-wise loop.  Only columns x0 - 3 .. x0 + 130 meet non-zero taps.
    const bool small = G.w < 16 || G.h < 16;
    auto srcRow = [&](int r) {
      int yy = y0 + r - 3;
      if (small) yy = reflect101(yy, G.h);
      else { yy = yy < 0 ? -yy : yy; yy = yy >= G.h ? 2 * (G.h - 1) - yy : yy; yy = max(yy, 0); }
      return img + mul24((uint32_t)yy, (uint32_t)pitch);
    };
    for (int idx = tid; idx < BLUR_ROWS_IN * 36; idx += 256) {          // dword columns 3 .. 38 of the 40: bytes x0 - 4 .. x0 + 139
      const uint32_t r = mul24((uint32_t)idx, 3641u) >> 17, c = 3u + ((uint32_t)idx - r * 36u);   // idx / 36, exact below 4824
      const int xb = x0 - 16 + 4 * (int)c;
      const uint8_t *row = srcRow((int)r);
      uint32_t v;
      if (aligned && xb >= 0 && xb + 3 < G.w) v = *reinterpret_cast<const uint32_t *>(row + xb);
      else {
        v = 0;
#pragma unroll
        for (int kk = 0; kk < 4; kk++) {
          int xx = xb + kk;
          if (small) xx = reflect101(xx, G.w);
          else { xx = xx < 0 ? -xx : xx; xx = xx >= G.w ? 2 * (G.w - 1) - xx : xx; xx = max(xx, 0); }   // beyond w + w - 1: never under a stored output
          v |= (uint32_t)row[xx] << (8 * kk);
        }
      }
      *reinterpret_cast<uint32_t *>(sIn + r * BLURM_PITCH + 4u * c) = v;
    }
    BSTAMP(0);
  }
  __syncthreads();
  BSTAMP(1);
  // ---- T = I H for a 32-row block of the tile's rows, seeded with 128 * 257 so that the accumulators are the row sums 0 .. 65535,
  // split into (high byte - 128, low byte - 128): the second product's B fragments (element j = register j)
  auto row_sums = [&](int mt, v4i &Bhi, v4i &Blo) {
    // (the seed is made opaque so that every block re-materialises its 16 copies: kept alive as one constant vector across the
    // kernel they cost 16 registers, i.e. resident wavefronts)
    int seedT = 128 * 257;
    asm volatile("" : "+v"(seedT));
    v16i acc;
#pragma unroll
    for (int j = 0; j < 16; j++) acc[j] = seedT;
#pragma unroll
    for (int s = 0; s < 2; s++) {
      v4i a = *reinterpret_cast<const v4i *>(sIn + (32 * mt + n) * BLURM_PITCH + 32 * wid + 32 * s + 16 * hh);
      a[0] ^= (int)0x80808080; a[1] ^= (int)0x80808080; a[2] ^= (int)0x80808080; a[3] ^= (int)0x80808080;
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, Hb[s], acc, 0, 0, 0);
    }
#pragma unroll
    for (int d = 0; d < 4; d++) {
      const uint32_t p01 = __builtin_amdgcn_perm((uint32_t)acc[4 * d + 1], (uint32_t)acc[4 * d], 0x05010400u);   // lo0 lo1 hi0 hi1
      const uint32_t p23 = __builtin_amdgcn_perm((uint32_t)acc[4 * d + 3], (uint32_t)acc[4 * d + 2], 0x05010400u);
      Blo[d] = (int)(__builtin_amdgcn_perm(p23, p01, 0x05040100u) ^ 0x80808080u);
      Bhi[d] = (int)(__builtin_amdgcn_perm(p23, p01, 0x07060302u) ^ 0x80808080u);
    }
  };
  // ---- O = V T over two blocks of row sums, high and low bytes separately; (256 aH + aL) >> 16 saturated to a byte into the staging
  // rows row0 .. row0 + 31 (register j is output row rho(h, j), the lane's column is 32 w + n)
  auto outputs = [&](const v4i &BhiA, const v4i &BloA, const v4i &BhiB, const v4i &BloB, int row0) {
    // ONE accumulator: the high-byte product first, then 256 * aH + the rounding constant is the C operand of the low-byte product
    // (two accumulators side by side cost 16 more registers, i.e. two resident wavefronts per SIMD)
    v16i acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(Va[0], BhiA, v16i{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(Va[1], BhiB, acc, 0, 0, 0);
    int seedL = 257 * 128 * 257 + 32768;
    asm volatile("" : "+v"(seedL));
#pragma unroll
    for (int j = 0; j < 16; j++) acc[j] = (int)(((uint32_t)acc[j] << 8) + (uint32_t)seedL);
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(Va[0], BloA, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(Va[1], BloB, acc, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint32_t b = min((uint32_t)acc[j] >> 16, 255u);
      sOut[(row0 + (j & 3) + 8 * (j >> 2) + 4 * hh) * BLURM_OPITCH + 32 * wid + n] = (uint8_t)b;
    }
  };
  // (the scheduling barriers keep the phases apart: interleaved, their accumulators need 84 registers instead of 64 and cost three
  // resident wavefronts per SIMD)
  v4i Hp, Lp, Hc, Lc;
  row_sums(0, Hp, Lp);
#pragma unroll
  for (int k = 0; k < BLUR_TY / 32; k++) {
    if (k > 0 && y0 + 32 * k >= G.h) break;      // no output row down there (uniform)
    __builtin_amdgcn_sched_barrier(0);
    row_sums(k + 1, Hc, Lc);
    __builtin_amdgcn_sched_barrier(0);
    outputs(Hp, Lp, Hc, Lc, 32 * k);
    Hp = Hc; Lp = Lc;
  }
  __syncthreads();
  // ---- stores: thread = 16-byte segment seg of staging rows tid / 8 and tid / 8 + 32.  One base per workgroup (the tile's first
  // output, scalar) and a 32-bit offset per thread that advances by 32 rows; the byte tail exists only where the record allows it.
  {
    uint8_t *out0 = P.blur + (size_t)frame * P.blur_fs + G.boff + (size_t)y0 * G.bpitch + x0;
    const int row = tid >> 3, seg = tid & 7, x = x0 + 16 * seg;
    const uint8_t *b = sOut + row * BLURM_OPITCH + 16 * seg;
    uint32_t off = mul24((uint32_t)row, (uint32_t)G.bpitch) + 16u * (uint32_t)seg;
#pragma unroll
    for (int t = 0; t < BLUR_TY / 32; t++) {
      if (y0 + row + 32 * t < G.h && x < G.w) {
        if (wholeStores || x + 16 <= G.bpitch) *reinterpret_cast<uint4 *>(out0 + off) = *reinterpret_cast<const uint4 *>(b);
        else {
#pragma clang loop vectorize(disable) unroll(disable)
          for (int cc = 0; cc < 16 && x + cc < G.w; cc++) out0[off + cc] = b[cc];
        }
      }
      b += 32 * BLURM_OPITCH;
      off += 32u * (uint32_t)G.bpitch;
    }
  }
  BSTAMP(2);
#undef BSTAMP
}

// ------------------------------------------------------------------------------------------------------------
// K4+K6+K7: IC_Angle (ORBextractor.cc:75-102), computeOrbDescriptor (:106-145) and the lapping-order scatter
// (:1159-1180).  One wavefront per keypoint: 749-pixel disc split over 64 lanes and reduced with shuffles;
// 256 binary tests = 4 rounds of 64 lanes, each round packed with one 64-bit ballot (= 8 descriptor bytes).
// ------------------------------------------------------------------------------------------------------------
// Device only: orbx_fast_atan2_device evaluates it for tests/test_gpu_libm_device.py, against the oracle's restatement.
__device__ __forceinline__ float fast_atan2_deg(float y, float x) {  // cv::fastAtan2, SURVEY.md A.6
  const float scale = (float)(180.0 / 3.1415926535897932384626433832795);
  const float p1 = 0.9997878412794807f * scale, p3 = -0.3258083974640975f * scale;
  const float p5 = 0.1555786518463281f * scale, p7 = -0.04432655554792128f * scale;
  float ax = fabsf(x), ay = fabsf(y);
  float a, c, c2;
  if (ax >= ay) {
    c = ay / (ax + (float)2.2204460492503131e-16);
    c2 = c * c;
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  } else {
    c = ax / (ay + (float)2.2204460492503131e-16);
    c2 = c * c;
    a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  }
  if (x < 0) a = 180.f - a;
  if (y < 0) a = 360.f - a;
  return a;
}

struct KpOut { float x, y, size, angle, response; int32_t octave, class_id; };

// K = 1, one keypoint per wavefront: the form of few-frame ("wide") calls, whose ~1000 keypoints per frame have to spread over the
// whole chip.  Four wavefronts per workgroup, grid = ceil(totalKp / 4) workgroups per frame.
__device__ __forceinline__ void describe_one(const FrameParams &P) {
  const int lane = threadIdx.x & 63;
  int frame, blk;
  xcd_map((P.totalKp + 3) / 4, P.magicKpBlk, P.nframes, frame, blk);
  const int j = blk * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // wave-uniform: scalar loads below
  if (j >= P.totalKp) return;
  // Everything that does not depend on the keypoint is requested first (one memory latency for all of it): my share of
  // the disc and pattern tables, the level counts, the keypoint itself (its slot j is level-independent).
  const uint32_t packed = P.lkp[(size_t)frame * P.lkp_fs + j];
  const uint32_t rk = P.lrank[(size_t)frame * P.lkp_fs + j];
  const uint4 dw0 = *reinterpret_cast<const uint4 *>(&c_disc.w[lane][0]);
  const uint2 dw1 = *reinterpret_cast<const uint2 *>(&c_disc.w[lane][4]);
  uint32_t pw[4];
#pragma unroll
  for (int r = 0; r < 4; r++) pw[r] = reinterpret_cast<const uint32_t *>(c_pattern)[r * 64 + lane];  // x0, y0, x1, y1 as int8
  const int32_t *lc = P.lcnt + (size_t)frame * P.nlevels * 2;
  int level = 0;
#pragma unroll
  for (int l = 1; l < ORB_MAXL; l++)
    if (l < P.nlevels && j >= P.geom[l].kpBase) level = l;
  int nTot = 0, lapTot = 0, lapBefore = 0, monoBefore = 0, myCount = 0;
#pragma unroll
  for (int l = 0; l < ORB_MAXL; l++)
    if (l < P.nlevels) {
      const int c = lc[l * 2], lp = lc[l * 2 + 1];
      nTot += c;
      lapTot += lp;
      if (l < level) { lapBefore += lp; monoBefore += c - lp; }
      if (l == level) myCount = c;
    }
  // the frame's totals (keypoints, monoIndex of operator(): ORBextractor.cc:1169-1182) are written by its first wavefront
  if (j == 0 && lane == 0) { P.out_counts[frame * 2] = nTot; P.out_counts[frame * 2 + 1] = nTot - lapTot; }
  const LevelGeom G = P.geom[level];
  const int i = j - G.kpBase;
  if (i >= myCount) return;
  const int X = (int)(packed & 0xfff) + ORB_MIN_BORDER, Y = (int)((packed >> 12) & 0xfff) + ORB_MIN_BORDER;
  const int dst = (rk & 0x8000u) ? nTot - 1 - (lapBefore + (int)(rk & 0x7fff)) : monoBefore + (int)(rk & 0x7fff);

  // IC_Angle on the unblurred level: 12 independent gathers per lane, all in flight together
  int pitch;
  const uint8_t *img = level_plane(P, frame, level, pitch);
  const uint8_t *centre = img + (size_t)Y * pitch + X;
  // The 37x37 blurred patch the 512 steered test points can fall into (|rotated offset| <= 18) is requested NOW, together
  // with the disc gathers, as 37 rows x 10 aligned dwords into this wave's LDS slice: the BRIEF gathers then never leave
  // the CU and the wave pays one global round trip less.  Keypoints are >= 19 px inside the level, so rows Y-18..Y+18 and
  // columns X-18..X+18 exist; the up to 3 extra bytes of the aligned dwords stay inside the plane's pitch padding / next row.
  __shared__ __align__(16) uint8_t sPatch[4][37 * 48];
  uint8_t *myPatch = sPatch[threadIdx.x >> 6];
  const int px0 = (X - 18) & ~3, pox = (X - 18) - px0;
  {
    // LDS-DMA, 16 bytes per lane straight into the patch (no register, no ds_write): 37 rows x 3 chunks, lane-linear;
    // idx / 3 as (idx * 21846) >> 16, exact below 111.  The 48-byte rows reach at most 11 bytes past column X+18+3: inside
    // the plane (the row below exists: keypoints stay 19 px away from the border).
    const uint8_t *brow = P.blur + (size_t)frame * P.blur_fs + G.boff + (size_t)(Y - 18) * G.bpitch + px0;
#pragma unroll
    for (int t = 0; t < 2; t++) {
      const uint32_t idx = (uint32_t)(lane + 64 * t), r = (idx * 21846u) >> 16, c = idx - 3u * r;
      if (idx < 111u)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(brow + (mul24(r, (uint32_t)G.bpitch) + 16u * c)),
                                         (__attribute__((address_space(3))) void *)&myPatch[idx * 16], 16, 0, 0);
    }
  }
  int m10 = 0, m01 = 0;
  int dv[12], du[12], dval[12];
  {
    const uint32_t uw[3] = {dw0.x, dw0.y, dw0.z}, vw[3] = {dw0.w, dw1.x, dw1.y};
#pragma unroll
    for (int t = 0; t < 12; t++) {
      du[t] = (int)(int8_t)(uw[t >> 2] >> (8 * (t & 3)));
      dv[t] = (int)(int8_t)(vw[t >> 2] >> (8 * (t & 3)));
    }
  }
  // The disc pixels: when the level plane is dword-aligned, its 31 rows x 48 bytes around the keypoint come in by LDS-DMA
  // as well (two 16-byte chunks per lane instead of twelve scattered byte gathers) and the disc is read from LDS.
  __shared__ __align__(16) uint8_t sDisc[4][31 * 48];
  uint8_t *myDisc = sDisc[threadIdx.x >> 6];
  if (((((uintptr_t)img) | (uintptr_t)pitch) & 3u) == 0) {
    const int qx0 = (X - 15) & ~3, qox = (X - 15) - qx0;
    const uint8_t *irow = img + (size_t)(Y - 15) * pitch + qx0;
#pragma unroll
    for (int t = 0; t < 2; t++) {
      const uint32_t idx = (uint32_t)(lane + 64 * t), r = (idx * 21846u) >> 16, c = idx - 3u * r;
      if (idx < 93u)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(irow + (mul24(r, (uint32_t)pitch) + 16u * c)),
                                         (__attribute__((address_space(3))) void *)&myDisc[idx * 16], 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // both patches have landed
    const uint8_t *dc = myDisc + 15 * 48 + qox + 15;
#pragma unroll
    for (int t = 0; t < 12; t++) dval[t] = dc[dv[t] * 48 + du[t]];
  } else {
#pragma unroll
    for (int t = 0; t < 12; t++) dval[t] = centre[dv[t] * pitch + du[t]];
  }
#pragma unroll
  for (int t = 0; t < 12; t++) { m10 += du[t] * dval[t]; m01 += dv[t] * dval[t]; }
  m10 = wave_sum_i32(m10);
  m01 = wave_sum_i32(m01);
  const float angle = fast_atan2_deg((float)m01, (float)m10);

  // steered BRIEF on the blurred level
  const float factorPI = (float)(3.1415926535897932384626433832795 / 180.f);
  const float arad = angle * factorPI;
  const float a = orbsc::ref_cosf(arad), b = orbsc::ref_sinf(arad);
  const uint8_t *bc = myPatch + 18 * 48 + pox + 18;   // patch centre; row pitch 48 B
  constexpr int bp = 48;
  unsigned long long bits[4];
  int o0[4], o1[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const float x0 = (float)(int8_t)(pw[r] & 0xff), y0 = (float)(int8_t)((pw[r] >> 8) & 0xff);
    const float x1 = (float)(int8_t)((pw[r] >> 16) & 0xff), y1 = (float)(int8_t)(pw[r] >> 24);
    o0[r] = __float2int_rn(x0 * b + y0 * a) * bp + __float2int_rn(x0 * a - y0 * b);
    o1[r] = __float2int_rn(x1 * b + y1 * a) * bp + __float2int_rn(x1 * a - y1 * b);
  }
  // the patch was written by this wavefront's own LDS-DMA loads (VM counter): long retired by now, but say so
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  int v0[4], v1[4];
#pragma unroll
  for (int r = 0; r < 4; r++) { v0[r] = bc[o0[r]]; v1[r] = bc[o1[r]]; }
#pragma unroll
  for (int r = 0; r < 4; r++) bits[r] = __ballot(v0[r] < v1[r]);
  if (dst < P.cap) {
    uint32_t *dd = reinterpret_cast<uint32_t *>(P.out_desc + ((size_t)frame * P.cap + dst) * 32);
    if (lane < 8) {
      unsigned long long w = bits[lane >> 1];
      dd[lane] = (uint32_t)((lane & 1) ? (w >> 32) : w);
    }
    if (lane == 8) {
      KpOut k;
      k.x = (float)X;
      k.y = (float)Y;
      if (level != 0) { k.x = k.x * G.scale; k.y = k.y * G.scale; }
      k.size = G.kpsize;
      k.angle = angle;
      k.response = (float)(packed >> 24);
      k.octave = level;
      k.class_id = -1;
      reinterpret_cast<KpOut *>(P.out_kps)[(size_t)frame * P.cap + dst] = k;
    }
  }
}

// K = 4, 8 or 16 (ORB_DESCRIBE_K), the batch form: a wavefront owns K consecutive keypoint slots of one frame.  Whatever has one value per keypoint (level,
// lapping slot, angle, cosine, sine, the KpOut record) is computed once for the block with lane = keypoint, whatever depends on the lane
// only (disc offsets, chunk coordinates of the DMA, the BRIEF pattern) once per wavefront, and only the pixel work runs per keypoint, 64
// lanes wide: 12 disc reads + 6 dot products, 8 rotated offsets + 8 patch reads + 4 ballots.  Every keypoint sees the operations of
// describe_one() on the same operands in the same order; the moment sums are integer, hence order-independent.
//
// One step of the transpose-reduce over partial sums: a and b are the partials of two keypoints (or keypoint groups); lanes whose bit
// LANEBIT is clear keep a, the others keep b, and each adds its partner lane's partial of the one it keeps.  The partner of bit 3 is the
// mirrored lane of the 16-lane row (lane ^ 15), of bit 2 the mirrored lane of the 8-lane half row (lane ^ 7), of bits 1 and 0 lane ^ 2
// and lane ^ 1: taken in that order, the partner agrees with the lane in every bit decided before, so both hold the same keypoints.
template <int LANEBIT>
__device__ __forceinline__ int tr_step(int a, int b, int lane) {
  constexpr int CTRL = LANEBIT == 3 ? 0x140 : LANEBIT == 2 ? 0x141 : LANEBIT == 1 ? 0x4e : 0xb1;   // row_mirror, row_half_mirror, quad_perm
  const bool hi = ((lane >> LANEBIT) & 1) != 0;
  const int keep = hi ? b : a, give = hi ? a : b;
  return keep + dpp_or_zero<CTRL, 0xf>(give);
}
// Keypoints LO .. LO + N - 1 of a block of 2^LOG, in order, combined as soon as two neighbouring groups are complete (at most
// 2 (LOG + 1) partials are live).  Index bit s of the keypoint is decided by lane bit LOG - 1 - s: afterwards lane l holds, summed over
// its group of 2^LOG lanes, the moments of keypoint bitreverse(l mod 2^LOG).
template <int LOG, int LO, int N, class F>
__device__ __forceinline__ void tr_range(F &one, int lane, int &r10, int &r01) {
  if constexpr (N == 1) one(std::integral_constant<int, LO>{}, r10, r01);
  else {
    int a10, a01, b10, b01;
    tr_range<LOG, LO, N / 2>(one, lane, a10, a01);
    tr_range<LOG, LO + N / 2, N / 2>(one, lane, b10, b01);
    constexpr int S = N == 2 ? 0 : N == 4 ? 1 : N == 8 ? 2 : 3;
    r10 = tr_step<LOG - 1 - S>(a10, b10, lane);
    r01 = tr_step<LOG - 1 - S>(a01, b01, lane);
  }
}

// (explicit address spaces: through generic pointers the two disc paths of the block form are merged into one set of flat loads)
typedef const __attribute__((address_space(3))) uint8_t *LdsBytes;
typedef const __attribute__((address_space(1))) uint8_t *GlobalBytes;
#define DESC_BUF (37 * 48)                  // a wave-private staging buffer: the 31 x 48 disc window, later the 37 x 48 blurred patch
#define DESC_WAVE_LDS (2 * DESC_BUF + 512)    // two of them (keypoint k + 1 arrives while k is read) + the 64 x 8 bytes of the reduction

template <int K>
__device__ __forceinline__ void describe_block(const FrameParams &P) {
  static_assert(K == 4 || K == 8 || K == 16, "a block is a quad, a half row or a row of DPP lanes");
  constexpr int LOG = K == 16 ? 4 : K == 8 ? 3 : 2;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  int frame, wg;
  xcd_map(ORB_DESCRIBE_GROUPS(P.totalKp, K), P.magicKpBlk, P.nframes, frame, wg);
  const int j0 = (wg * 4 + wid) * K;   // first slot of this wavefront's block
  if (j0 >= P.totalKp) return;
  // all LDS of the kernel is ONE array (a second object beside a DMA target makes the compiler drain the DMA before reading either)
  __shared__ __align__(16) uint8_t sDesc[4][DESC_WAVE_LDS];
  uint8_t *myLds = sDesc[wid];

  // ---- header, lane = keypoint (lanes >= K idle along).  The frame's level counts come in with one load: lane l holds level l's.
  // So does its first slot; the walk over the levels below then waits for memory once, not once per level.
  int cL = 0, lpL = 0, kbL = 0;
  if (lane < P.nlevels) {
    const int2 v = reinterpret_cast<const int2 *>(P.lcnt + (size_t)frame * P.nlevels * 2)[lane];
    cL = v.x; lpL = v.y;
    kbL = P.geom[lane].kpBase;
  }
  const int j = j0 + lane;
  int level = 0, kb = __builtin_amdgcn_readlane(kbL, 0), myCount = __builtin_amdgcn_readlane(cL, 0);
  int lapBefore = 0, monoBefore = 0, nTot = myCount, lapTot = __builtin_amdgcn_readlane(lpL, 0);
  for (int l = 1; l < P.nlevels; l++) {
    const int c = __builtin_amdgcn_readlane(cL, l), lp = __builtin_amdgcn_readlane(lpL, l), base = __builtin_amdgcn_readlane(kbL, l);
    const bool ge = j >= base;   // bases ascend: the last level whose base is not above j is the lane's
    level = ge ? l : level; kb = ge ? base : kb; myCount = ge ? c : myCount;
    lapBefore = ge ? lapTot : lapBefore; monoBefore = ge ? nTot - lapTot : monoBefore;
    nTot += c; lapTot += lp;
  }
  // the frame's totals (keypoints, monoIndex of operator(): ORBextractor.cc:1169-1182) are written by its first wavefront
  if (j0 == 0 && lane == 0) { P.out_counts[frame * 2] = nTot; P.out_counts[frame * 2 + 1] = nTot - lapTot; }
  const bool valid = lane < K && j < P.totalKp && j - kb < myCount;
  const uint32_t validMask = (uint32_t)__ballot(valid);
  if (validMask == 0) return;
  uint32_t packed = 0, rk = 0;
  if (valid) { packed = P.lkp[(size_t)frame * P.lkp_fs + j]; rk = P.lrank[(size_t)frame * P.lkp_fs + j]; }
  const int X = (int)(packed & 0xfff) + ORB_MIN_BORDER, Y = (int)((packed >> 12) & 0xfff) + ORB_MIN_BORDER;
  const int dst = (rk & 0x8000u) ? nTot - 1 - (lapBefore + (int)(rk & 0x7fff)) : monoBefore + (int)(rk & 0x7fff);
  int pitch = (int)P.img0_stride;
  const uint8_t *img = P.img0 + (size_t)frame * P.img0_frame_stride;
  if (level != 0) { pitch = P.geom[level].pitch; img = P.pyr + (size_t)frame * P.pyr_fs + P.geom[level].off; }
  // Both windows are addressed from their centre pixel: the planes that take the DMA path have a dword-aligned base and pitch, so the
  // low two bits of (centre - 15) are those of X - 15, and the aligned window start follows by masking them off.
  const uint8_t *centre = img + (size_t)Y * pitch + X;
  // level 0 is the caller's buffer: when it is not dword-aligned its keypoints gather their disc bytes from global memory
  const uint32_t dmaMask = (uint32_t)__ballot(valid && ((((uintptr_t)img) | (uintptr_t)pitch) & 3u) == 0);
  const uint32_t cenLo = (uint32_t)(uintptr_t)centre, cenHi = (uint32_t)((uintptr_t)centre >> 32);

  // ---- lane only: my share of a disc window, and my two 16-byte chunks of a window (chunk idx = row 3 r + c; idx / 3 as
  // (idx * 21846) >> 16, exact below 111).
  // A window holds the disc as 31 rows of 48 bytes, disc column c = u + 15 at byte o + c of its row, o = (X - 15) & 3.  Lane L < 62
  // takes row L >> 1 and the columns 16 (L & 1) .. + 15 of it (column 31 lies outside the disc): bytes 16 (L & 1) .. + 19 of the row
  // come in with one aligned 16-byte read and one dword, four v_alignbyte_b32 by the wave-uniform o bring the 16 columns to byte 0,
  // and eight signed dot products against per-lane weights sum u * pixel and v * pixel: wu holds the column's u where (u, v) is
  // inside the disc (|u| <= umax[|v|], the definition behind c_disc) and 0 elsewhere, wv the row's v or 0.  |u|, |v| <= 15: signed bytes.
  const int drow = min(lane >> 1, 30), dhalf = lane & 1, dvv = drow - 15;
  const uint32_t rowOff = (uint32_t)(drow * 48 + 16 * dhalf);
  uint32_t wu[4], wv[4];
  {
    const int d = (int)((make_disc_umax_nibbles() >> (4 * (dvv < 0 ? -dvv : dvv))) & 15u);
    // my columns inside the disc are the bytes [first, end) of my 16: u = byte - 15 >= -d in the left half, u = byte + 1 <= d in the right
    const int first = dhalf ? 0 : 15 - d, end = lane < 62 ? (dhalf ? d : 16) : first;
    const uint32_t vrep = (uint32_t)(dvv & 0xff) * 0x01010101u;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int lo = min(max(first - 4 * i, 0), 4), hi = min(max(end - 4 * i, 0), 4);
      const uint32_t inside = (uint32_t)(0xffffffffull << (8 * lo)) & ~(uint32_t)(0xffffffffull << (8 * hi));
      auto ub = [](int u0) { return (uint32_t)(uint8_t)u0 | ((uint32_t)(uint8_t)(u0 + 1) << 8) | ((uint32_t)(uint8_t)(u0 + 2) << 16) | ((uint32_t)(uint8_t)(u0 + 3) << 24); };
      wu[i] = (dhalf ? ub(4 * i + 1) : ub(4 * i - 15)) & inside;
      wv[i] = vrep & inside;
      asm volatile("" : "+v"(wu[i]), "+v"(wv[i]));   // opaque: otherwise every keypoint re-derives them
    }
  }
  const uint32_t cr0 = ((uint32_t)lane * 21846u) >> 16, cc0 = 16u * ((uint32_t)lane - 3u * cr0);
  const uint32_t cr1 = ((uint32_t)(lane + 64) * 21846u) >> 16, cc1 = 16u * ((uint32_t)(lane + 64) - 3u * cr1);
  // nchunks (93 or 111) chunks of the window whose first row starts at row0 (uniform, dword-aligned) into staging buffer `which`.
  // Always two instructions.  The buffer's previous reads must have returned before the DMA may overwrite it.
  auto issue = [&](const uint8_t *row0, uint32_t rowPitch, int which, uint32_t nchunks) {
    uint8_t *buf = myLds + which * DESC_BUF;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(row0 + (mul24(cr0, rowPitch) + cc0)),
                                     (__attribute__((address_space(3))) void *)&buf[lane * 16], 16, 0, 0);
    if ((uint32_t)lane + 64u < nchunks)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(row0 + (mul24(cr1, rowPitch) + cc1)),
                                       (__attribute__((address_space(3))) void *)&buf[(lane + 64) * 16], 16, 0, 0);
  };
  auto centre_of = [&](uint32_t lo, uint32_t hi, int k) {
    return (uintptr_t)(uint32_t)__builtin_amdgcn_readlane((int)lo, k) | ((uintptr_t)(uint32_t)__builtin_amdgcn_readlane((int)hi, k) << 32);
  };
  auto issue_disc = [&](int k) {   // rows Y - 15 .. Y + 15, 48 bytes from the aligned column at or below X - 15
    const uintptr_t c15 = centre_of(cenLo, cenHi, k) - 15;
    const uint32_t p = (uint32_t)__builtin_amdgcn_readlane(pitch, k);
    issue(reinterpret_cast<const uint8_t *>(c15 & ~(uintptr_t)3) - 15 * (size_t)p, p, k & 1, 93u);
  };

  // ---- moments (IC_Angle).  Keypoint k's window is requested while k - 1's is read; the waits are counted: two DMA instructions
  // per window, loads retire in order.  With d = pixel - 128 as a signed byte, sum u * d differs from sum u * pixel by 128 * sum u,
  // and the disc's offsets - in either form, the row weights or c_disc's twelve pixels per lane - sum to zero over the wavefront,
  // so the signed dot products give m10 and m01 exactly.
  if (dmaMask & 1u) issue_disc(0);
  auto one = [&](auto kc, int &p10, int &p01) {
    constexpr int k = decltype(kc)::value;
    const bool nextDma = k + 1 < K && ((dmaMask >> ((k + 1) & 31)) & 1u) != 0;
    if (nextDma) issue_disc(k + 1);
    p10 = 0; p01 = 0;
    if ((validMask >> k) & 1u) {
      const uintptr_t cen = centre_of(cenLo, cenHi, k);
      if ((dmaMask >> k) & 1u) {
        if (nextDma) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // (in assembly: on a ds_read_b128 of its own making the compiler drains the DMA queue first, window k + 1 included, which
        // the counted wait above has just let travel on)
        const uint32_t rp = (uint32_t)(uintptr_t)(LdsBytes)myLds + rowOff;   // a 32-bit LDS address
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        u32x4 q;
        uint32_t q4;
        asm volatile("ds_read_b128 %0, %2 offset:%3\n\tds_read_b32 %1, %2 offset:%4\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(q), "=&v"(q4) : "v"(rp), "n"((k & 1) * DESC_BUF), "n"((k & 1) * DESC_BUF + 16) : "memory");
        const uint32_t raw[5] = {q.x, q.y, q.z, q.w, q4};
        const uint32_t o = (uint32_t)((cen - 15) & 3);
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const uint32_t d = __builtin_amdgcn_alignbyte(raw[g + 1], raw[g], o) ^ 0x80808080u;
          p10 = __builtin_amdgcn_sdot4((int)wu[g], (int)d, p10, false);
          p01 = __builtin_amdgcn_sdot4((int)wv[g], (int)d, p01, false);
        }
      } else {
        // a level 0 that is not dword-aligned (the caller's buffer): the lane's twelve disc pixels of c_disc, gathered from global
        // memory (the table is read here, inside the rare path, through an opaque copy of the lane index: read once for all keypoints,
        // its six registers would be live through the whole block)
        const uint32_t p = (uint32_t)__builtin_amdgcn_readlane(pitch, k);
        const GlobalBytes cp = (GlobalBytes)cen - (15 * (size_t)p + 15);   // the window's first pixel: uniform base, unsigned 32-bit offsets
        int tl = lane;
        asm volatile("" : "+v"(tl));
        const uint4 dw0 = *reinterpret_cast<const uint4 *>(&c_disc.w[tl][0]);
        const uint2 dw1 = *reinterpret_cast<const uint2 *>(&c_disc.w[tl][4]);
        const uint32_t uw[3] = {dw0.x, dw0.y, dw0.z}, vw[3] = {dw0.w, dw1.x, dw1.y};
        uint32_t dval[12];
#pragma unroll
        for (int t = 0; t < 12; t++)
          dval[t] = cp[(uint32_t)((int)(int8_t)(vw[t >> 2] >> (8 * (t & 3))) + 15) * p + (uint32_t)((int)(int8_t)(uw[t >> 2] >> (8 * (t & 3))) + 15)];
#pragma unroll
        for (int g = 0; g < 3; g++) {
          const uint32_t d = ((dval[4 * g] | (dval[4 * g + 1] << 8)) | ((dval[4 * g + 2] | (dval[4 * g + 3] << 8)) << 16)) ^ 0x80808080u;
          p10 = __builtin_amdgcn_sdot4((int)uw[g], (int)d, p10, false);
          p01 = __builtin_amdgcn_sdot4((int)vw[g], (int)d, p01, false);
        }
      }
    }
  };
  int r10, r01;
  tr_range<LOG, 0, K>(one, lane, r10, r01);
  // the groups' sums meet through LDS: lane k < K adds up the 64 / K entries of keypoint k
  int2 *sRed = reinterpret_cast<int2 *>(myLds + 2 * DESC_BUF);
  sRed[lane] = make_int2(r10, r01);
  int m10 = 0, m01 = 0;
  if (lane < K) {
    const int q = (int)(__builtin_bitreverse32((uint32_t)lane) >> (32 - LOG));
#pragma unroll
    for (int g = 0; g < 64 / K; g++) { const int2 v = sRed[q + K * g]; m10 += v.x; m01 += v.y; }
  }
  // the blurred patches (their addresses only now: fewer registers live across the moments); the first travels during the trigonometry
  const int bpitch = P.geom[level].bpitch;
  const uint8_t *bcentre = P.blur + (size_t)frame * P.blur_fs + P.geom[level].boff + (size_t)Y * bpitch + X;
  const uint32_t bcenLo = (uint32_t)(uintptr_t)bcentre, bcenHi = (uint32_t)((uintptr_t)bcentre >> 32);
  auto issue_patch = [&](int k, int which) {   // rows Y - 18 .. Y + 18 of the blurred plane (always dword-aligned: workspace)
    const uintptr_t c18 = centre_of(bcenLo, bcenHi, k) - 18;
    const uint32_t p = (uint32_t)__builtin_amdgcn_readlane(bpitch, k);
    issue(reinterpret_cast<const uint8_t *>(c18 & ~(uintptr_t)3) - 18 * (size_t)p, p, which, 111u);
  };
  issue_patch(__builtin_ctz(validMask), 0);

  // ---- angle and rotation, lane = keypoint (idle lanes compute on zeros); the branches inside are per lane here
  const float angle = fast_atan2_deg((float)m01, (float)m10);
  const float factorPI = (float)(3.1415926535897932384626433832795 / 180.f);
  const float arad = angle * factorPI;
  const float ca = orbsc::ref_cosf(arad), sb = orbsc::ref_sinf(arad);

  // ---- steered BRIEF, one keypoint at a time: a, b are scalar operands, the pattern stays in registers
  float pf[16];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint32_t pw = reinterpret_cast<const uint32_t *>(c_pattern)[r * 64 + lane];  // x0, y0, x1, y1 as int8
    pf[4 * r] = (float)(int8_t)(pw & 0xff); pf[4 * r + 1] = (float)(int8_t)((pw >> 8) & 0xff);
    pf[4 * r + 2] = (float)(int8_t)((pw >> 16) & 0xff); pf[4 * r + 3] = (float)(int8_t)(pw >> 24);
  }
  constexpr int bp = 48;
  int which = 0;
  for (uint32_t m = validMask; m != 0; which ^= 1) {
    const int k = __builtin_ctz(m);
    m &= m - 1;
    if (m != 0) issue_patch(__builtin_ctz(m), which ^ 1);
    const float a = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ca), k));
    const float b = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, sb), k));
    // cvRound as the bits of v + 1.5 * 2^23: for |v| < 2^22 the sum is rounded to the nearest-even integer n exactly as rint does,
    // and its low 24 bits are 2^22 + n.  The 24-bit multiply-add reads just those, so row * 48 + column costs one instruction (the
    // 32-bit multiply issues at a quarter rate) and the constant RN_BIAS too much comes off with the patch's base address.
    auto rn_bits = [](float v) { return __float_as_uint(v + 12582912.0f); };
    constexpr uint32_t RN_BIAS = 48u * 0x400000u + 0x4b400000u;
    uint32_t o0[4], o1[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const float x0 = pf[4 * r], y0 = pf[4 * r + 1], x1 = pf[4 * r + 2], y1 = pf[4 * r + 3];
      o0[r] = __umul24(rn_bits(x0 * b + y0 * a), (uint32_t)bp) + rn_bits(x0 * a - y0 * b);
      o1[r] = __umul24(rn_bits(x1 * b + y1 * a), (uint32_t)bp) + rn_bits(x1 * a - y1 * b);
    }
    // (a store of the previous keypoint may still be in flight: the count only relies on loads retiring in order among themselves)
    if (m != 0) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // patch centre (a 32-bit LDS address), less the bias of the offsets
    const uint32_t bc = (uint32_t)(uintptr_t)(LdsBytes)myLds + (uint32_t)(which * DESC_BUF + 18 * 48 + 18) + (uint32_t)((centre_of(bcenLo, bcenHi, k) - 18) & 3) - RN_BIAS;
    int v0[4], v1[4];
#pragma unroll
    for (int r = 0; r < 4; r++) { v0[r] = *(LdsBytes)(uintptr_t)(bc + o0[r]); v1[r] = *(LdsBytes)(uintptr_t)(bc + o1[r]); }
    unsigned long long bits[4];
#pragma unroll
    for (int r = 0; r < 4; r++) bits[r] = __ballot(v0[r] < v1[r]);
    const int d = __builtin_amdgcn_readlane(dst, k);
    if (d < P.cap && lane < 8) {
      const unsigned long long w = bits[lane >> 1];
      reinterpret_cast<uint32_t *>(P.out_desc + ((size_t)frame * P.cap + d) * 32)[lane] = (uint32_t)((lane & 1) ? (w >> 32) : w);
    }
  }
  // ---- the keypoint records, one per lane
  if (valid && dst < P.cap) {
    KpOut o;
    o.x = (float)X;
    o.y = (float)Y;
    if (level != 0) { const float sc = P.geom[level].scale; o.x = o.x * sc; o.y = o.y * sc; }
    o.size = P.geom[level].kpsize;
    o.angle = angle;
    o.response = (float)(packed >> 24);
    o.octave = level;
    o.class_id = -1;
    reinterpret_cast<KpOut *>(P.out_kps)[(size_t)frame * P.cap + dst] = o;
  }
}

// (the block form is held to eight wavefronts per SIMD: left alone, the scheduler spreads K = 16 over 118 registers, i.e. four)
template <int K>
__global__ __launch_bounds__(256, K == 1 ? 1 : 8) void k_describe(FrameParams P) {
  if constexpr (K == 1) describe_one(P);
  else describe_block<K>(P);
}

// cv::cvtColor(im, gray, CV_RGB2GRAY / CV_BGR2GRAY / CV_RGBA2GRAY / CV_BGRA2GRAY) as called by Tracking::GrabImage*
// (Tracking.cc:1122-1135) for 8-bit images: OpenCV's fixed-point RGB2Gray, (R*4899 + G*9617 + B*1868 + 8192) >> 14
// (R2Y, G2Y, B2Y with yuv_shift 14; alpha ignored).  Four output pixels per thread, dword store.
__global__ __launch_bounds__(256) void k_cvt_gray(const uint8_t *src, int rows, int cols, size_t sstride, int ch, int rgb, uint8_t *dst,
                                                  size_t dstride) {
  const int q = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  const int x0 = 4 * q;
  if (x0 >= cols || y >= rows) return;
  const uint8_t *s = src + (size_t)y * sstride + (size_t)x0 * ch;
  const int cr = rgb ? 0 : 2, cb = rgb ? 2 : 0;
  uint32_t packed = 0;
  const int n = min(4, cols - x0);
  for (int j = 0; j < n; j++) {
    const uint32_t g = ((uint32_t)s[j * ch + cr] * 4899u + (uint32_t)s[j * ch + 1] * 9617u + (uint32_t)s[j * ch + cb] * 1868u + 8192u) >> 14;
    packed |= g << (8 * j);
  }
  uint8_t *d = dst + (size_t)y * dstride + x0;
  if (n == 4 && ((((uintptr_t)dst) | dstride) & 3u) == 0) *reinterpret_cast<uint32_t *>(d) = packed;
  else for (int j = 0; j < n; j++) d[j] = (uint8_t)(packed >> (8 * j));
}

// cv::CLAHE::apply as the TUM-VI examples run it on every image before TrackMonocular / TrackStereo
// (Examples/Monocular/mono_tum_vi.cc:101-109, createCLAHE(3.0, Size(8, 8))), OpenCV 3.4/4.x clahe.cpp for CV_8UC1:
// per-tile histogram -> clip at clipLimit, the excess spread evenly (batch + every residualStep-th bin) -> cumulative
// LUT saturate_cast<uchar>(sum * lutScale); then every pixel blends the LUTs of its four neighbouring tiles bilinearly
// in float.  When the image size is not a multiple of the tile grid the histogram runs over the image extended to the
// next multiple with BORDER_REFLECT_101 (tw, th are the tile sizes of the extended image).
// clahe_lut_entry: bin t's histogram count v -> its LUT byte (clip, redistribution, inclusive scan, lutScale rounding).  Called by all
// 256 threads of a workgroup; hist[256] and part[4] are its LDS scratch (hist may still be read by others on entry).
__device__ __forceinline__ uint8_t clahe_lut_entry(int v, int t, int clipLimit, float lutScale, uint32_t *hist, int *part) {
  if (clipLimit > 0) {
    int excess = v > clipLimit ? v - clipLimit : 0;
    if (v > clipLimit) v = clipLimit;
    const int ws = wave_sum_i32(excess);
    if ((t & 63) == 0) part[t >> 6] = ws;
    __syncthreads();
    const int clipped = part[0] + part[1] + part[2] + part[3];
    const int redistBatch = clipped / 256;
    const int residual = clipped - redistBatch * 256;
    v += redistBatch;
    if (residual != 0) {
      const int step = max(256 / residual, 1);
      if (t % step == 0 && t / step < residual) v++;
    }
  }
  __syncthreads();
  hist[t] = (uint32_t)v;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {   // inclusive scan over the 256 bins
    const uint32_t a = t >= d ? hist[t - d] : 0u;
    __syncthreads();
    hist[t] += a;
    __syncthreads();
  }
  const int r = __float2int_rn(__fmul_rn((float)(int)hist[t], lutScale));
  return (uint8_t)min(max(r, 0), 255);
}

// k_clahe_lut: one workgroup per tile, thread b owns histogram bin b.
__global__ __launch_bounds__(256) void k_clahe_lut(const uint8_t *src, int rows, int cols, size_t sstride, int tilesX, int tw, int th, int clipLimit,
                                                   float lutScale, uint8_t *lut) {
  __shared__ uint32_t hist[256];
  __shared__ int part[4];
  const int t = threadIdx.x, tile = blockIdx.x, tx = tile % tilesX, ty = tile / tilesX;
  hist[t] = 0;
  __syncthreads();
  const int x0 = tx * tw, y0 = ty * th;
  for (int i = t; i < tw * th; i += 256) {
    int y = y0 + i / tw, x = x0 + i % tw;
    if (y >= rows) y = 2 * (rows - 1) - y;   // BORDER_REFLECT_101, the extension is narrower than the image
    if (x >= cols) x = 2 * (cols - 1) - x;
    atomicAdd(&hist[src[(size_t)y * sstride + x]], 1u);
  }
  __syncthreads();
  lut[(size_t)tile * 256 + t] = clahe_lut_entry((int)hist[t], t, clipLimit, lutScale, hist, part);
}

// Tile coordinate of pixel index v along one axis (clahe.cpp, CLAHE_Interpolation_Body): t1 / t2 the two neighbouring tiles
// (clamped), a / a1 the weights of t2 / t1.  Every product and sum is rounded on its own.  Host and device: the launch code sizes
// the staged part of the table with it.
__host__ __device__ __forceinline__ void clahe_tile_coord(int v, float inv_t, int ntiles, int &t1, int &t2, float &a, float &a1) {
#ifdef __HIP_DEVICE_COMPILE__
  const float tf = __fsub_rn(__fmul_rn((float)v, inv_t), 0.5f);
  t1 = (int)floorf(tf);
  a = __fsub_rn(tf, (float)t1);
  a1 = __fsub_rn(1.0f, a);
#else
  const float tf = (float)v * inv_t - 0.5f;
  t1 = (int)floorf(tf);
  a = tf - (float)t1;
  a1 = 1.0f - a;
#endif
  t2 = t1 + 1 < ntiles - 1 ? t1 + 1 : ntiles - 1;
  t1 = t1 > 0 ? t1 : 0;
}

// The blend of the four tables' entries for one pixel: p1 / p2 the table rows of ty1 / ty2, i1 / i2 = tx1 * 256 + value, tx2 * 256 + value.
__device__ __forceinline__ uint32_t clahe_blend(const uint8_t *p1, const uint8_t *p2, int i1, int i2, float xa, float xa1, float ya, float ya1) {
  const float top = __fadd_rn(__fmul_rn((float)p1[i1], xa1), __fmul_rn((float)p1[i2], xa));
  const float bot = __fadd_rn(__fmul_rn((float)p2[i1], xa1), __fmul_rn((float)p2[i2], xa));
  const float res = __fadd_rn(__fmul_rn(top, ya1), __fmul_rn(bot, ya));
  return (uint32_t)min(max(__float2int_rn(res), 0), 255);
}

// Dynamic LDS of the two interpolation kernels: `rows` rows of the frame's table, tilesX * 256 bytes each, copied a dword at a time.
struct ClaheCarve {
  LdsRegion<uint8_t> lut;
  int bytes;
  __host__ __device__ static constexpr ClaheCarve of(int rows, int tilesX) {
    LdsCarver c;
    ClaheCarve r{c.take<uint8_t>(rows * tilesX * 256, 4), 0};
    r.bytes = c.at;
    return r;
  }
};
// k_clahe_interp: the whole LUT (tilesX*tilesY*256 bytes, 16 KB for 8x8) sits in LDS; four pixels per thread.
// Every product and sum is rounded on its own, as the reference's scalar float expression is (no fused multiply-add).
__global__ __launch_bounds__(256) void k_clahe_interp(const uint8_t *src, int rows, int cols, size_t sstride, int tilesX, int tilesY, float inv_tw,
                                                      float inv_th, const uint8_t *lut, uint8_t *dst, size_t dstride, int rowsPerBlock) {
  extern __shared__ uint8_t smem_lut[];
  uint8_t *sLut = ClaheCarve::of(tilesY, tilesX).lut.in(smem_lut);
  const int nl = tilesX * tilesY * 256;
  for (int i = threadIdx.x * 4; i < nl; i += 1024) *reinterpret_cast<uint32_t *>(sLut + i) = *reinterpret_cast<const uint32_t *>(lut + i);
  __syncthreads();
  const int yb = blockIdx.x * rowsPerBlock, ye = min(yb + rowsPerBlock, rows);
  const int nq = (cols + 3) >> 2;
  for (int i = threadIdx.x; i < (ye - yb) * nq; i += 256) {
    const int y = yb + i / nq, xq = (i % nq) * 4;
    int ty1, ty2;
    float ya, ya1;
    clahe_tile_coord(y, inv_th, tilesY, ty1, ty2, ya, ya1);
    const uint8_t *p1 = sLut + ty1 * tilesX * 256, *p2 = sLut + ty2 * tilesX * 256;
    const uint8_t *srow = src + (size_t)y * sstride;
    uint8_t *drow = dst + (size_t)y * dstride;
    const int n = min(4, cols - xq);
    uint32_t packed = 0;
    for (int j = 0; j < n; j++) {
      const int x = xq + j;
      int tx1, tx2;
      float xa, xa1;
      clahe_tile_coord(x, inv_tw, tilesX, tx1, tx2, xa, xa1);
      const int sv = srow[x];
      packed |= clahe_blend(p1, p2, tx1 * 256 + sv, tx2 * 256 + sv, xa, xa1, ya, ya1) << (8 * j);
    }
    if (n == 4 && ((((uintptr_t)dst) | dstride) & 3u) == 0) *reinterpret_cast<uint32_t *>(drow + xq) = packed;
    else for (int j = 0; j < n; j++) drow[xq + j] = (uint8_t)(packed >> (8 * j));
  }
}

// cv::remap(im, imRect, M1, M2, cv::INTER_LINEAR) of the stereo examples (Examples/Stereo/stereo_euroc.cc:166-167), with the
// CV_32FC1 maps initUndistortRectifyMap(..., CV_32F, M1, M2) produced (:113-114) and the default BORDER_CONSTANT (0).  OpenCV
// quantises the source coordinate to 1/32 pixel (cvRound(map * INTER_TAB_SIZE)), takes the bilinear weights from a table of
// 15-bit fixed-point products -- for the linear kernel exactly 32 * (32-fx|fx) * (32-fy|fy); the one saturated entry of the table
// (fx = fy = 0: {32767, 0, 0, 1} after its correction step) yields the same pixel as {32768, 0, 0, 0} for 8-bit taps -- and rounds
// with (sum + (1 << 14)) >> 15.  A tap outside the source contributes the border value.
struct RemapEntry {
  int ix, iy;               // top-left tap, saturate_cast<short>
  int w00, w01, w10, w11;   // 15-bit weights of the taps (iy, ix), (iy, ix + 1), (iy + 1, ix), (iy + 1, ix + 1)
};

__device__ __forceinline__ RemapEntry remap_decode(float mx, float my) {
  // cvRound = cvtss2si: out-of-range and NaN inputs give INT_MIN there; __float2int_rn saturates, NaN is patched to match
  const int sx = (mx != mx || fabsf(mx) >= 67108864.0f) ? INT_MIN : __float2int_rn(__fmul_rn(mx, 32.0f));
  const int sy = (my != my || fabsf(my) >= 67108864.0f) ? INT_MIN : __float2int_rn(__fmul_rn(my, 32.0f));
  const int fx = sx & 31, fy = sy & 31;
  RemapEntry e;
  e.ix = min(max(sx >> 5, -32768), 32767);   // saturate_cast<short>
  e.iy = min(max(sy >> 5, -32768), 32767);
  e.w00 = 32 * (32 - fx) * (32 - fy); e.w01 = 32 * fx * (32 - fy); e.w10 = 32 * (32 - fx) * fy; e.w11 = 32 * fx * fy;
  return e;
}

__global__ __launch_bounds__(256) void k_remap_linear(const uint8_t *src, int srows, int scols, size_t sstride, const float *mapx, const float *mapy,
                                                      size_t mstride, int rows, int cols, uint8_t *dst, size_t dstride) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= cols || y >= rows) return;
  const RemapEntry e = remap_decode(mapx[(size_t)y * mstride + x], mapy[(size_t)y * mstride + x]);
  auto tap = [&](int yy, int xx) -> int { return ((unsigned)xx < (unsigned)scols && (unsigned)yy < (unsigned)srows) ? src[(size_t)yy * sstride + xx] : 0; };
  const int acc = tap(e.iy, e.ix) * e.w00 + tap(e.iy, e.ix + 1) * e.w01 + tap(e.iy + 1, e.ix) * e.w10 + tap(e.iy + 1, e.ix + 1) * e.w11;
  dst[(size_t)y * dstride + x] = (uint8_t)((acc + (1 << 14)) >> 15);
}

// ---- CLAHE and remap for a batch of resident frames (orbx_clahe_batch_device, orbx_remap_linear_batch_device) ----
// Same expressions as the three kernels above (clahe_lut_entry, clahe_tile_coord, clahe_blend, remap_decode), so the same bytes.
#ifndef CLAHE_BAND_ROWS
#define CLAHE_BAND_ROWS ORBX_CLAHE_BAND_ROWS
#endif
#ifndef REMAP_FRAME_CHUNK
#define REMAP_FRAME_CHUNK ORBX_REMAP_FRAME_CHUNK
#endif
#ifndef CLAHE_SUBHIST
#define CLAHE_SUBHIST 8   // sub-histograms of k_clahe_lut_batch: a multiple of its 4 wavefronts; with 8, even and odd lanes of a wavefront have their own
#endif

struct ClaheBatch {
  const uint8_t *src;
  uint8_t *dst, *lut;
  size_t sstride, sframe, dstride, dframe;
  int nframes, rows, cols, tilesX, tilesY, tw, th, clipLimit;
  float lutScale, inv_tw, inv_th;
};

// The table rows (tile rows) the image rows y0 .. y1 read in the blend: ty1 of y0 through ty2 of y1, both clamped as the blend clamps
// them.  ty1 does not decrease with y (a float product with a positive constant, a float difference and floor are all monotone).
__host__ __device__ __forceinline__ void clahe_band_lut_rows(int y0, int y1, float inv_th, int tilesY, int &first, int &count) {
  int a1, a2, b1, b2;
  float w, w1;
  clahe_tile_coord(y0, inv_th, tilesY, a1, a2, w, w1);
  clahe_tile_coord(y1, inv_th, tilesY, b1, b2, w, w1);
  first = a1;
  count = b2 - a1 + 1;
}

// k_clahe_lut_batch: grid (tile, frame), thread b owns bin b.  The part of the tile inside the image is read as aligned dwords with
// bytes at the two ends of a row; the columns of the reflect-101 extension (last tile columns only) have a loop of their own, the
// rows of the extension are a row index.  CLAHE_SUBHIST sub-histograms (each wavefront has its own), merged before the clip.
__global__ __launch_bounds__(256) void k_clahe_lut_batch(ClaheBatch P) {
  __shared__ uint32_t hist[CLAHE_SUBHIST][256];
  __shared__ int part[4];
  const int t = threadIdx.x, tile = blockIdx.x, tx = tile % P.tilesX, ty = tile / P.tilesX;
  const int x0 = tx * P.tw, y0 = ty * P.th;
  const int w = max(0, min(P.tw, P.cols - x0)), ext = P.tw - w;   // columns inside the image, columns of the extension
  const int nslot = ((w + 3) >> 2) + 1;                           // dword slots that cover a row of w bytes at any alignment
  uint32_t *h = hist[(t >> 6) * (CLAHE_SUBHIST / 4) + (t & (CLAHE_SUBHIST / 4 - 1))];
  for (int f = blockIdx.y; f < P.nframes; f += gridDim.y) {
    const uint8_t *base = P.src + (size_t)f * P.sframe;
    for (int k = 0; k < CLAHE_SUBHIST; k++) hist[k][t] = 0;
    __syncthreads();
    if (w > 0) {
      for (int i = t; i < P.th * nslot; i += 256) {
        const int r = i / nslot, k = i - r * nslot;
        int y = y0 + r;
        if (y >= P.rows) y = 2 * (P.rows - 1) - y;   // BORDER_REFLECT_101, the extension is narrower than the image
        const uint8_t *row = base + (size_t)y * P.sstride + x0;
        const int b = 4 * k - (int)((uintptr_t)row & 3u);   // first byte of this slot, relative to the row start
        if (b >= w) continue;
        if (b >= 0 && b + 4 <= w) {
          const uint32_t v = *reinterpret_cast<const uint32_t *>(row + b);
          atomicAdd(&h[v & 255u], 1u);
          atomicAdd(&h[(v >> 8) & 255u], 1u);
          atomicAdd(&h[(v >> 16) & 255u], 1u);
          atomicAdd(&h[v >> 24], 1u);
        } else {
          for (int j = max(b, 0); j < min(b + 4, w); j++) atomicAdd(&h[row[j]], 1u);
        }
      }
    }
    for (int i = t; i < P.th * ext; i += 256) {
      int y = y0 + i / ext;
      const int x = 2 * (P.cols - 1) - (x0 + w + i % ext);
      if (y >= P.rows) y = 2 * (P.rows - 1) - y;
      atomicAdd(&h[base[(size_t)y * P.sstride + x]], 1u);
    }
    __syncthreads();
    uint32_t v = 0;
    for (int k = 0; k < CLAHE_SUBHIST; k++) v += hist[k][t];
    P.lut[((size_t)f * P.tilesX * P.tilesY + tile) * 256 + t] = clahe_lut_entry((int)v, t, P.clipLimit, P.lutScale, hist[0], part);
    __syncthreads();
  }
}

// k_clahe_interp_batch: grid (band of CLAHE_BAND_ROWS rows, frame).  Only the table rows the band reads are staged in LDS
// (clahe_band_lut_rows: two inside a tile row, more when the tiles are shorter than the band).  A thread owns a quad of four columns
// and walks down the band: the column terms are computed once per quad, the row terms once per row.  With fewer quads than threads
// the threads split into row phases.
__global__ __launch_bounds__(256) void k_clahe_interp_batch(ClaheBatch P) {
  extern __shared__ uint8_t smem_lut[];
  uint8_t *sLut = ClaheCarve::of(0, P.tilesX).lut.in(smem_lut);   // (the host's count is the most rows any band stages)
  const int yb = blockIdx.x * CLAHE_BAND_ROWS, ye = min(yb + CLAHE_BAND_ROWS, P.rows);
  int first, count;
  clahe_band_lut_rows(yb, ye - 1, P.inv_th, P.tilesY, first, count);
  const int rowBytes = P.tilesX * 256, nstage = count * rowBytes;
  const int nq = (P.cols + 3) >> 2, T = (int)blockDim.x;
  const int qstep = nq >= T ? T : nq, nphase = nq >= T ? 1 : T / nq;
  const int phase = (int)threadIdx.x / qstep, q0 = (int)threadIdx.x - phase * qstep;
  for (int f = blockIdx.y; f < P.nframes; f += gridDim.y) {
    const uint8_t *lut = P.lut + ((size_t)f * P.tilesY + first) * rowBytes;
    if (((uintptr_t)P.lut & 3u) == 0)
      for (int i = threadIdx.x * 4; i < nstage; i += 4 * T) *reinterpret_cast<uint32_t *>(sLut + i) = *reinterpret_cast<const uint32_t *>(lut + i);
    else
      for (int i = threadIdx.x; i < nstage; i += T) sLut[i] = lut[i];
    __syncthreads();
    const uint8_t *sbase = P.src + (size_t)f * P.sframe;
    uint8_t *dbase = P.dst + (size_t)f * P.dframe;
    const bool salign = ((((uintptr_t)sbase) | P.sstride) & 3u) == 0, dalign = ((((uintptr_t)dbase) | P.dstride) & 3u) == 0;
    if (phase < nphase) {
      for (int q = q0; q < nq; q += qstep) {
        const int xq = 4 * q, n = min(4, P.cols - xq);
        int o1[4], o2[4];
        float xa[4], xa1[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          int tx1, tx2;
          clahe_tile_coord(xq + j, P.inv_tw, P.tilesX, tx1, tx2, xa[j], xa1[j]);
          o1[j] = tx1 * 256;
          o2[j] = tx2 * 256;
        }
        for (int y = yb + phase; y < ye; y += nphase) {
          int ty1, ty2;
          float ya, ya1;
          clahe_tile_coord(y, P.inv_th, P.tilesY, ty1, ty2, ya, ya1);
          const uint8_t *p1 = sLut + (ty1 - first) * rowBytes, *p2 = sLut + (ty2 - first) * rowBytes;
          const uint8_t *s = sbase + (size_t)y * P.sstride + xq;
          uint8_t *d = dbase + (size_t)y * P.dstride + xq;
          uint32_t sv = 0;
          if (n == 4 && salign) sv = *reinterpret_cast<const uint32_t *>(s);
          else for (int j = 0; j < n; j++) sv |= (uint32_t)s[j] << (8 * j);
          uint32_t packed = 0;
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const int v = (int)((sv >> (8 * j)) & 255u);
            if (j < n) packed |= clahe_blend(p1, p2, o1[j] + v, o2[j] + v, xa[j], xa1[j], ya, ya1) << (8 * j);
          }
          if (n == 4 && dalign) *reinterpret_cast<uint32_t *>(d) = packed;
          else for (int j = 0; j < n; j++) d[j] = (uint8_t)(packed >> (8 * j));
        }
      }
    }
    __syncthreads();
  }
}

struct RemapBatch {
  const uint8_t *src;
  uint8_t *dst;
  const float *mapx, *mapy;
  size_t sstride, sframe, mstride, dstride, dframe;
  int nframes, srows, scols, rows, cols;
};

// k_remap_linear_batch: one map pair for all frames.  grid (256-pixel run, row, chunk of REMAP_FRAME_CHUNK frames): a thread decodes
// the map entry of its output pixel once and then does only the taps, the sum and the store for every frame of the chunk.  A tap
// outside the source gets weight 0, which gives the sum the border value 0 gives.  PAIR (sources of two columns or more): the two taps
// of a source row come from ONE 16-bit load at the column pair [ixc, ixc + 1], ixc = ix clamped to [0, scols - 2], so both bytes lie
// inside the row whatever ix is; a tap in range is byte ix - ixc or ix + 1 - ixc of it (0 or 1), a row out of range reads row 0.  The
// load has byte alignment (the packed struct says so); gfx950 takes it as one global_load_ushort.  Without PAIR: four byte loads.
struct __attribute__((packed)) RemapPair { uint16_t v; };

template <bool PAIR>
__global__ __launch_bounds__(256) void k_remap_linear_batch(RemapBatch P) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= P.cols) return;
  const RemapEntry e = remap_decode(P.mapx[(size_t)y * P.mstride + x], P.mapy[(size_t)y * P.mstride + x]);
  const bool x0in = (unsigned)e.ix < (unsigned)P.scols, x1in = (unsigned)(e.ix + 1) < (unsigned)P.scols;
  const bool y0in = (unsigned)e.iy < (unsigned)P.srows, y1in = (unsigned)(e.iy + 1) < (unsigned)P.srows;
  const int w00 = x0in && y0in ? e.w00 : 0, w01 = x1in && y0in ? e.w01 : 0, w10 = x0in && y1in ? e.w10 : 0, w11 = x1in && y1in ? e.w11 : 0;
  const ptrdiff_t down = (ptrdiff_t)P.sstride;
  const size_t dpix = (size_t)y * P.dstride + x;
  const int nchunks = (P.nframes + REMAP_FRAME_CHUNK - 1) / REMAP_FRAME_CHUNK;
  if constexpr (PAIR) {
    const int ixc = min(max(e.ix, 0), P.scols - 2);
    const ptrdiff_t oT = (y0in ? (ptrdiff_t)e.iy * down : 0) + ixc, oB = (y1in ? (ptrdiff_t)(e.iy + 1) * down : 0) + ixc;
    const int sh0 = x0in ? 8 * (e.ix - ixc) : 0, sh1 = x1in ? 8 * (e.ix + 1 - ixc) : 0;
    for (int c = blockIdx.z; c < nchunks; c += gridDim.z) {
      const int f1 = min((c + 1) * REMAP_FRAME_CHUNK, P.nframes);
#pragma unroll 4
      for (int f = c * REMAP_FRAME_CHUNK; f < f1; f++) {
        const uint8_t *s = P.src + (size_t)f * P.sframe;
        const uint32_t vT = reinterpret_cast<const RemapPair *>(s + oT)->v, vB = reinterpret_cast<const RemapPair *>(s + oB)->v;
        const int acc = (int)((vT >> sh0) & 255u) * w00 + (int)((vT >> sh1) & 255u) * w01 + (int)((vB >> sh0) & 255u) * w10 + (int)((vB >> sh1) & 255u) * w11;
        P.dst[(size_t)f * P.dframe + dpix] = (uint8_t)((acc + (1 << 14)) >> 15);
      }
    }
  } else {
    const ptrdiff_t off = (ptrdiff_t)e.iy * down + e.ix;
    const ptrdiff_t o00 = x0in && y0in ? off : 0, o01 = x1in && y0in ? off + 1 : 0, o10 = x0in && y1in ? off + down : 0, o11 = x1in && y1in ? off + down + 1 : 0;
    for (int c = blockIdx.z; c < nchunks; c += gridDim.z) {
      const int f1 = min((c + 1) * REMAP_FRAME_CHUNK, P.nframes);
#pragma unroll 4
      for (int f = c * REMAP_FRAME_CHUNK; f < f1; f++) {
        const uint8_t *s = P.src + (size_t)f * P.sframe;
        const int acc = (int)s[o00] * w00 + (int)s[o01] * w01 + (int)s[o10] * w10 + (int)s[o11] * w11;
        P.dst[(size_t)f * P.dframe + dpix] = (uint8_t)((acc + (1 << 14)) >> 15);
      }
    }
  }
}
