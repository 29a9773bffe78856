// orb_common.h -- shared host/device structures of liborbhip (not part of the public ABI).
#pragma once
#include <stdint.h>
#include <stddef.h>

#define ORB_EDGE_THRESHOLD 19  // ORBextractor.cc:72
#define ORB_PATCH_SIZE 31      // ORBextractor.cc:70
#define ORB_HALF_PATCH 15      // ORBextractor.cc:71
#define ORB_MIN_BORDER 16      // EDGE_THRESHOLD-3, ORBextractor.cc:771
#define ORB_DISC_PIXELS 749    // pixels of the radius-15 disc given by umax (ORBextractor.cc:452-467)
#define ORB_MAXL 16

// FAST cell tile in LDS: interior <= 59x59 (wCell = ceil(width/floor(width/30)) < 60), +3 px ring.  The pitch is five
// 16-byte chunks: the tile is filled by global_load_lds_dwordx4, whose LDS image is lane-linear (no padding between rows).
#define FAST_TILE_PITCH 80
#define FAST_TILE_COLS 65      // widest cell window (interior 59 + 6)
#define FAST_TILE_ROWS 76      // tallest group window: two cells of up to 35 rows + 6 (a single cell: up to 59 + 6)
#define FAST_S_PITCH 64  // score plane incl. 1-px zero ring: <= 61 columns

// k_fast's group records (orbx_configure): one per group of up to 2 x 2 neighbouring cells, everything the workgroup needs about
// the group and its cells, so that a group costs one round trip of scalar loads.  128 bytes, aligned to 128.
//   group part, words 0-7:  tileX | tileY << 16;  tile width | height << 8 | level << 16 | (any valid cell) << 24;  cells in the group;
//                           level pitch;  level plane offset, low and high word (level 0: the caller's image, kernel arguments);
//                           slots per cell;  0
//   cell w, words 8+4w ..:  iniX | iniY << 16;  window width | height << 8 | (inside the detection rectangle) << 24;
//                           first slot of the cell in a frame's slot array;  cell index in a frame's cell table
// (cj * wCell, ci * hCell of the packed output coordinates are iniX, iniY - ORB_MIN_BORDER.)  Cells the group does not have: zeros.
#define FAST_REC_WORDS 32
#define FAST_REC_GROUP_WORDS 8
#define FAST_REC_CELL_WORDS 4

// k_resize's row-tile records (orbx_configure): one per (level >= 1, tile of resizeRows output rows), everything the two-pass form
// needs of the y table, so that a tile costs one scalar load in front of its staging.  272 bytes, aligned to 16.
//   group part, words 0-3:  first source row of the tile (clamped);  source rows it stages;  output rows it has;  its first output row
//   row r, words 4+4r ..:   byte offset of the row's upper and of its lower source row in the T plane, (sy - first source row) * tPitch;
//                           b0 | b1 << 16;  byte offset of output row dy0 + r in the level plane
// Rows the tile does not have: zeros.
#define RESIZE_ROWS_MAX 16
#define RESIZE_REC_GROUP_WORDS 4
#define RESIZE_REC_WORDS (RESIZE_REC_GROUP_WORDS + 4 * RESIZE_ROWS_MAX)

// k_blur's tile records (orbx_configure), 8 words: x0 | y0 << 16;  level | flags;  w | h << 16;  pitch | bpitch << 16;  level plane
// offset, low and high word;  blurred plane offset, low and high word.  Flags, from the level's geometry alone:
#define BLUR_TILE_INTERIOR 0x100u       // input rows y0 - 3 .. y0 + 66 and the eleven 16-byte chunks from column x0 - 16 all lie inside the
                                        // level (inside its pitch; level 0: inside its width), and no stored output needs a column outside it
#define BLUR_TILE_WHOLE_STORES 0x200u   // every 16-byte segment of the tile's outputs that starts inside the level ends inside bpitch

// k_describe: keypoint slots per wavefront in batch calls (few-frame calls: 1), and the workgroups (four wavefronts) a frame's totalKp
// slots then take; at least one, which writes the frame's totals.  4, 8 or 16: 8 measured best (open item 6).
#ifndef ORB_DESCRIBE_K
#define ORB_DESCRIBE_K 8
#endif
#define ORB_DESCRIBE_GROUPS(totalKp, K) ((((totalKp) + (K) - 1) / (K) + 3) / 4 > 1 ? (((totalKp) + (K) - 1) / (K) + 3) / 4 : 1)

// Live counts of ragged batches.  A count from device memory is whatever an earlier kernel (or the caller) left there, so every kernel
// takes it into [0, cap] - cap: what the host sized the problem's arrays and scratch for - before it indexes anything with it:
__host__ __device__ constexpr int clamp_count(int n, int cap) { return (n > 0 ? n : 0) < cap ? (n > 0 ? n : 0) : cap; }   // min(max(n, 0), cap)
static_assert(clamp_count(-1, 8) == 0 && clamp_count(0, 8) == 0 && clamp_count(5, 8) == 5 && clamp_count(8, 8) == 8 && clamp_count(9, 8) == 8, "clamp_count");
static_assert(clamp_count(-1, 0) == 0 && clamp_count(0, 0) == 0 && clamp_count(1, 0) == 0, "clamp_count: cap == 0");

// The live count of problem p of one side of a ragged batch: dev[p * stride] taken into [0, cap], or - dev == NULL - the constant
// the host validated, as it is.  p comes from blockIdx, so the read is a scalar load: kernels resolve it once, at the top.
struct LiveCount {
  const int32_t *dev; int stride; int konst;
  __device__ __forceinline__ int at(int p, int cap) const { return dev ? clamp_count(dev[(size_t)p * stride], cap) : konst; }
};

// k_octree's code form: the rounds run on nodes that know their cell (depth, ix, iy) of the split grid, down to depth OCT_D
// (tools/octree_depth_counts.py: the deepest split seen on the bench's streams plus one).  16-bit key counts of every cell of depths
// OCT_D .. 0, leaves first: depth d starts at entry OCT_PYR_OFF(nIni, d) and holds nIni << 2d cells, cell (ix, iy) at (ix << d) + iy.
#define OCT_D 5
#define OCT_PYR_OFF(nIni, d) ((uint32_t)(nIni) * (((1u << (2 * OCT_D + 2)) - (4u << (2 * (d)))) / 3u))
#define OCT_TABLE_BYTES(nIni) ((size_t)((2u * OCT_PYR_OFF(nIni, 0) + 2u * (uint32_t)(nIni) + 3u) & ~3u))

// Geometry of one pyramid level; filled on the host (orbx_configure), read by every kernel.
struct LevelGeom {
  int w, h;          // level image size (ORBextractor.cc:1192-1193)
  int pitch;         // bytes per row of the level plane in the workspace
  int bpitch;        // bytes per row of the blurred plane
  size_t off;        // byte offset of the level plane inside one frame's pyramid block (level 0: unused)
  size_t boff;       // byte offset of the blurred plane inside one frame's blur block
  // FAST cell grid (ORBextractor.cc:771-785)
  int maxBorderX, maxBorderY;
  int nCols, nRows, wCell, hCell;
  int cellCap;       // slots per cell = ceil(wCell/2)*ceil(hCell/2): no two 8-neighbours are both strict maxima
  int cellBase;      // index of this level's first cell in a frame's cell table
  int slotBase;      // index of this level's first slot in a frame's slot array
  // octree (ORBextractor.cc:537-761)
  int N;             // mnFeaturesPerLevel[level]
  int nIni;          // round(width/height), :541
  float hX;          // :543
  int candBase;      // first dense candidate of this level in a frame's candidate arrays
  int candCap;
  int kpBase, kpCap; // level keypoint arrays (octree output)
  int octTabX, octTabY; // first byte of this level's column / row code table in FrameParams::octTab (k_octree's code form)
  float scale;       // mvScaleFactor[level]
  float kpsize;      // (float)(int)(PATCH_SIZE*scale), :862
  // resize tables (level >= 1): index into xtab/ytab
  int xtabBase, ytabBase;
  int resizeRows;    // output rows per k_resize workgroup of this level: 16, or 8 when the 16-row LDS stage would not fit (host)
  int resizeSrcRows; // most source rows any resizeRows-row tile of this level reads (host: sizes k_resize's LDS stage)
  int resizeTPitch;  // bytes per row of k_resize's LDS plane of horizontally interpolated rows; 0: the level takes the one-pass form (host)
  int resizeRecBase; // index of this level's first row-tile record in resizeRecs
  // blur tiles
  int tilesX, tilesY, tileBase;
  uint32_t rowTileMagic;  // floor(2^32 / row tiles of k_resize), see xcd_map
};

// k_pyramid_chain (single-frame calls): one record per 32x32 output tile of a level L >= 1.  rect[l] = the rectangle of level l
// (l < L: everything the tile needs of that level, derived on the host from the resize tables; l = L: the tile itself).
#define CHAIN_TILE 32
#define CHAIN_NT 1024
struct ChainTile {
  uint16_t level, pad;
  uint16_t x[ORB_MAXL], y[ORB_MAXL], w[ORB_MAXL], h[ORB_MAXL];
};

struct FrameParams {
  LevelGeom geom[ORB_MAXL];  // by value: lives in the kernarg segment, so every geometry access is a scalar load
  int nlevels;
  int nframes;
  int iniTh, minTh;
  int lap0, lap1;
  // level 0 = caller's images
  const uint8_t *img0;
  size_t img0_stride, img0_frame_stride;
  // workspace (per-frame strides in elements of the pointed type)
  uint8_t *pyr;    size_t pyr_fs;
  uint8_t *blur;   size_t blur_fs;
  uint32_t *cellCnt; int cell_fs;
  uint32_t *slots;   size_t slot_fs;
  uint32_t *cand;    int cand_fs;   // packed (S<<24 | y<<12 | x), detection-rectangle coordinates
  uint16_t *knode;                  // node id per candidate (same indexing as cand)
  uint32_t *lkp;     int lkp_fs;    // octree output, packed like cand, list order
  uint16_t *lrank;                  // bit15 = inside lapping area, bits0..14 = rank among same class in the level
  int32_t *lcnt;                    // [frame][nlevels][2] = {count, lapped count}
  int32_t *candCnt;                 // [frame][nlevels] dense candidate count
  const int2 *xtab, *ytab;          // resize tables {src index, a0 | a1<<16}
  const int8_t *disc;               // ORB_DISC_PIXELS x (u, v)
  const uint32_t *tiles;            // blur tile records, 8 words each (above)
  uint32_t magicCells, magicTiles, magicKpBlk;  // floor(2^32 / items per frame) of k_fast, k_blur, k_describe (xcd_map)
  int totalTiles;                   // blur tiles per frame
  int totalCells;                   // FAST cells per frame
  int totalGroups;                  // k_fast workgroups per frame: groups of up to 2 x 2 neighbouring cells
  uint32_t magicGroups;             // floor(2^32 / totalGroups), xcd_map
  const uint32_t *fastRecs;         // k_fast's group records, FAST_REC_WORDS each (above), same for every frame; written by the host only
  const uint32_t *resizeRecs;       // k_resize's row-tile records, RESIZE_REC_WORDS each (above), same for every frame; written by the host only
  int totalKp;                      // sum of kpCap
  int octCap;                       // node capacity of the octree kernel
  int octHead;                      // bytes of k_octree's first LDS region (chcnt / chpos; the code form's counts and map): >= 32 * octCap
  const uint8_t *octTab;            // k_octree's code tables (LevelGeom::octTabX / octTabY), written by the host only; NULL: the per-key rounds
  const ChainTile *chain;           // k_pyramid_chain's tile records
  int chainBuf0, chainBuf1;         // bytes of its two LDS level buffers (even / odd levels)
  // outputs
  void *out_kps;       // orbx_keypoint_t [nframes][cap]
  uint8_t *out_desc;   // [nframes][cap][32]
  int32_t *out_counts; // [nframes][2]
  int cap;
};
