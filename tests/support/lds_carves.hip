// Host program of tests/test_lds_carves.py: prints the dynamic-LDS carves of the kernel headers, the very types the kernels take their
// pointers from and the host sizes its launches with.  It launches nothing and calls nothing of the HIP runtime.
// One request per line on stdin, one answer line each: "<request> | <region>:<off>:<size>:<align>:<over> ... | <bytes>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include "orbhip.h"   // the public header first, as the library does
#include "orb_kernels.h"
#include "orb_match_kernels.h"
#include "orb_sort.h"

static std::string g_line;
template <typename T>
static void region(const char *name, const LdsRegion<T> &r) {
  char buf[128];
  static uint8_t block[1 << 21];   // stands in for the LDS block: in() must be base + off for every element type
  if (r.off >= 0 && r.off <= (int)sizeof block && reinterpret_cast<uint8_t *>(r.in(block)) != block + r.off) {
    fprintf(stderr, "lds_carves: %s: in() is not base + off\n", name);
    exit(3);
  }
  snprintf(buf, sizeof buf, " %s:%d:%d:%d:%d", name, r.off, r.size(), r.align, (int)r.over);
  g_line += buf;
}
#define R(c, member) region(#member, (c).member)

int main() {
  char req[256];
  while (fgets(req, sizeof req, stdin)) {
    req[strcspn(req, "\n")] = 0;
    int a = 0, b = 0, c = 0, d = 0, bytes = -1;
    char kind[32] = "";
    if (sscanf(req, "%31s %d %d %d %d", kind, &a, &b, &c, &d) < 1) continue;
    g_line.clear();
    const std::string k = kind;
    if (k == "resolve") {   // maxn, partner table, records in LDS, fused
      const ResolveCarve v = ResolveCarve::of(a, b != 0, c != 0, d != 0);
      R(v, desc); R(v, meta); R(v, owner); R(v, slot); R(v, perm); R(v, partner); R(v, oct); R(v, rank);
      bytes = v.bytes;
    } else if (k == "form") {   // maxn, partner table, fused allowed but for LDS -> the host's decision
      const ResolveForm f = resolve_form(a, b != 0, c != 0);
      char buf[64];
      snprintf(buf, sizeof buf, " ldscand:%d fused:%d refused:%d", (int)f.ldscand, (int)f.fused, (int)(f.bytes > RESOLVE_LDS_MAX));
      g_line = buf;
      bytes = f.bytes;
    } else if (k == "init") {   // maxn
      const InitResolveCarve v = InitResolveCarve::of(a);
      R(v, vmd);
      bytes = v.bytes;
    } else if (k == "walk") {   // capn, scan mode, lanes per query; the host's u_right rule is the mode's own here
      const WalkCarve<Key32::T> v = WalkCarve<Key32::T>::of(a, walk_needs_ur(b), c);
      R(v, cell); R(v, rec); R(v, ur); R(v, list); R(v, merge);
      bytes = v.bytes;
    } else if (k == "resize") {   // source rows, source width, padded level width, two-pass
      const ResizeCarve v = ResizeCarve::of(a, resize_row_bytes(b), d ? resize_t_pitch(c) : 0, c);
      R(v, rows); R(v, t); R(v, rowRec); R(v, xtab);
      bytes = v.bytes;
    } else if (k == "chain") {   // bytes of the two level buffers, table entries
      const ChainCarve v = ChainCarve::of(a, b, c);
      R(v, buf0); R(v, buf1); R(v, tab);
      bytes = v.bytes;
    } else if (k == "clahe") {   // table rows, tiles per row
      const ClaheCarve v = ClaheCarve::of(a, b);
      R(v, lut);
      bytes = v.bytes;
    } else if (k == "octree") {   // nodes, head bytes, threads, cells (0: offsets in global memory)
      const OctreeCarve v = OctreeCarve::of(a, b, c, d);
      R(v, chcnt); R(v, chpos); R(v, best); R(v, pyr); R(v, nodeA); R(v, nodeB); R(v, cntA); R(v, cntB); R(v, npos); R(v, rankOf); R(v, codeA); R(v, codeB);
      R(v, incl); R(v, sflag); R(v, sw); R(v, cellOff);
      bytes = v.bytes;
    } else if (k == "sort") {   // keys
      const SortCarve v = SortCarve::of(a);
      R(v, keys);
      bytes = v.bytes;
    } else if (k == "consts") {   // the named bounds and the constants the test's restated formulas use
      char buf[512];
      snprintf(buf, sizeof buf, " ORB_LDS_LIMIT:%d RESOLVE_LDSCAND_MAX:%d RESOLVE_FUSED_MAX:%d RESOLVE_LDS_MAX:%d OCT_LDS_MAX:%d OCT_CELLS_LDS_MAX:%d OCT_GROWN_HEAD_MAX:%d "
               "CHAIN_LDS_MAX:%d RESIZE_STAGE_MAX:%d RESIZE_LDS_MAX:%d GRID_CELLS:%d MATCH_NT:%d MATCH_TOPK:%d WALK_LIST:%d WALK_MAX_N:%d RESIZE_ROWS_MAX:%d "
               "ORBM_MAX_KEYPOINTS:%d",
               ORB_LDS_LIMIT, RESOLVE_LDSCAND_MAX, RESOLVE_FUSED_MAX, RESOLVE_LDS_MAX, OCT_LDS_MAX, OCT_CELLS_LDS_MAX, OCT_GROWN_HEAD_MAX, CHAIN_LDS_MAX, RESIZE_STAGE_MAX,
               RESIZE_LDS_MAX, GRID_CELLS, MATCH_NT, MATCH_TOPK, WALK_LIST, WALK_MAX_N, RESIZE_ROWS_MAX, ORBM_MAX_KEYPOINTS);
      g_line = buf;
      bytes = 0;
    } else {
      fprintf(stderr, "lds_carves: unknown request '%s'\n", req);
      return 2;
    }
    printf("%s |%s | %d\n", req, g_line.c_str(), bytes);
  }
  return 0;
}
