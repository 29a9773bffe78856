// orb_ref_voc.h -- DBoW2's TemplatedVocabulary<FORB::TDescriptor, FORB>::transform(features, BowVector, FeatureVector, levelsup)
// (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1126-1194 over :1217-1259) as Frame::ComputeBoW (Frame.cc:828-835) and
// KeyFrame::ComputeBoW (KeyFrame.cc:100-110) call it, stated once for the host entry orbv_transform_host and the kernels of
// orb_voc_kernels.h.  Held against that text itself, compiled unmodified (oracle/ref_voc_driver.cc; tests/test_ref_voc.py for the host
// entry, tests/test_gpu_ref_voc.py for the kernels), besides the literal model of tests/voc_model.py.  Integer arithmetic in the descent, IEEE-754 double `+=`, fabs and `/=` in the reference's order in the assembly,
// no contraction; no libm call and no OpenCV primitive is involved.
//
// The vocabulary is held re-laid so that the children of a node are contiguous ("entries"; entry 0 is the root):
//   desc[e][8]   the node's descriptor as eight dwords
//   rec[e]       {first child entry, child count, original node id, word id}
//   weight[e]    the node's weight (a double, as loaded)
// Children keep the order of Node::children, which the loader fills by push_back in ascending node id (:1385-1392).  A node ends the
// descent when it has no children (Node::isLeaf() is children.empty(), :328), whatever its leaf flag said; its word id is the one the
// loader counted over the flagged nodes (:1408-1415), or 0 (Node(), :316) for a childless node that was not flagged.  That is why the
// weight is kept per entry and not per word: such a node answers "word 0" with its OWN weight.
//
// Descent (:1217-1259): from the root, at every level the child with the smallest FORB::distance (FORB.cpp:81-101, a popcount over the
// 256 bits), the FIRST of equal distances by the strict `<` of :1244, in children order; until a node without children.  *nid is the
// node chosen at level m_L - levelsup (:1226, :1251), or 0 when that level is <= 0 (:1227).
// Assembly (:1145-1193, BowVector.cpp:34-84, FeatureVector.cpp:31-45): a feature with w > 0 enters both containers, in ascending
// feature order; TF_IDF / TF add with addWeight (`second += w`, the first feature of a word inserts w), IDF / BINARY with
// addIfNotExist (the first feature's w stays).  Then, for TF_IDF / TF under a scoring that does not normalise (DOT_PRODUCT),
// `second /= (double)v.size()` (:1164-1170); under every other scoring BowVector::normalize(L1): `norm += fabs(second)` in ascending
// word order, one add after another, and `second /= norm` when norm > 0.
//
// Settled here:
//   * L2_NORM scoring (type 1) is REFUSED.  No configuration of the reference uses it, and it would need a device sqrt proven equal to
//     glibc's.
//   * A vocabulary with a childless node of weight > 0 above level m_L - levelsup is REFUSED for that levelsup: the reference leaves
//     *nid unset there (:1251 never fires) and FeatureVector::addFeature (:1160, :1188) reads an uninitialised NodeId.  A childless
//     node of weight <= 0 above that level is harmless - a feature that ends there is stopped (:1157, :1185) and its NodeId is never
//     read - and is accepted.  The node that the loader makes of each trailing empty line (:1378-1420) has weight 0 (Node()) wherever
//     it hangs, so a vocabulary loaded from a file that ends in a newline works as it does in the reference.  Where it hangs is not
//     the text's choice: `>> pid` and `>> nIsLeaf` fail at the stream's sentry and store nothing, so both are indeterminate reads.
//     Compiled with g++ -std=c++11 -O2 (oracle/_ref/libref_voc.so, tests/test_ref_voc.py) it is a child of the previous line's
//     parent, flagged as a leaf, with a word id of its own; nothing here depends on that.  node_of_feature of a stopped feature that
//     ends above the level is 0 here, unset there.
//   * An empty vocabulary (no word, :1134) gives two empty containers.
#pragma once
#include <stdint.h>

#define ORB_REF __host__ __device__ __forceinline__

// WeightingType and ScoringType of BowVector.h:39-56
enum { VOC_TF_IDF = 0, VOC_TF = 1, VOC_IDF = 2, VOC_BINARY = 3 };
enum { VOC_L1_NORM = 0, VOC_L2_NORM = 1, VOC_CHI_SQUARE = 2, VOC_KL = 3, VOC_BHATTACHARYYA = 4, VOC_DOT_PRODUCT = 5 };

struct alignas(16) VocRec { int32_t first, count; uint32_t node, word; };   // 16 bytes: one load

// mustNormalize (ScoringObject.h:74-89): every scoring but DOT_PRODUCT normalises; L1 for all of those this file accepts
ORB_REF bool voc_must_normalize(int scoring) { return scoring != VOC_DOT_PRODUCT; }
// `m_weighting == TF || m_weighting == TF_IDF` (:1145): addWeight, else addIfNotExist
ORB_REF bool voc_adds_weight(int weighting) { return weighting == VOC_TF || weighting == VOC_TF_IDF; }

// FORB::distance (FORB.cpp:81-101): the bit count of the xor, eight dwords
ORB_REF int voc_distance(const uint32_t *a, const uint32_t *b) {
  int d = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
#ifdef __HIP_DEVICE_COMPILE__
    d += __popc(a[k] ^ b[k]);
#else
    d += __builtin_popcount(a[k] ^ b[k]);
#endif
  }
  return d;
}

// The choice among up to 16 children at positions base .. base + 15: distance above position, so the smallest key is the first minimum
ORB_REF uint32_t voc_key(int dist, int pos16) { return ((uint32_t)dist << 8) | (uint32_t)pos16; }
// `if (d < best_d)` (:1244) of a round's smallest key against the running choice: an equal distance of a later round loses
ORB_REF void voc_take(uint32_t round_key, int base, uint32_t *best_d, int *best_pos) {
  if ((round_key >> 8) < *best_d) { *best_d = round_key >> 8; *best_pos = base + (int)(round_key & 255u); }
}
#define VOC_NO_CHILD 0xffffffffu   // above every key and every distance

// :1217-1259 for one descriptor, one child after another
ORB_REF void voc_descend(const uint32_t *desc, const VocRec *rec, const uint32_t *q, int nid_level, int32_t *entry, uint32_t *nid) {
  int cur = 0, level = 0;
  uint32_t node = 0;   // :1227
  VocRec r = rec[0];
  while (r.count > 0) {
    ++level;
    uint32_t best_d = VOC_NO_CHILD;
    int best_pos = 0;
    for (int c = 0; c < r.count; c++) voc_take(voc_key(voc_distance(q, desc + 8 * (size_t)(r.first + c)), c & 15), c & ~15, &best_d, &best_pos);
    cur = r.first + best_pos;
    r = rec[cur];
    if (level == nid_level) node = r.node;   // :1251
  }
  *entry = cur;
  *nid = node;
}

// BowVector::addWeight / addIfNotExist on the value of one word: `first` = the word is not in the map yet
ORB_REF void voc_add(double *second, double w, bool first, bool adds) {
  if (first) *second = w;          // insert(vit, value_type(id, v))
  else if (adds) *second += w;     // vit->second += v
}
// one step of `norm += fabs(it->second)` (BowVector.cpp:69-70)
ORB_REF void voc_l1_step(double *norm, double second) { *norm += fabs(second); }
// `vit->second /= nd` (:1169) and `it->second /= norm` (BowVector.cpp:82): an IEEE division
ORB_REF double voc_div(double second, double by) { return second / by; }

#undef ORB_REF
