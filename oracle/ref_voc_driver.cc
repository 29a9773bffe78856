/*
 * ref_voc_driver.cc -- extern "C" face of libref_voc.so (TEST INFRASTRUCTURE).
 *
 * libref_voc.so = the reference's own Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h (instantiated here for FORB), FORB.cpp, BowVector.cpp,
 * FeatureVector.cpp, ScoringObject.cpp and DUtils/Random.cpp, Timestamp.cpp, compiled unmodified against the stand-in headers of
 * oracle/ref_cam_shim, plus this file.  The reference's text is read from $(ORB_REFERENCE) at build time and is never copied into this
 * repository.  This file includes nothing of the product, of orb_oracle.c or of tests/, and the library links neither.
 *
 * What is pinned: loadFromTextFile (TemplatedVocabulary.h:1338-1424), transform(features, BowVector, FeatureVector, levelsup)
 * (:1126-1194), the single-feature transform under it (:1217-1259), FORB::fromString / FORB::distance, BowVector::addWeight /
 * addIfNotExist / normalize, FeatureVector::addFeature, the scoring objects' mustNormalize, and the iteration order of the two std::maps.
 *
 * What is ours: a subclass that reads the protected m_nodes / m_words and calls the protected single-feature transform; the flattening
 * of the two maps; and bodies for the cv::FileStorage family, which the stand-in header only declares.  The class template's virtual
 * save / load name them, so they must exist at link time; no pinned member reaches them, and each aborts with its name.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "Thirdparty/DBoW2/DBoW2/FORB.h"
#include "Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h"

/* ---- cv::FileStorage and its nodes: never reached ------------------------------------------------------------------------------- */
#define REFV_NOT_REACHED(name)                                                                      \
  do {                                                                                              \
    fprintf(stderr, "ref_voc_driver: %s is reached by no pinned member and has no body\n", name); \
    abort();                                                                                        \
  } while (0)

namespace cv {
FileNodeIterator &FileNodeIterator::operator++() { REFV_NOT_REACHED("FileNodeIterator::operator++"); }
FileNode FileNodeIterator::operator*() const { REFV_NOT_REACHED("FileNodeIterator::operator*"); }
bool FileNodeIterator::operator!=(const FileNodeIterator &) const { REFV_NOT_REACHED("FileNodeIterator::operator!="); }
FileNode FileNode::operator[](const char *) const { REFV_NOT_REACHED("FileNode::operator[]"); }
FileNode FileNode::operator[](const std::string &) const { REFV_NOT_REACHED("FileNode::operator[]"); }
FileNode FileNode::operator[](int) const { REFV_NOT_REACHED("FileNode::operator[]"); }
FileNode::operator int() const { REFV_NOT_REACHED("FileNode::operator int"); }
FileNode::operator float() const { REFV_NOT_REACHED("FileNode::operator float"); }
FileNode::operator double() const { REFV_NOT_REACHED("FileNode::operator double"); }
FileNode::operator std::string() const { REFV_NOT_REACHED("FileNode::operator string"); }
bool FileNode::empty() const { REFV_NOT_REACHED("FileNode::empty"); }
size_t FileNode::size() const { REFV_NOT_REACHED("FileNode::size"); }
int FileNode::type() const { REFV_NOT_REACHED("FileNode::type"); }
bool FileNode::isSeq() const { REFV_NOT_REACHED("FileNode::isSeq"); }
FileNodeIterator FileNode::begin() const { REFV_NOT_REACHED("FileNode::begin"); }
FileNodeIterator FileNode::end() const { REFV_NOT_REACHED("FileNode::end"); }
FileStorage::FileStorage() { REFV_NOT_REACHED("FileStorage::FileStorage"); }
FileStorage::FileStorage(const std::string &, int) { REFV_NOT_REACHED("FileStorage::FileStorage"); }
bool FileStorage::isOpened() const { REFV_NOT_REACHED("FileStorage::isOpened"); }
void FileStorage::release() { REFV_NOT_REACHED("FileStorage::release"); }
FileNode FileStorage::operator[](const char *) const { REFV_NOT_REACHED("FileStorage::operator[]"); }
FileNode FileStorage::operator[](const std::string &) const { REFV_NOT_REACHED("FileStorage::operator[]"); }
template <typename T> FileStorage &operator<<(FileStorage &, const T &) { REFV_NOT_REACHED("operator<<(FileStorage)"); }
template <typename T> void operator>>(const FileNode &, T &) { REFV_NOT_REACHED("operator>>(FileNode)"); }
}  // namespace cv

namespace {

typedef DBoW2::TemplatedVocabulary<DBoW2::FORB::TDescriptor, DBoW2::FORB> Base;

/* m_nodes, m_words and the single-feature transform are protected members of the template */
class Voc : public Base {
 public:
  typedef Base::Node NodeRec;
  size_t n_nodes() const { return m_nodes.size(); }
  size_t n_words() const { return m_words.size(); }
  int k() const { return m_k; }
  int L() const { return m_L; }
  int weighting() const { return (int)m_weighting; }
  int scoring() const { return (int)m_scoring; }
  const NodeRec &node(size_t i) const { return m_nodes[i]; }
  void one(const cv::Mat &feature, DBoW2::WordId &id, DBoW2::WordValue &w, DBoW2::NodeId *nid, int levelsup) const {
    Base::transform(feature, id, w, nid, levelsup);
  }
};

void to_mats(const uint8_t *desc, int n, std::vector<cv::Mat> &out) {
  out.resize((size_t)(n > 0 ? n : 0));
  for (int i = 0; i < n; i++) {
    out[i].create(1, 32, CV_8U);
    memcpy(out[i].ptr<unsigned char>(), desc + 32 * (size_t)i, 32);
  }
}

}  // namespace

extern "C" {

/* loadFromTextFile(path) on a fresh vocabulary: the handle, or NULL where the loader returned false */
void *refv_load(const char *path) {
  Voc *v = new Voc();
  if (!v->loadFromTextFile(std::string(path))) {
    delete v;
    return NULL;
  }
  return v;
}

void refv_destroy(void *h) { delete (Voc *)h; }

/* out[6] = {m_k, m_L, m_weighting, m_scoring, m_nodes.size(), size()} */
void refv_params(const void *h, int32_t *out) {
  const Voc *v = (const Voc *)h;
  out[0] = v->k();
  out[1] = v->L();
  out[2] = v->weighting();
  out[3] = v->scoring();
  out[4] = (int32_t)v->n_nodes();
  out[5] = (int32_t)v->size();
}

/* m_nodes in id order, each array [m_nodes.size()] (desc [..][32]); returns the count, or -1 where a node's id is not its index or its
   descriptor is not a 1 x 32 byte row (node 0, the root, has the empty matrix the loader left it: its 32 bytes are written as 0).
   flagged[i] = 1 where the loader took the `nIsLeaf > 0` branch for node i, 0 where it did not, 2 where that cannot be told.  It is
   told from word_id alone (m_words holds pointers that a reallocation of m_nodes leaves dangling; they are not followed): the flagged
   nodes carry 0, 1, 2, .. in id order and every other node carries 0, so a non-zero word_id settles it, and so does a zero one after
   word 0 is taken.  Among the nodes before word 1 that carry 0, word 0 is the only one without children, if there is exactly one. */
int refv_nodes(const void *h, uint32_t *parent, int32_t *n_children, uint32_t *word_id, double *weight, uint8_t *desc, uint8_t *flagged) {
  const Voc *v = (const Voc *)h;
  const size_t n = v->n_nodes();
  const size_t n_words = v->n_words();
  for (size_t i = 0; i < n; i++) {
    const Voc::NodeRec &nd = v->node(i);
    if (nd.id != (DBoW2::NodeId)i) return -1;
    parent[i] = nd.parent;
    n_children[i] = (int32_t)nd.children.size();
    word_id[i] = nd.word_id;
    weight[i] = nd.weight;
    if (nd.descriptor.empty()) {
      if (i != 0) return -1;
      memset(desc + 32 * i, 0, 32);
    } else {
      if (nd.descriptor.rows != 1 || nd.descriptor.cols != 32 || nd.descriptor.type() != CV_8U) return -1;
      memcpy(desc + 32 * i, nd.descriptor.ptr<unsigned char>(), 32);
    }
    flagged[i] = 0;
  }
  size_t first_nonzero = n; /* the node that carries word 1 */
  for (size_t i = 1; i < n && first_nonzero == n; i++)
    if (word_id[i] != 0) first_nonzero = i;
  size_t next = 1;
  for (size_t i = first_nonzero; i < n; i++)
    if (word_id[i] != 0) {
      if (word_id[i] != next) return -1;
      flagged[i] = 1;
      next++;
    }
  if (n_words > 0) {
    if (next != n_words) return -1;
    size_t candidates = 0, at = 0;
    for (size_t i = 1; i < first_nonzero; i++)
      if (n_children[i] == 0) { candidates++; at = i; }
    if (candidates == 1) flagged[at] = 1;
    else
      for (size_t i = 1; i < first_nonzero; i++) flagged[i] = 2;
  }
  return (int)n;
}

/* Which descriptor bytes FORB::fromString (FORB.cpp:120-135) stores for each node line of the file: stored[n_nodes][32], node i = line
   i (the loader makes a node of every line it reads, :1378-1386); row 0 (the root) is 0.  The stand-in cv::Mat::create zero-fills and
   leaves an existing 1 x 32 row as it is, so the reference's own fromString is run here twice on the string the loader builds of the
   line (:1397-1404, restated: tokens 3 .. 34, each followed by a blank), over a row filled with 0x00 and one filled with 0xff; a byte is
   stored where the two results agree.  Returns the number of node lines. */
int refv_desc_stored(const char *path, int n_nodes, uint8_t *stored) {
  std::ifstream f(path);
  std::string line;
  std::getline(f, line);
  int i = 0;
  if (n_nodes > 0) memset(stored, 0, 32);
  while (!f.eof()) {
    std::getline(f, line);
    i++;
    if (i >= n_nodes) continue;
    std::stringstream in, built;
    in << line;
    std::string tok;
    in >> tok;
    tok.clear();
    in >> tok;
    for (int d = 0; d < 32; d++) {
      std::string e;
      in >> e;
      built << e << " ";
    }
    cv::Mat lo(1, 32, CV_8U), hi(1, 32, CV_8U);
    memset(lo.ptr<unsigned char>(), 0x00, 32);
    memset(hi.ptr<unsigned char>(), 0xff, 32);
    DBoW2::FORB::fromString(lo, built.str());
    DBoW2::FORB::fromString(hi, built.str());
    for (int d = 0; d < 32; d++) stored[32 * (size_t)i + d] = lo.ptr<unsigned char>()[d] == hi.ptr<unsigned char>()[d];
  }
  return i;
}

/* transform(features, v, fv, levelsup) (:1126-1194) of desc [n][32], flattened in the order the two std::maps iterate in:
   bow_id / bow_val [n_bow]; fv_node_id [n_fv], fv_start [n_fv + 1], fv_idx [fv_start[n_fv]].  Every array holds n (n + 1) entries. */
int refv_transform(const void *h, const uint8_t *desc, int n, int levelsup, uint32_t *bow_id, double *bow_val, int32_t *n_bow,
                   uint32_t *fv_node_id, int32_t *fv_start, int32_t *fv_idx, int32_t *n_fv) {
  const Voc *v = (const Voc *)h;
  std::vector<cv::Mat> features;
  to_mats(desc, n, features);
  DBoW2::BowVector bv;
  DBoW2::FeatureVector fv;
  v->transform(features, bv, fv, levelsup);
  if ((long)bv.size() > (long)n || (long)fv.size() > (long)n) return -1;
  int b = 0;
  for (DBoW2::BowVector::const_iterator it = bv.begin(); it != bv.end(); ++it, ++b) {
    bow_id[b] = it->first;
    bow_val[b] = it->second;
  }
  *n_bow = b;
  int g = 0, at = 0;
  fv_start[0] = 0;
  for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it, ++g) {
    fv_node_id[g] = it->first;
    for (size_t j = 0; j < it->second.size(); j++) {
      if (at >= n) return -1;
      fv_idx[at++] = (int32_t)it->second[j];
    }
    fv_start[g + 1] = at;
  }
  *n_fv = g;
  return 0;
}

/* transform(feature, word_id, weight, &nid, levelsup) (:1217-1259) per feature; nid[i] is preset to 0xffffffff, so that it shows where
   the reference never writes it */
int refv_transform_each(const void *h, const uint8_t *desc, int n, int levelsup, uint32_t *word, double *weight, uint32_t *nid) {
  const Voc *v = (const Voc *)h;
  if (v->empty()) return -1; /* the batch form returns before any descent (:1134); the single one would index an empty children */
  std::vector<cv::Mat> features;
  to_mats(desc, n, features);
  for (int i = 0; i < n; i++) {
    DBoW2::WordId id = 0;
    DBoW2::WordValue w = 0;
    DBoW2::NodeId node = 0xffffffffu;
    v->one(features[i], id, w, &node, levelsup);
    word[i] = id;
    weight[i] = w;
    nid[i] = node;
  }
  return 0;
}

}  // extern "C"
