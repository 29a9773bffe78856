// ComputeBoW_hip.cc -- drop-in bodies of void Frame::ComputeBoW() (src/Frame.cc:828-835) and void KeyFrame::ComputeBoW()
// (src/KeyFrame.cc:100-110): both are `mpORBvocabulary->transform(vCurrentDesc, mBowVec, mFeatVec, 4)`
// (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1126-1194), here orbv_transform of include/orbhip.h.
//
// Delete (or #if 0) the two members in src/Frame.cc and src/KeyFrame.cc and add this file to the library's sources.  The vocabulary is
// flattened ONCE per ORBVocabulary object, from m_nodes AS THE LOADER LEFT THEM (a trailing empty line of ORBvoc.txt gives some
// node one more child of weight 0, TemplatedVocabulary.h:1378-1392; it is carried over, not repaired), and the handle is kept in a mutex-guarded map: Tracking
// and LocalMapping call ComputeBoW on the same vocabulary from their own threads, which orbv_transform allows.  m_nodes is protected;
// it is reached through a derived class's pointer to member, without touching DBoW2's sources.  The two containers are filled by hinted
// insert from the sorted output, so they hold exactly the keys, values and per-node index order the reference's loop builds.
// There is no CPU fallback: a failed orbv_create or orbv_transform throws.
#include <cstdlib>
#include <cstring>
#include <list>   // Map.h names std::list without including it
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "ORBVocabulary.h"
#include "orbhip.h"

namespace ORB_SLAM3 {

namespace {

struct VocAccess : public ORBVocabulary {
  // m_nodes, m_words and the four parameters of `voc`, flattened in id order as orbv_nodes_t wants them
  static orbv_t *flatten(const ORBVocabulary &voc, int device) {
    const std::vector<Node> &nodes = voc.*(&VocAccess::m_nodes);
    const std::vector<Node *> &words = voc.*(&VocAccess::m_words);
    const size_t n = nodes.size();
    std::vector<uint32_t> parent(n);
    std::vector<uint8_t> leaf(n), desc(n * 32, 0);
    std::vector<double> weight(n);
    size_t flagged = 0;
    for (size_t i = 0; i < n; i++) {
      const Node &nd = nodes[i];
      parent[i] = (uint32_t)nd.parent;
      leaf[i] = nd.word_id < words.size() && words[nd.word_id] == &nd;   // the loader gave it a word (:1408-1415)
      flagged += leaf[i];
      if (!nd.descriptor.empty()) std::memcpy(&desc[i * 32], nd.descriptor.ptr<uint8_t>(), 32);   // the root has none
      weight[i] = nd.weight;
    }
    // m_words points into m_nodes, and the loader reserves (k^(L+1) - 1)/(k - 1) nodes once (:1370-1372): a file with more node lines
    // than that (a COMPLETE tree plus the node of a trailing empty line; ORBvoc.txt is pruned and stays below) makes m_nodes grow and
    // leaves every pointer of m_words dangling, in the reference too.  Then no node would pass for a word: an error, not an empty BoW.
    if (flagged != words.size()) throw std::runtime_error("ComputeBoW: m_words does not point into m_nodes (the vocabulary grew after its words were filed)");
    orbv_nodes_t t;
    t.k = voc.*(&VocAccess::m_k);
    t.L = voc.*(&VocAccess::m_L);
    t.weighting = (int32_t)(voc.*(&VocAccess::m_weighting));
    t.scoring = (int32_t)(voc.*(&VocAccess::m_scoring));
    t.n_nodes = (int32_t)n;
    t.parent = parent.data(); t.is_leaf = leaf.data(); t.descriptor = desc.data(); t.weight = weight.data();
    return orbv_create(&t, device);
  }
};

orbv_t *vocabulary_handle(const ORBVocabulary *voc) {
  static std::mutex mu;
  static std::map<const ORBVocabulary *, orbv_t *> handles;   // one per vocabulary object, for the life of the process
  std::lock_guard<std::mutex> lock(mu);
  std::map<const ORBVocabulary *, orbv_t *>::iterator it = handles.find(voc);
  if (it != handles.end()) return it->second;
  const char *e = std::getenv("ORBHIP_DEVICE");
  orbv_t *v = VocAccess::flatten(*voc, e ? std::atoi(e) : 0);
  if (!v) throw std::runtime_error(std::string("ComputeBoW: orbv_create failed (there is no CPU fallback): ") + orbv_last_error(NULL));
  handles[voc] = v;
  return v;
}

// mpORBvocabulary->transform(Converter::toDescriptorVector(descriptors), bow, fv, 4)
void compute_bow(const ORBVocabulary *voc, const cv::Mat &descriptors, DBoW2::BowVector &bow, DBoW2::FeatureVector &fv) {
  bow.clear();   // :1131-1132
  fv.clear();
  const int n = descriptors.rows;
  if (n <= 0) return;
  orbv_t *v = vocabulary_handle(voc);
  std::vector<uint8_t> desc((size_t)n * 32);
  for (int i = 0; i < n; i++) std::memcpy(&desc[(size_t)i * 32], descriptors.ptr<uint8_t>(i), 32);
  std::vector<uint32_t> bow_id(n), node_id(n);
  std::vector<double> bow_val(n);
  std::vector<int32_t> start(n + 1), idx(n);
  int32_t n_bow = 0, n_fv = 0;
  if (orbv_transform(v, desc.data(), n, 4, NULL, NULL, bow_id.data(), bow_val.data(), &n_bow, node_id.data(), start.data(), idx.data(), &n_fv) < 0)
    throw std::runtime_error(std::string("ComputeBoW: ") + orbv_last_error(v));
  for (int t = 0; t < n_bow; t++) bow.insert(bow.end(), DBoW2::BowVector::value_type(bow_id[t], bow_val[t]));   // ascending: the hint is exact
  for (int g = 0; g < n_fv; g++) {
    DBoW2::FeatureVector::iterator it = fv.insert(fv.end(), DBoW2::FeatureVector::value_type(node_id[g], std::vector<unsigned int>()));
    it->second.assign(idx.begin() + start[g], idx.begin() + start[g + 1]);
  }
}

}  // namespace

void Frame::ComputeBoW() {
  if (mBowVec.empty()) compute_bow(mpORBvocabulary, mDescriptors, mBowVec, mFeatVec);
}

void KeyFrame::ComputeBoW() {
  if (mBowVec.empty() || mFeatVec.empty()) compute_bow(mpORBvocabulary, mDescriptors, mBowVec, mFeatVec);
}

}  // namespace ORB_SLAM3
