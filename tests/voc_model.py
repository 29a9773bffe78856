"""A literal Python model of DBoW2's vocabulary transform as Frame::ComputeBoW / KeyFrame::ComputeBoW call it
(TemplatedVocabulary.h:1126-1194 over :1217-1259, BowVector.cpp:34-84, FeatureVector.cpp:31-45): a dict plus its sorted keys for each
std::map, Python floats (IEEE doubles) for the values, Python ints for the descriptors.  It shares no code with csrc/orb_ref_voc.h.

What it does not pin by itself: that std::map iterates in ascending key order, and that `+=`, fabs and `/=` on doubles are the IEEE
operations.  Both are pinned by the reference's own text, compiled unmodified into oracle/_ref/libref_voc.so (oracle/ref_voc_driver.cc):
tests/test_ref_voc.py holds this model and orbv_transform_host against it on every scene, tests/test_gpu_ref_voc.py the kernels."""
import numpy as np

TF_IDF, TF, IDF, BINARY = range(4)
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)


class ShallowLeaf(ValueError):
    """The reference would file a feature under an unset *nid (:1251 never fires, :1160): refused by the library, csrc/orb_ref_voc.h."""


class VocModel:
    def __init__(self, k, L, weighting, scoring, parent, is_leaf, descriptor, weight):
        self.k, self.L, self.weighting, self.scoring = k, L, weighting, scoring
        n = len(parent)
        self.children = [[] for _ in range(n)]
        for i in range(1, n):                                   # m_nodes[pid].children.push_back(nid) (:1392)
            self.children[int(parent[i])].append(i)
        self.word_id = [0] * n                                  # Node(): word_id(0) (:316)
        self.n_words = 0
        for i in range(1, n):                                   # :1408-1415
            if is_leaf[i]:
                self.word_id[i] = self.n_words
                self.n_words += 1
        self.desc = [int.from_bytes(bytes(bytearray(np.asarray(d, np.uint8))), "little") for d in descriptor]
        self.weight = [float(w) for w in weight]
        # the level of the shallowest node without children whose weight lets a feature in (w > 0, :1157), and the lowest id among those:
        # a feature that ends there above level m_L - levelsup is filed under an unset NodeId (:1251 never fires, :1160 reads it)
        level = [0] * n
        for i in range(1, n):
            level[i] = level[int(parent[i])] + 1
        leaves = [(level[i], i) for i in range(n) if not self.children[i] and self.weight[i] > 0]
        self.min_leaf_level, self.min_leaf_node = min(leaves) if leaves else (2 ** 31 - 1, 0)
        self._paths = {}

    @staticmethod
    def distance(a, b):                                         # FORB::distance (FORB.cpp:81-101)
        return bin(a ^ b).count("1")

    def path(self, q):
        """The nodes chosen at levels 1, 2, .. for the descriptor q (an int), with whether a tie was decided by position."""
        if q in self._paths:
            return self._paths[q]
        final_id, nodes, tie, max_pos = 0, [], False, 0
        while True:
            ch = self.children[final_id]
            final_id = ch[0]
            best_d = self.distance(q, self.desc[final_id])
            pos, ties = 0, 1
            for p in range(1, len(ch)):
                d = self.distance(q, self.desc[ch[p]])
                if d < best_d:                                  # :1244
                    best_d, final_id, pos, ties = d, ch[p], p, 1
                elif d == best_d:
                    ties += 1
            tie |= ties > 1
            max_pos = max(max_pos, pos)
            nodes.append(final_id)
            if not self.children[final_id]:                     # isLeaf() (:1254, :328)
                break
        self._paths[q] = (nodes, tie, max_pos)
        return self._paths[q]

    def transform(self, desc, levelsup):
        """Returns the flat layouts the library returns, plus `stats` about what the call exercised."""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc)
        nid_level = self.L - levelsup
        if self.n_words > 0 and nid_level > 0 and self.min_leaf_level < nid_level:
            raise ShallowLeaf("node %d at level %d" % (self.min_leaf_node, self.min_leaf_level))
        word, node = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        bow, fv = {}, {}
        stats = dict(stop=0, tie=0, max_pos=0, counts={})
        adds = self.weighting in (TF, TF_IDF)                   # :1145
        must = self.scoring != DOT_PRODUCT                      # ScoringObject.h:74-89
        if self.n_words > 0:                                    # empty() (:1134)
            for i in range(n):
                q = int.from_bytes(desc[i].tobytes(), "little")
                nodes, tie, max_pos = self.path(q)
                # :1227, :1251; a feature that ends above the level is stopped here (transform refuses the others), its NodeId is never read
                nid = 0 if nid_level <= 0 or len(nodes) < nid_level else nodes[nid_level - 1]
                leaf = nodes[-1]
                wid, w = self.word_id[leaf], self.weight[leaf]
                word[i], node[i] = wid, nid
                stats["tie"] += tie
                stats["max_pos"] = max(stats["max_pos"], max_pos)
                if w > 0:                                       # :1157, :1185
                    if wid in bow:
                        if adds:
                            bow[wid] += w                       # addWeight
                    else:
                        bow[wid] = w                            # insert in both
                    stats["counts"].setdefault(wid, []).append(w)
                    fv.setdefault(nid, []).append(i)
                else:
                    stats["stop"] += 1
            ids = sorted(bow)
            stats["unnormalised"] = [bow[i] for i in ids]
            if adds and not must and bow:                       # :1164-1170
                nd = float(len(bow))
                for i in ids:
                    bow[i] /= nd
            if must:                                            # BowVector::normalize(L1)
                norm = 0.0
                for i in ids:
                    norm += abs(bow[i])
                if norm > 0.0:
                    for i in ids:
                        bow[i] /= norm
        ids = sorted(bow)
        nodes_sorted = sorted(fv)
        fv_start, fv_idx = [0], []
        for nid in nodes_sorted:
            fv_idx.extend(fv[nid])
            fv_start.append(len(fv_idx))
        return dict(word=word, node=node, bow_id=np.array(ids, np.uint32), bow_val=np.array([bow[i] for i in ids], np.float64),
                    fv_node_id=np.array(nodes_sorted, np.uint32), fv_start=np.array(fv_start, np.int32), fv_idx=np.array(fv_idx, np.int32),
                    stats=stats)


def same(a, b, what=""):
    """The flat layouts of two transforms are equal, the doubles by bit pattern."""
    for key in ("word", "node", "bow_id", "fv_node_id", "fv_start", "fv_idx"):
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), "%s: %s differs" % (what, key)
    va, vb = np.asarray(a["bow_val"], np.float64), np.asarray(b["bow_val"], np.float64)
    assert va.shape == vb.shape and np.array_equal(va.view(np.uint64), vb.view(np.uint64)), "%s: bow_val differs in its bits" % what
