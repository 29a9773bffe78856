"""What tests/test_ref_voc.py and tests/test_gpu_ref_voc.py share: the scenes of tests/voc_scene.py written as ORBvoc-format text files,
loaded by the reference's own loadFromTextFile (oracle/_ref/libref_voc.so, oracle.RefVocabulary), and the comparison of a product
transform with the compiled text's."""
import os

import numpy as np

import voc_model as VM
import voc_scene as VS

ORBVOC_CASE = ("orbvoc_shaped", 0, 0, 4)                        # TF_IDF, L1_NORM, levelsup 4: the only configuration the reference runs


class Files:
    """Vocabulary files under one directory.  A scene's node lines are written once by VS.write_text with `newlines` newlines after the
    last node line; the other (weighting, scoring) files of the scene differ in their first line alone."""

    def __init__(self, oracle, directory):
        self.oracle, self.dir = oracle, str(directory)
        self.body, self.refs = {}, {}

    def path(self, name, weighting, scoring, newlines=0, scene=None):
        key = (name, newlines)
        if key not in self.body:
            first = os.path.join(self.dir, "%s_nl%d.body" % key)
            VS.write_text(scene or VS.scene(name), 0, 0, first, newlines=newlines)
            with open(first) as f:
                f.readline()
                self.body[key] = f.read()
        S = scene or VS.scene(name)
        p = os.path.join(self.dir, "%s_w%d_s%d_nl%d.txt" % (name, weighting, scoring, newlines))
        if not os.path.exists(p):
            with open(p, "w") as f:
                f.write("%d %d %d %d\n" % (S["k"], S["L"], scoring, weighting))
                f.write(self.body[key])
        return p

    def ref(self, name, weighting, scoring, newlines=0, scene=None):
        """The compiled vocabulary after its own loadFromTextFile of that file."""
        key = (name, weighting, scoring, newlines)
        if key not in self.refs:
            self.refs[key] = self.oracle.RefVocabulary(self.path(name, weighting, scoring, newlines, scene))
        return self.refs[key]

    def close(self):
        for r in self.refs.values():
            r.close()
        self.refs = {}


def ref_transform(oracle, R, desc, levelsup):
    """Both compiled transforms of one call: the containers, and word / weight / *nid per feature."""
    t = R.transform(desc, levelsup)
    if R.n_words > 0:
        t["word"], t["weight"], t["nid"] = R.transform_each(desc, levelsup)
    else:
        n = len(np.asarray(desc).reshape(-1, 32))
        t["word"], t["weight"], t["nid"] = np.zeros(n, np.uint32), np.zeros(n, np.float64), np.zeros(n, np.uint32)
    return t


def same_as_ref(oracle, got, want, what):
    """A product transform `got` against the compiled text's `want` (ref_transform): the two containers equal, the doubles by bit
    pattern; word equal; node equal wherever the reference wrote *nid, and where it did not (the sentinel stays) the product gives 0 and
    the feature is a stopped one.  Returns how many features had the sentinel."""
    VM.same(got, dict(want, node=got["node"]), what)           # word, the two containers; node follows

    unset = want["nid"] == oracle.REF_VOC_UNSET
    assert np.array_equal(got["node"][~unset], want["nid"][~unset]), "%s: node differs where the reference wrote *nid" % what
    assert not np.any(got["node"][unset]), "%s: node is not 0 where the reference left *nid unset" % what
    assert np.all(want["weight"][unset] <= 0), "%s: the reference left *nid unset for a feature that is not stopped" % what
    return int(unset.sum())


def loaded_tables(R):
    """from_nodes arguments of the compiled loader's m_nodes: is_leaf is what the loader FLAGGED, not the child count."""
    N = R.nodes()
    return N, (R.k, R.L, R.weighting, R.scoring, N["parent"], N["flagged"], N["descriptor"], N["weight"])
