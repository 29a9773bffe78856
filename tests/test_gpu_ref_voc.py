"""GPU: the device vocabulary transform (orbv_transform, orbv_transform_batch_device: k_voc_descend / k_voc_descend_lane + k_voc_collect)
against the reference's own DBoW2, compiled (oracle/_ref/libref_voc.so: TemplatedVocabulary.h, FORB.cpp, BowVector.cpp,
FeatureVector.cpp and ScoringObject.cpp unmodified against the stand-in headers of oracle/ref_cam_shim, with oracle/ref_voc_driver.cc).

tests/test_gpu_voc.py compares the kernels with tests/voc_model.py, a restatement by the same hands; a misreading of DBoW2's own text
that the model, csrc/orb_ref_voc.h and the kernels share shows here.  Every vocabulary is a text file of a tests/voc_scene.py scene written
into tmp_path and loaded by the reference's own loadFromTextFile; every comparison is exact, doubles by bit pattern.  The sizes are the
smallest that cross the 16-lane DPP row (15 / 16 / 17 children: `wide`, 20 plus one), the 64-lane wavefront (n = 63, 64, 65) and a second
LDS sort tile (n = 257); the 15360-descriptor case stays in tests/test_gpu_voc.py, against the model.

The library is built by __graft_entry__.build() where the reference tree exists and travels with the tree; these tests only load it and
never look for the reference.  They skip where the library is absent.  One process, no subprocesses."""
import numpy as np
import pytest

import ref_matcher_cases as MC
import ref_voc_cases as RC
import voc_model as VM
import voc_scene as VS
from test_gpu_voc import _batch, _frame_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(oracle):
    try:
        oracle.ref_voc_lib(build_if_possible=False)
    except (RuntimeError, OSError):
        pytest.skip("no oracle/_ref/libref_voc.so: __graft_entry__.build() makes it where the reference tree exists")
    return oracle


@pytest.fixture(scope="module")
def files(ref, tmp_path_factory):
    f = RC.Files(ref, tmp_path_factory.mktemp("voc"))
    yield f
    f.close()


def _refused(model, levelsup):
    """The reference would read an unset NodeId (the model's ShallowLeaf): the product refuses, the reference is not called."""
    try:
        model.transform(np.zeros((0, 32), np.uint8), levelsup)
    except VM.ShallowLeaf:
        return True
    return False


def _single_frame(ref, voc, R, model, queries, L, name, tag):
    compared = 0
    for levelsup in VS.levelsups(L):
        if _refused(model, levelsup):
            with pytest.raises(ValueError):
                voc.transform(queries[:5], levelsup)
            continue
        for n in VS.N_VALUES:
            what = "%s %s levelsup %d n %d" % (name, tag, levelsup, n)
            RC.same_as_ref(ref, voc.transform(queries[:n], levelsup), RC.ref_transform(ref, R, queries[:n], levelsup), what)
            compared += 1
    return compared


@pytest.mark.parametrize("name", VS.NAMES)
def test_single_frame_entry_equals_the_compiled_transform(pkg, ref, files, name):
    S = VS.scene(name)
    compared = 0
    for weighting in VS.WEIGHTINGS:
        for scoring in VS.SCORINGS_ACCEPTED:
            voc = VS.vocabulary(pkg, name, weighting, scoring, device=0)
            compared += _single_frame(ref, voc, files.ref(name, weighting, scoring), VS.model(name, weighting, scoring), S["queries"], S["L"],
                                      name, "weighting %d scoring %d" % (weighting, scoring))
    left_out = sum(_refused(VS.model(name, 0, 0), ls) for ls in VS.levelsups(S["L"]))
    assert left_out == {"irregular": 2, "wide": 1}.get(name, 0)
    assert compared == len(VS.WEIGHTINGS) * len(VS.SCORINGS_ACCEPTED) * len(VS.N_VALUES) * (len(VS.levelsups(S["L"])) - left_out)
    print("\n%s: %d device transforms compared with the compiled text" % (name, compared))


def test_single_frame_entry_on_the_orbvoc_shaped_scene(pkg, ref, files):
    name, weighting, scoring, levelsup = RC.ORBVOC_CASE
    S = VS.scene(name)
    voc, R = VS.vocabulary(pkg, name, weighting, scoring, device=0), files.ref(name, weighting, scoring)
    for n in VS.N_VALUES:
        RC.same_as_ref(ref, voc.transform(S["queries"][:n], levelsup), RC.ref_transform(ref, R, S["queries"][:n], levelsup), "n %d" % n)


@pytest.mark.parametrize("name", VS.NAMES)
def test_single_frame_entry_on_the_loaders_own_tables(pkg, ref, files, name):
    """A file that ends in a newline, and one that ends in two: m_nodes as the compiled loader left them (the extra nodes included, is_leaf
    = what the loader flagged) through from_nodes - the drop-in path - with copies of the extra nodes' descriptors among the queries."""
    S = VS.scene(name)
    for newlines in (1, 2):
        R = files.ref(name, 0, 0, newlines=newlines)
        N, args = RC.loaded_tables(R)
        assert R.n_nodes == len(S["parent"]) + newlines
        voc = pkg.ORBVocabulary.from_nodes(*args, device=0)
        assert voc.n_words == R.n_words
        queries = np.concatenate([np.repeat(N["descriptor"][len(S["parent"]):], 3, axis=0), S["queries"]])
        assert _single_frame(ref, voc, R, VM.VocModel(*args), queries, S["L"], name, "%d trailing newline(s)" % newlines) >= 2 * len(VS.N_VALUES)


@pytest.mark.parametrize("name,weighting,scoring,levelsup", [("regular", 0, 0, 1), ("wide", 1, 5, 1), ("deep", 2, 0, 4), RC.ORBVOC_CASE])
def test_batch_entry_equals_the_compiled_transform(pkg, ref, files, name, weighting, scoring, levelsup):
    """Ragged live counts, among them 0, 1, the capacity, one above it (taken as the capacity) and a negative one (taken as 0); both
    descent kernels and the default; every frame against the compiled transform of its live descriptors."""
    import torch
    dev = torch.device("cuda", 0)
    S = VS.scene(name)
    voc, R = VS.vocabulary(pkg, name, weighting, scoring, device=0), files.ref(name, weighting, scoring)
    cap = 300
    counts = [0, 1, 65, cap, 257, cap + 100, -5, 64]
    live = [min(max(c, 0), cap) for c in counts]
    B = len(counts)
    rng = np.random.default_rng(3)
    desc = S["queries"][rng.integers(0, 1000, (B, cap))]
    d_desc = torch.from_numpy(np.ascontiguousarray(desc)).to(dev)
    d_n = torch.tensor(counts, dtype=torch.int32, device=dev)
    want = [RC.ref_transform(ref, R, desc[p, :live[p]], levelsup) for p in range(B)]
    for form in (None, 0, 1):
        out = _batch(pkg, voc, torch, d_desc, B, cap, d_n, 1, levelsup, descend_form=form)
        for p in range(B):
            RC.same_as_ref(ref, _frame_of(out, p, live[p]), want[p], "form %s frame %d" % (form, p))


@pytest.mark.parametrize("name,levelsup", [("regular", 2), (RC.ORBVOC_CASE[0], RC.ORBVOC_CASE[3])])
def test_chain_into_search_by_bow(pkg, ref, files, name, levelsup):
    """Two synthetic frames: the device transform's FeatureVector, unchanged, into the device SearchByBoW; the compiled DBoW2's
    FeatureVector of the same descriptors into the compiled ORBmatcher.cc's SearchByBoW.  No model of ours stands between the
    reference's two texts."""
    try:
        ref.ref_match_lib(build_if_possible=False)
    except (RuntimeError, OSError):
        pytest.skip("no oracle/_ref/libref_matcher.so")
    S = MC.bow("mono")
    ones = np.ones(MC.NLEVELS, np.float32)
    voc, R = VS.vocabulary(pkg, name, 0, 0, device=0), files.ref(name, 0, 0)

    def keys(k):
        out = np.zeros(len(k), pkg.KP_DTYPE)
        for f in ("x", "y", "octave", "angle"):
            out[f] = k[f]
        return out

    def view(k, d, **kw):
        """KeyFrameView whose three FeatureVector arrays ARE the device transform's outputs."""
        t = voc.transform(d, levelsup)
        V = pkg.KeyFrameView(keys(k), d, {}, MC.SF, ones, **kw)
        V.node_id, V.node_start, V.node_idx = t["fv_node_id"], t["fv_start"], t["fv_idx"]
        return V
    fv_of = pkg.ORBVocabulary.feat_vec                              # the flat layout as {node: [indices]}; no arithmetic
    KR = ref.OracleKeyFrame(S["kf_keys"], S["kf_desc"], fv_of(R.transform(S["kf_desc"], levelsup)), MC.SF, ones, has_mp=S["has_mp"])
    FR = ref.OracleKeyFrame(S["f_keys"], S["f_desc"], fv_of(R.transform(S["f_desc"], levelsup)), MC.SF, ones)
    n_r, m_r = ref.ref_search_by_bow(KR, FR, S["nnratio"], True)
    m = pkg.ORBmatcher(S["nnratio"], True)
    try:
        n_d, m_d = m.SearchByBoW(view(S["kf_keys"], S["kf_desc"], has_mappoint=(S["has_mp"] == 1).astype(np.uint8)), view(S["f_keys"], S["f_desc"]))
    finally:
        m.close()
    assert n_r >= 30 and n_d == n_r and np.array_equal(m_d, m_r)
