"""CPU: the vocabulary transform and the text loader against the reference's own DBoW2, compiled.

oracle/_ref/libref_voc.so is the reference's unmodified Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h (instantiated for FORB), FORB.cpp,
BowVector.cpp, FeatureVector.cpp, ScoringObject.cpp and DUtils, built against the stand-in headers of oracle/ref_cam_shim with
oracle/ref_voc_driver.cc.  tests/voc_model.py is a restatement of that text by the same hands as csrc/orb_ref_voc.h and the kernels; a
misreading of DBoW2 that all three share - the order a std::map iterates in, a `<` against a `<=`, which weighting adds, the order of the
L1 sum, the level *nid is taken at, what the loader makes of a line - shows here.  Every vocabulary is a text file written by
tests/voc_scene.py::write_text into tmp_path, loaded by the reference's own loadFromTextFile; every comparison is exact, doubles by bit
pattern.

The library is built here when the reference tree is present; the tests skip only where there is neither a library nor a tree.  Run
with -s to read the counts and what the loader made of trailing newlines."""
import numpy as np
import pytest

import ref_voc_cases as RC
import voc_model as VM
import voc_scene as VS

# the reference is not called where it would read an unset NodeId (TemplatedVocabulary.h:1160 after :1251 never fired): exactly the
# model's ShallowLeaf cases, which the product refuses.  On the scenes of VS.NAMES these are:
LEFT_OUT = {("irregular", 0), ("irregular", 1), ("wide", 0)}


@pytest.fixture(scope="module")
def ref(oracle):
    try:
        oracle.ref_voc_lib()
    except RuntimeError:
        pytest.skip("no oracle/_ref/libref_voc.so and no reference tree to build it from")
    return oracle


@pytest.fixture(scope="module")
def files(ref, tmp_path_factory):
    f = RC.Files(ref, tmp_path_factory.mktemp("voc"))
    yield f
    f.close()


def _three_way(pkg, ref, files, name, weighting, scoring, levelsup, n_values):
    """Model, host form and compiled text on one (scene, weighting, scoring, levelsup): the number of compared cases, or None where the
    model refuses - then the product must refuse too and the reference is not called."""
    S = VS.scene(name)
    model = VS.model(name, weighting, scoring)
    voc = VS.vocabulary(pkg, name, weighting, scoring, device=-1)
    compared = 0
    for n in n_values:
        what = "%s weighting %d scoring %d levelsup %d n %d" % (name, weighting, scoring, levelsup, n)
        q = S["queries"][:n]
        try:
            want = model.transform(q, levelsup)
        except VM.ShallowLeaf:
            with pytest.raises(ValueError):
                voc.transform_host(q, levelsup)
            return None
        got = voc.transform_host(q, levelsup)
        R = files.ref(name, weighting, scoring)
        assert (R.k, R.L, R.weighting, R.scoring, R.n_nodes, R.n_words) == (S["k"], S["L"], weighting, scoring, len(S["parent"]), model.n_words)
        rt = RC.ref_transform(ref, R, q, levelsup)
        RC.same_as_ref(ref, got, rt, what + " (host form against the compiled text)")
        RC.same_as_ref(ref, want, rt, what + " (model against the compiled text)")
        VM.same(got, want, what + " (host form against the model)")
        compared += 1
    return compared


@pytest.mark.parametrize("name", VS.NAMES)
def test_model_and_host_form_equal_the_compiled_transform(pkg, ref, files, name):
    S = VS.scene(name)
    compared, left_out = 0, set()
    for weighting in VS.WEIGHTINGS:
        for scoring in VS.SCORINGS_ACCEPTED:
            for levelsup in VS.levelsups(S["L"]):
                c = _three_way(pkg, ref, files, name, weighting, scoring, levelsup, VS.N_VALUES)
                if c is None:
                    left_out.add((name, levelsup))
                else:
                    assert c == len(VS.N_VALUES)
                    compared += c
    print("\n%s: %d (weighting, scoring, levelsup, n) cases compared with the compiled transform; left out (the reference would read an "
          "unset NodeId, the product refuses): %s" % (name, compared, sorted(left_out) or "none"))
    assert left_out == {c for c in LEFT_OUT if c[0] == name}
    per_levelsup = len(VS.WEIGHTINGS) * len(VS.SCORINGS_ACCEPTED) * len(VS.N_VALUES)
    assert compared == per_levelsup * (len(VS.levelsups(S["L"])) - len(left_out))


def test_left_out_set_is_exactly_what_the_model_and_the_product_refuse(pkg, ref):
    """Independent of the comparison above: every (scene, weighting, scoring, levelsup) asked of the model and of the product with one
    query; both refuse the same set, and it is the three scene / levelsup pairs."""
    model_refuses, product_refuses = set(), set()
    total = 0
    for name in VS.NAMES:
        S = VS.scene(name)
        for weighting in VS.WEIGHTINGS:
            for scoring in VS.SCORINGS_ACCEPTED:
                voc = VS.vocabulary(pkg, name, weighting, scoring, device=-1)
                for levelsup in VS.levelsups(S["L"]):
                    total += 1
                    try:
                        VS.model(name, weighting, scoring).transform(S["queries"][:1], levelsup)
                    except VM.ShallowLeaf:
                        model_refuses.add((name, weighting, scoring, levelsup))
                    try:
                        voc.transform_host(S["queries"][:1], levelsup)
                    except ValueError:
                        product_refuses.add((name, weighting, scoring, levelsup))
    assert model_refuses == product_refuses
    assert {(c[0], c[3]) for c in model_refuses} == LEFT_OUT
    assert len(model_refuses) == len(LEFT_OUT) * len(VS.WEIGHTINGS) * len(VS.SCORINGS_ACCEPTED)
    print("\nleft out of %d (scene, weighting, scoring, levelsup) combinations: exactly %s, under every weighting and scoring; nothing else "
          "is skipped" % (total, sorted(LEFT_OUT)))


def test_l2_norm_stays_refused(pkg, ref, files):
    """The compiled text loads and runs scoring 1; orbv_create refuses it (csrc/orb_ref_voc.h)."""
    R = files.ref("flat", 0, 1)
    assert R.scoring == 1 and R.n_words == 10
    with pytest.raises(ValueError) as e:
        VS.vocabulary(pkg, "flat", 0, 1, device=-1)
    assert "L2_NORM" in str(e.value)
    with pytest.raises(ValueError):
        pkg.ORBVocabulary.load_text(files.path("flat", 0, 1), device=-1)


def test_orbvoc_shaped_scene(pkg, ref, files):
    """k = 10, L = 6 and levelsup = 4 under TF_IDF and L1_NORM: the only configuration the reference itself runs (Frame.cc:833,
    KeyFrame.cc:107).  The FeatureVector's nodes are those of level L - 4 = 2, which the other trees reach only on `deep`."""
    name, weighting, scoring, levelsup = RC.ORBVOC_CASE
    S = VS.scene(name)
    model = VS.model(name, weighting, scoring)
    level = np.zeros(len(S["parent"]), int)
    for i in range(1, len(level)):
        level[i] = level[S["parent"][i]] + 1
    assert (S["k"], S["L"]) == (10, 6) and 2000 <= len(S["parent"]) <= 5000
    assert (level == 1).sum() == 10 and model.min_leaf_level == 2 and level.max() == 6
    assert len(set(level[S["is_leaf"] == 1])) == 5                  # leaves at every level from 2 to 6
    assert _three_way(pkg, ref, files, name, weighting, scoring, levelsup, VS.N_VALUES) == len(VS.N_VALUES)
    t = model.transform(S["queries"], levelsup)
    assert len(t["fv_node_id"]) >= 30 and set(level[t["fv_node_id"]]) == {2}
    # and the levelsup the shape does not allow is refused, not compared
    assert _three_way(pkg, ref, files, name, weighting, scoring, 0, (5,)) is None


def test_the_run_holds_ties_stop_words_and_the_accumulation(ref):
    """What the comparison above relies on is really in the compared queries (the model's stats): descents decided by position among equal
    distances, stopped features, and a word hit six times or more with weight 0.1, whose sequential sum is not count x weight."""
    ties = stops = tenths = 0
    for name in VS.NAMES + (RC.ORBVOC_CASE[0],):
        S = VS.scene(name)
        levelsup = RC.ORBVOC_CASE[3] if name == RC.ORBVOC_CASE[0] else S["L"]
        st = VS.model(name, 0, 0).transform(S["queries"], levelsup)["stats"]
        ties += st["tie"]
        stops += st["stop"]
        for ws in st["counts"].values():
            if len(ws) >= 6 and set(ws) == {0.1}:
                acc = 0.0
                for w in ws:
                    acc += w
                tenths += acc != len(ws) * 0.1
    print("\nin the compared queries: %d descents decided by position, %d stopped features, %d words of weight 0.1 whose sequential sum "
          "differs from count x weight" % (ties, stops, tenths))
    assert ties > 0 and stops > 0 and tenths > 0


# ---- the loader ----------------------------------------------------------------------------------------------------------------------
def _weights_scene():
    """`irregular` with weights whose text is long or in exponent form."""
    S = dict(VS.scene("irregular"))
    w = S["weight"].copy()
    special = [0.30000000000000004, 1.2345678901234567e-05, 1e-05, 3.0517578125e-05, 1e+16, 5.551115123125783e-17, 2.2250738585072014e-308,
               1.7976931348623157e+308, 0.1]
    at = np.flatnonzero(S["is_leaf"])[:len(special)]
    assert len(at) == len(special)
    w[at] = special
    S["weight"] = w
    S["name"] = "irregular_weights"
    return S


def _significant_digits(x):
    return len(repr(float(x)).split("e")[0].replace(".", "").replace("-", "").strip("0"))


def _same_tables(pkg, R, path, S_name):
    k, L, scoring, weighting, parent, leaf, desc, weight = pkg.ORBVocabulary.parse_text(path)
    N = R.nodes()
    assert (R.k, R.L, R.scoring, R.weighting, R.n_nodes) == (k, L, scoring, weighting, len(parent)), S_name
    assert np.array_equal(N["parent"], parent), S_name
    assert np.array_equal(N["flagged"], leaf), S_name
    assert np.array_equal(N["n_children"], np.bincount(parent[1:], minlength=len(parent))), S_name
    assert np.array_equal(N["word_id"], np.where(leaf == 1, np.cumsum(leaf) - 1, 0)), S_name   # :1408-1415, Node() : word_id(0)
    assert R.n_words == int(leaf.sum())
    assert N["stored"][1:].all(), "%s: fromString did not store every descriptor byte of a node line" % S_name
    assert np.array_equal(N["descriptor"][1:], desc[1:]), S_name                                # the root is not in the file
    assert np.array_equal(N["weight"].view(np.uint64), weight.view(np.uint64)), "%s: float() and operator>>(double&) disagree" % S_name
    return N


@pytest.mark.parametrize("name", VS.NAMES + (RC.ORBVOC_CASE[0], "irregular_weights"))
def test_parse_text_equals_the_compiled_loader(pkg, ref, files, name):
    """No trailing newline: the tables of ORBVocabulary.parse_text against m_nodes as loadFromTextFile left them."""
    S = _weights_scene() if name == "irregular_weights" else VS.scene(name)
    path = files.path(name, 2, 5, newlines=0, scene=S)
    assert not open(path).read().endswith("\n")
    R = files.ref(name, 2, 5, newlines=0, scene=S)
    N = _same_tables(pkg, R, path, name)
    assert np.array_equal(N["weight"].view(np.uint64), S["weight"].view(np.uint64)) and np.array_equal(N["parent"], S["parent"])
    assert any(_significant_digits(w) == 17 for w in S["weight"]), "no weight that repr writes with 17 digits"
    if name == "irregular_weights":
        texts = [repr(float(w)) for w in S["weight"]]
        assert sum("e-" in t for t in texts) >= 4 and sum("e+" in t for t in texts) >= 2


@pytest.mark.parametrize("name", VS.NAMES)
def test_trailing_newlines_as_the_compiled_loader_takes_them(pkg, ref, files, name):
    """One trailing newline and two.  The loader makes a node of every line it reads (:1378-1386), and `while(!f.eof())` reads one
    empty line per trailing newline.  On an empty line `>> pid` (:1390) and `>> nIsLeaf` (:1395) fail at the stream's sentry and store
    nothing, so the parent and the leaf flag of that node are indeterminate reads: what is asserted is the part that is not the
    toolchain's choice (one node per empty line, weight 0, no children, no descriptor byte stored); the parent and the flag seen are
    printed.  Then the drop-in path: m_nodes as the loader left them through from_nodes, against the compiled transform."""
    S = VS.scene(name)
    n0, words0 = len(S["parent"]), int(S["is_leaf"].sum())
    for newlines in (1, 2):
        R = files.ref(name, 0, 0, newlines=newlines)
        N, args = RC.loaded_tables(R)
        assert R.n_nodes == n0 + newlines, "one extra node per empty line"
        extra = np.arange(n0, R.n_nodes)
        assert np.all(N["weight"][extra] == 0) and not np.any(N["n_children"][extra]) and not N["stored"][extra].any()
        assert np.all(N["parent"][extra] < n0)
        flagged = N["flagged"][extra]
        assert R.n_words == words0 + int(flagged.sum())
        print("\n%s, %d trailing newline(s): %d extra node(s), parent %s (the last node line's parent is %d), flagged as a leaf %s, word id "
              "%s, weight %s, size() %d -> %d" % (name, newlines, newlines, N["parent"][extra].tolist(), S["parent"][-1], flagged.tolist(),
                                                 N["word_id"][extra].tolist(), N["weight"][extra].tolist(), words0, R.n_words))
        # the tables before the extra nodes are the file's, and load_text (which skips blank lines) has one word fewer per flagged extra
        assert np.array_equal(N["parent"][:n0], S["parent"]) and np.array_equal(N["flagged"][:n0], S["is_leaf"])
        skipping = pkg.ORBVocabulary.load_text(files.path(name, 0, 0, newlines=newlines), device=-1)
        assert skipping.n_nodes == n0 and skipping.n_words == R.n_words - int(flagged.sum())
        # the drop-in path, with queries that are exact copies of the extra nodes' descriptors as well
        queries = np.concatenate([S["queries"], np.repeat(N["descriptor"][extra], 3, axis=0)])
        reached = 0
        for weighting, scoring in ((0, 0), (1, 5)):
            Rw = files.ref(name, weighting, scoring, newlines=newlines)
            a = list(args)
            a[2], a[3] = weighting, scoring
            voc = pkg.ORBVocabulary.from_nodes(*a, device=-1)
            model = VM.VocModel(*a)
            assert voc.n_nodes == R.n_nodes and voc.n_words == R.n_words == model.n_words
            for levelsup in VS.levelsups(S["L"]):
                what = "%s, %d trailing newline(s), weighting %d scoring %d levelsup %d" % (name, newlines, weighting, scoring, levelsup)
                try:
                    want = model.transform(queries, levelsup)
                except VM.ShallowLeaf:
                    assert (name, levelsup) in LEFT_OUT, what
                    with pytest.raises(ValueError):
                        voc.transform_host(queries, levelsup)
                    continue
                got = voc.transform_host(queries, levelsup)
                rt = RC.ref_transform(ref, Rw, queries, levelsup)
                RC.same_as_ref(ref, got, rt, what)
                VM.same(got, want, what + " (model)")
                ends_there = rt["word"] >= words0                       # a word id that only an extra node carries
                assert np.all(rt["weight"][ends_there] <= 0)            # stopped in both: same_as_ref held got to rt
                reached += int(ends_there.sum())
        print("    features that ended in an extra node (all stopped): %d" % reached)
        if name == "flat" and flagged.all():
            assert reached > 0                                          # under the root the copies of its descriptor find it
