"""Seeded vocabularies and query descriptors for the vocabulary transform (orbv_*; tests/test_voc_abi.py, tests/test_gpu_voc.py).

Seven trees in NAMES, each flattened as orbv_nodes_t wants it (node 0 the root, parent[i] < i):
  regular    k = 10, L = 3, complete, ids in depth-first order, about 3 % stop words (weight 0)
  irregular  k = 3,  L = 4, nodes with one to three children, leaves at levels 2 .. 4, ids in breadth-first order
  wide       k = 20, L = 2, complete, plus a 21st child of the root appended last: not flagged as a leaf, no children, weight 0.7 - it
             answers word 0 with its own weight, and levelsup 0 is refused for it (a childless node that lets features in above level
             L - levelsup).  No trailing empty line makes this node (see wide_trailing); it is here for the refusal and for Node() : word_id(0);
             twins (equal descriptors) among the root's children at positions (3, 7), (17, 19) and (5, 18)
  wide_as_loaded  the same shape with the 21st child's weight 0.  A feature that ends there is stopped, so the childless node at
             level 1 is harmless and every levelsup is accepted.  Despite its name this is NOT what loadFromTextFile makes of a trailing
             empty line (see wide_trailing); it stays as the unflagged, childless, weightless node the library must accept
  wide_trailing   k = 20, L = 2, complete, plus the node the compiled loadFromTextFile (TemplatedVocabulary.h:1378-1420; g++ -std=c++11
             -O2, libstdc++) was seen to make of ONE trailing empty line: the extractions `>> pid` and `>> nIsLeaf` fail at the stream's
             sentry and store nothing, so both are read uninitialised - indeterminate by the language.  Observed with this compiler
             (tests/test_ref_voc.py prints it): the parent is the previous line's parent (here node 20, so that node has 21 children at
             level 2), the node is flagged as a leaf and gets a new word id (m_words grows by one), weight 0 from Node(), descriptor
             whatever cv::Mat::create(1, 32, CV_8U) returns (here a near copy of its parent, so that queries end there: all stopped)
  deep       k = 2,  L = 10, complete, depth-first
  flat       k = 10, L = 1
And one outside NAMES (scene("orbvoc_shaped")), run only as the reference runs its vocabulary (TF_IDF, L1_NORM, levelsup 4):
  orbvoc_shaped  k = 10, L = 6 as ORBvoc.txt, pruned to a few thousand nodes: level 1 complete, six to ten children at level 1, none
             to three below, no leaf above level 2 - so levelsup = 4 (the FeatureVector's nodes at level 2) is accepted
Children are bit-flipped copies of their parent, fewer bits the deeper, so that a copy of a node's descriptor mostly descends to it.
Queries: random descriptors, exact copies of node descriptors (some leaves six times over, among them stop words and a leaf of weight 0.1),
and descriptors built equidistant to two siblings."""
import numpy as np
import pytest

from voc_model import ShallowLeaf, VocModel, same

N_VALUES = (0, 1, 3, 4, 5, 63, 64, 65, 257, 1000)
WEIGHTINGS = (0, 1, 2, 3)
SCORINGS = (0, 5)
SCORINGS_OTHER_L1 = (2, 3, 4)                                   # CHI_SQUARE, KL, BHATTACHARYYA: accepted as "L1 for all of those"
SCORINGS_ACCEPTED = SCORINGS + SCORINGS_OTHER_L1                # everything but L2_NORM (1), which orbv_create refuses


def levelsups(L):
    return sorted({0, 1, 4, L, L + 1})


def _flip(rng, d, nbits):
    out = d.copy()
    for b in rng.choice(256, size=nbits, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def _grow(rng, shape_fn, L, order):
    """shape_fn(level, rng) -> number of children of a node at `level` (0 = it is a leaf).  Returns parent, level, descriptor."""
    parent, level, desc = [0], [0], [rng.integers(0, 256, 32, dtype=np.uint8)]

    def add_child(i):
        parent.append(i)
        level.append(level[i] + 1)
        desc.append(_flip(rng, desc[i], max(2, 40 >> level[i])))
        return len(parent) - 1

    def count(i):
        return shape_fn(level[i], rng) if level[i] < L else 0

    if order == "bfs":
        queue = [0]
        while queue:
            i = queue.pop(0)
            queue.extend([add_child(i) for _ in range(count(i))])
    else:
        # depth-first: a child's whole subtree gets its ids before the next child, so siblings are not contiguous in id
        def rec(i):
            for _ in range(count(i)):
                rec(add_child(i))
        rec(0)
    return np.array(parent, np.uint32), np.array(level), np.stack(desc)


def _finish(name, seed, k, L, parent, level, desc, extra_root_child=False, extra_weight=0.7, extra_parent=0, extra_flagged=0):
    rng = np.random.default_rng(seed + 1000)
    n = len(parent)
    has_child = np.zeros(n, bool)
    has_child[parent[1:]] = True
    is_leaf = (~has_child).astype(np.uint8)
    is_leaf[0] = 0
    weight = np.where(is_leaf == 1, rng.uniform(0.05, 9.0, n), 0.0)
    leaves = np.flatnonzero(is_leaf)
    stop = rng.choice(leaves, size=max(1, int(round(0.03 * len(leaves)))), replace=False)
    weight[stop] = 0.0
    live = np.setdiff1d(leaves, stop)
    weight[live[0]] = 0.1                                       # six sequential adds of 0.1 are 0.6, 6 * 0.1 is 0.6000000000000001
    if extra_root_child:
        parent = np.append(parent, np.uint32(extra_parent))
        level = np.append(level, level[extra_parent] + 1)
        extra_desc = rng.integers(0, 256, (1, 32), dtype=np.uint8)
        if extra_parent:
            extra_desc = _flip(rng, desc[extra_parent], 2)[None]
        desc = np.concatenate([desc, extra_desc])
        is_leaf = np.append(is_leaf, np.uint8(extra_flagged))
        weight = np.append(weight, extra_weight)
    # queries
    q = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(500)]
    repeated = [live[0]] + list(stop[:2]) + list(rng.choice(live, size=min(5, len(live)), replace=False))
    for node in repeated:
        q.extend([desc[node].copy()] * 6)
    if extra_root_child:
        q.extend([desc[len(parent) - 1].copy()] * 3)
    kids_of = {}
    for i in range(1, len(parent)):
        kids_of.setdefault(int(parent[i]), []).append(i)
    parents = [p for p, c in kids_of.items() if len(c) >= 2]
    while len(q) < 1000:
        if len(q) % 3 == 0 and parents:
            ch = kids_of[int(rng.choice(parents))]
            a, b = rng.choice(len(ch), size=2, replace=False)
            da, db = desc[ch[a]], desc[ch[b]]
            diff = np.flatnonzero(np.unpackbits(da ^ db, bitorder="little"))
            d = da.copy()
            for bit in diff[:len(diff) // 2]:                   # half of the differing bits from b: equidistant when their number is even
                d[bit >> 3] ^= np.uint8(1 << (bit & 7))
            q.append(d)
        else:
            q.append(desc[int(rng.integers(1, len(parent)))].copy())
    q = np.stack(q[:1000])
    q = q[rng.permutation(len(q))]
    return dict(name=name, k=k, L=L, parent=parent.astype(np.uint32), is_leaf=is_leaf, descriptor=np.ascontiguousarray(desc), weight=weight,
                queries=np.ascontiguousarray(q))


def _regular():
    rng = np.random.default_rng(11)
    return _finish("regular", 11, 10, 3, *_grow(rng, lambda lvl, r: 10, 3, "dfs"))


def _irregular():
    rng = np.random.default_rng(12)

    def shape(lvl, r):
        if lvl < 2:
            return int(r.integers(2, 4))                        # levels 0, 1: two or three children, so no leaf above level 2
        return int(r.integers(0, 3))                            # below: none, one or two
    return _finish("irregular", 12, 3, 4, *_grow(rng, shape, 4, "bfs"))


def _wide():
    rng = np.random.default_rng(13)
    parent, level, desc = _grow(rng, lambda lvl, r: 20, 2, "bfs")
    root_kids = [i for i in range(1, len(parent)) if parent[i] == 0]
    for a, b in ((3, 7), (17, 19), (5, 18)):
        desc[root_kids[b]] = desc[root_kids[a]]
    return _finish("wide", 13, 20, 2, parent, level, desc, extra_root_child=True)


def _deep():
    rng = np.random.default_rng(14)
    return _finish("deep", 14, 2, 10, *_grow(rng, lambda lvl, r: 2, 10, "dfs"))


def _flat():
    rng = np.random.default_rng(15)
    return _finish("flat", 15, 10, 1, *_grow(rng, lambda lvl, r: 10, 1, "bfs"))


def _wide_as_loaded():
    rng = np.random.default_rng(13)
    parent, level, desc = _grow(rng, lambda lvl, r: 20, 2, "bfs")
    return _finish("wide_as_loaded", 13, 20, 2, parent, level, desc, extra_root_child=True, extra_weight=0.0)


def _wide_trailing():
    rng = np.random.default_rng(13)
    parent, level, desc = _grow(rng, lambda lvl, r: 20, 2, "bfs")
    last_parent = int(parent[-1])                               # the previous line's parent: the last node of level 1
    return _finish("wide_trailing", 17, 20, 2, parent, level, desc, extra_root_child=True, extra_weight=0.0, extra_parent=last_parent,
                   extra_flagged=1)


def _orbvoc_shaped():
    rng = np.random.default_rng(18)

    def shape(lvl, r):
        if lvl == 0:
            return 10
        if lvl == 1:
            return int(r.integers(6, 11))                       # six to ten, so no leaf above level 2
        return int(r.choice((0, 2, 3, 3)))                      # below: none to three
    return _finish("orbvoc_shaped", 18, 10, 6, *_grow(rng, shape, 6, "bfs"))


_BUILDERS = dict(regular=_regular, irregular=_irregular, wide=_wide, wide_as_loaded=_wide_as_loaded, wide_trailing=_wide_trailing, deep=_deep,
                 flat=_flat)
NAMES = tuple(_BUILDERS)
_BUILDERS["orbvoc_shaped"] = _orbvoc_shaped                     # not in NAMES: see the module docstring
_cache = {}


def scene(name):
    if name not in _cache:
        _cache[name] = _BUILDERS[name]()
    return _cache[name]


def flat_big(n):
    """n descriptors for the `flat` tree (the 15360 / 15361 cases): its queries, tiled with one bit of noise."""
    rng = np.random.default_rng(16)
    q = scene("flat")["queries"]
    out = q[rng.integers(0, len(q), n)].copy()
    out[:, 31] ^= rng.integers(0, 2, n, dtype=np.uint8)
    return out


_models = {}


def model(name, weighting, scoring):
    """The model of one scene under a weighting and a scoring; the descents are shared between all of a scene's models."""
    key = (name, weighting, scoring)
    if key not in _models:
        S = scene(name)
        m = VocModel(S["k"], S["L"], weighting, scoring, S["parent"], S["is_leaf"], S["descriptor"], S["weight"])
        first = _models.get((name, "paths"))
        if first is None:
            _models[(name, "paths")] = m._paths
        else:
            m._paths = first
        _models[key] = m
    return _models[key]


def vocabulary(pkg, name, weighting, scoring, device):
    S = scene(name)
    return pkg.ORBVocabulary.from_nodes(S["k"], S["L"], weighting, scoring, S["parent"], S["is_leaf"], S["descriptor"], S["weight"], device=device)


def write_text(S, weighting, scoring, path, trailing_blank=False, newlines=None):
    """The scene as an ORBvoc-format text file (the layout loadFromTextFile reads, TemplatedVocabulary.h:1338-1424).  Every line ends in
    a newline, the last one too - which the reference's loader already takes for one empty line more (`while(!f.eof())`, :1378) - and
    trailing_blank adds a second.  newlines = 0, 1, 2 .. sets the number of newlines after the last node line exactly."""
    with open(path, "w") as f:
        f.write("%d %d %d %d\n" % (S["k"], S["L"], scoring, weighting))
        n = len(S["parent"])
        for i in range(1, n):
            end = "\n" if newlines is None or i < n - 1 else "\n" * newlines
            f.write("%d %d %s %s%s" % (S["parent"][i], S["is_leaf"][i], " ".join(str(int(b)) for b in S["descriptor"][i]),
                                      repr(float(S["weight"][i])), end))
        if trailing_blank:
            f.write("\n")


def check_against_model(voc, model, desc, levelsup, what, transform="transform_host"):
    try:
        want = model.transform(desc, levelsup)
    except ShallowLeaf:
        with pytest.raises(ValueError) as e:
            getattr(voc, transform)(desc, levelsup)
        assert "node %d " % model.min_leaf_node in str(e.value), what
        return None
    got = getattr(voc, transform)(desc, levelsup)
    same(got, want, what)
    return want
