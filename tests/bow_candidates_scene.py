"""One fixed frame / keyframe and its K = 6 candidates for the one-call SearchByBoW (orbm_search_by_bow_candidates: the loop of
Tracking::Relocalization, Tracking.cc:3796-3816; orbm_search_by_bow_keyframes_candidates: the loop of
LoopClosing::DetectCommonRegionsFromBoW, LoopClosing.cc:724-739), built without images.  A helper, not a conftest.

The same scene serves both entries.  `base` is the fixed operand: the frame F of SearchByBoW(pKF, F) - the SECOND operand, its keypoints
are taken - or pKF1 of SearchByBoW(pKF1, pKF2) - the FIRST, its keypoints are walked.  Descriptors are random 256-bit strings; a
candidate's keypoint is a copy of a base keypoint with 0-13 bits flipped in bytes 8..31 only, so that the node hash of
triangulation_kb8_scene.bow (bytes 0 and 7) keeps the pair in one node.  A copy's angle is the base keypoint's plus a rotation common to
the candidate plus up to 3 degrees of noise; every tenth copy gets a random angle instead, for the rotation histogram to remove.
has_mappoint: about 80 % where an operand is walked (`mpW`), about 70 % where a candidate is the second keyframe (`mpS`).

Candidates (kind, keypoints), ragged on purpose:
  0 "real"   400  `wide`, see below;
  1 "nonode" 200  copies, but the feature vector uses node ids the base does not have;
  2 "real"   250
  3 "nomp"   180  copies without any map point;
  4 "empty"    0
  5 "small"  120  12 copies among unrelated keypoints: fewer than 15 matches.
`wide`: the nodes with hash 0, 1, 2 hold nothing but 63, 64 and 129 fillers (descriptors far from everything) followed by ONE real
keypoint, in the base and in candidate 0 alike: the true partner is the second operand's member 63, 64 resp. 129 of a node of 64, 65
resp. 130 - the last lane-held position, the first one read from memory, and a third trip - whichever operand is the second one.
Twins exercise `taken`: two walkers of one node whose best is the same second-operand keypoint; the first (in node order) takes it, the
second must take its next best or fail.  `twinsF` [(j, base index, first, second)]: two copies of one base keypoint in candidate j (the
walkers of the frame form).  `twinsK` [(a, b)]: base keypoint b is a near copy of base keypoint a (the walkers of the keyframe form);
every real candidate holds one copy of a.  All of them have a map point.
Fisheye variant: `right` holds near copies of base keypoints as the frame's right image, F = [base; right], Nleft = len(base)."""
import numpy as np

import triangulation_kb8_scene as SC

f32 = np.float32
KINDS = (("real", 400), ("nonode", 200), ("real", 250), ("nomp", 180), ("empty", 0), ("small", 120))
WIDE = ((0, 63), (1, 64), (2, 129))      # (hash, fillers in front of the real keypoint)
N_REAL = 300                             # real keypoints of the base
N_TWINS = 6
ROTATIONS = (25.0, 100.0, 190.0, 250.0, 0.0, 310.0)


def _hash(d):
    return (int(d[0]) >> 2) * 2 + (int(d[7]) >> 7)


def _force_hash(d, h):
    d[0] = ((h >> 1) << 2) | (int(d[0]) & 3)
    d[7] = ((h & 1) << 7) | (int(d[7]) & 0x7f)
    return d


def _plain(rng, nodes):
    """A random descriptor outside the three wide nodes."""
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    while _hash(d) % nodes in (0, 1, 2):
        d[0] = rng.integers(0, 256)
    return d


def _copy(rng, d):
    c = d.copy()
    for b in rng.choice(np.arange(64, 256), int(rng.integers(0, 14)), replace=False):
        c[b // 8] ^= np.uint8(1 << (b % 8))
    return c


def _keys(angles, rng):
    n = len(angles)
    k = np.zeros(n, SC.KP_DTYPE)
    k["x"], k["y"] = rng.uniform(20, 732, n), rng.uniform(20, 460, n)
    k["size"] = 31.0
    k["octave"] = rng.integers(0, 8, n)
    k["angle"] = np.asarray(angles, f32)
    return k


def _fillers(rng, out, angles):
    for h, count in WIDE:
        for _ in range(count):
            out.append(_force_hash(rng.integers(0, 256, 32, dtype=np.uint8), h))
            angles.append(rng.uniform(0, 360))


def make_scene(nodes=6, seed=23):
    assert nodes >= 6
    rng = np.random.default_rng(seed + nodes)
    sf = SC.scale_factors(8)
    S = dict(nodes=nodes, sf=sf, sigma2=(sf * sf).astype(f32), cands=[], twinsF=[], twinsK=[])
    # ---- base: the fillers of the three wide nodes, their three real keypoints, then the other real keypoints
    bd, bang = [], []
    _fillers(rng, bd, bang)
    nfill = len(bd)
    for h, _ in WIDE:
        bd.append(_force_hash(rng.integers(0, 256, 32, dtype=np.uint8), h))
    for _ in range(N_REAL - len(WIDE)):
        bd.append(_plain(rng, nodes))
    real = list(range(nfill, nfill + N_REAL))           # indices of the real keypoints; real[:3] are the wide nodes' own
    bang += list(rng.uniform(0, 360, N_REAL))
    twin_src = real[3:3 + N_TWINS]                       # a of twinsK
    for a in twin_src:                                   # b: a near copy of a, later in a's node
        S["twinsK"].append((a, len(bd)))
        bd.append(_copy(rng, bd[a]))
        bang.append(bang[a])
    twinF_src = real[3 + N_TWINS:3 + 2 * N_TWINS]        # base keypoints that get two copies in every real candidate
    nb = len(bd)
    bmp = (rng.random(nb) < 0.8).astype(np.uint8)
    bmp[real[:3]] = 1
    for a, b in S["twinsK"]:
        bmp[a] = bmp[b] = 1
    bd = np.array(bd, np.uint8).reshape(nb, 32)
    S["base"] = dict(k=_keys(bang, rng), d=bd, fv=SC.bow(bd, nodes), mpW=bmp, real=real, partners=real[:3])
    # ---- the frame's right image: near copies of 150 real keypoints
    src = rng.permutation(real)[:150]
    rd = np.array([_copy(rng, bd[i]) for i in src], np.uint8).reshape(len(src), 32)
    S["right"] = dict(k=_keys([(bang[i] + rng.uniform(-3, 3)) % 360.0 for i in src], rng), d=rd, src=src)
    # ---- candidates
    plain_real = [i for i in real[3:] if i not in twinF_src and i not in twin_src]
    for j, (kind, n) in enumerate(KINDS):
        cd, cang, force_mp = [], [], []
        c = dict(kind=kind, partners=[], src=[])
        rot = ROTATIONS[j]

        def put(i):
            cd.append(_copy(rng, bd[i]))
            outlier = len(cd) % 10 == 0
            cang.append(rng.uniform(0, 360) if outlier else (bang[i] - rot + rng.uniform(-3, 3)) % 360.0)
            c["src"].append(i)
            return len(cd) - 1

        if kind == "small":
            for i in rng.permutation(plain_real)[:12]:
                put(int(i))
            while len(cd) < n:
                cd.append(_plain(rng, nodes)); cang.append(rng.uniform(0, 360)); c["src"].append(-1)
        elif kind != "empty":
            if j == 0:                                   # wide: fillers first, then the three partners
                _fillers(rng, cd, cang)
                c["src"] += [-1] * len(cd)
                for i in real[:3]:
                    c["partners"].append(put(i))
                force_mp += c["partners"]
            if kind == "real":
                for a in twin_src:
                    force_mp.append(put(a))
                for i in twinF_src:
                    first = put(i)
                    second = put(i)
                    cang[second] = cang[first]
                    S["twinsF"].append((j, i, first, second))
                    force_mp += [first, second]
            for i in rng.permutation(plain_real):
                if len(cd) >= n:
                    break
                put(int(i))
        assert len(cd) == n, (j, len(cd))
        c["k"] = _keys(cang, rng)
        c["d"] = np.array(cd, np.uint8).reshape(n, 32)
        c["mpW"], c["mpS"] = (rng.random(n) < 0.8).astype(np.uint8), (rng.random(n) < 0.7).astype(np.uint8)
        c["mpW"][force_mp] = 1
        c["mpS"][force_mp] = 1
        if kind == "nomp":
            c["mpW"][:] = 0
            c["mpS"][:] = 0
        fv = SC.bow(c["d"], nodes) if n else {}
        c["fv"] = {k + 1000: v for k, v in fv.items()} if kind == "nonode" else fv
        S["cands"].append(c)
    return S


# ---- views.  what: "frame" (candidates walked, base = F) or "kf" (base = pKF1 walked, candidates = pKF2)
def frame_arrays(S, fisheye=False):
    """(keys, descriptors, feature vector, n_left) of the frame: the base, for the fisheye variant followed by its right image."""
    B = S["base"]
    if not fisheye:
        return B["k"], B["d"], B["fv"], None
    k, d = np.concatenate([B["k"], S["right"]["k"]]), np.concatenate([B["d"], S["right"]["d"]])
    return k, d, SC.bow(d, S["nodes"]), len(B["k"])


def product_fixed(pkg, S, what, fisheye=False):
    if what == "kf":
        B = S["base"]
        return pkg.KeyFrameView(B["k"], B["d"], B["fv"], S["sf"], S["sigma2"], has_mappoint=B["mpW"])
    k, d, fv, _ = frame_arrays(S, fisheye)
    return pkg.KeyFrameView(k, d, fv, S["sf"], S["sigma2"])


def product_cand(pkg, S, j, what):
    c = S["cands"][j]
    return pkg.KeyFrameView(c["k"], c["d"], c["fv"], S["sf"], S["sigma2"], has_mappoint=c["mpS" if what == "kf" else "mpW"])


def oracle_fixed(oracle, S, what, fisheye=False):
    if what == "kf":
        B = S["base"]
        return oracle.OracleKeyFrame(B["k"], B["d"], B["fv"], S["sf"], S["sigma2"], has_mp=B["mpW"])
    k, d, fv, _ = frame_arrays(S, fisheye)
    return oracle.OracleKeyFrame(k, d, fv, S["sf"], S["sigma2"])


def oracle_cand(oracle, S, j, what):
    c = S["cands"][j]
    return oracle.OracleKeyFrame(c["k"], c["d"], c["fv"], S["sf"], S["sigma2"], has_mp=c["mpS" if what == "kf" else "mpW"])


NNRATIO = {"frame": 0.75, "kf": 0.9}      # Tracking.cc:3782 ORBmatcher matcher(0.75,true); LoopClosing.cc:661 ORBmatcher matcherBoW(0.9, true)


def oracle_rows(oracle, S, what, check_ori=True, fisheye=False, which=None):
    """The reference's loop on the oracle: (nmatches [K], rows [K, n]) of the per-pair member for the candidates `which`."""
    which = range(len(S["cands"])) if which is None else which
    fixed = oracle_fixed(oracle, S, what, fisheye)
    n_left = len(S["base"]["k"]) if fisheye else -1
    nm, rows = [], []
    for j in which:
        if what == "kf":
            n, row = oracle.search_by_bow_keyframes(fixed, oracle_cand(oracle, S, j, what), NNRATIO[what], check_ori)
        else:
            n, row = oracle.search_by_bow(oracle_cand(oracle, S, j, what), fixed, NNRATIO[what], check_ori, n_left=n_left)
        nm.append(n)
        rows.append(np.array(row, np.int32))
    return np.array(nm, np.int32), np.stack(rows) if rows else np.zeros((0, fixed.N), np.int32)


def make_uniform_scene(points, K, nodes, n_right=0, seed=31):
    """The shapes tools/bow_candidates_bench.py times: a base of `points` keypoints and K candidates of `points` keypoints each, 70 %
    of them copies of base keypoints, the others unrelated; n_right > 0 adds a right image of near copies to the frame (and the same
    number of unrelated keypoints to every candidate, which a rig keyframe has).  The dict has the layout of make_scene."""
    rng = np.random.default_rng(seed)
    sf = SC.scale_factors(8)
    S = dict(nodes=nodes, sf=sf, sigma2=(sf * sf).astype(f32), cands=[], twinsF=[], twinsK=[])
    bd = rng.integers(0, 256, (points, 32), dtype=np.uint8)
    bang = rng.uniform(0, 360, points)
    S["base"] = dict(k=_keys(bang, rng), d=bd, fv=SC.bow(bd, nodes), mpW=(rng.random(points) < 0.8).astype(np.uint8), real=list(range(points)), partners=[])
    src = rng.permutation(points)[:n_right]
    rd = np.array([_copy(rng, bd[i]) for i in src], np.uint8).reshape(len(src), 32)
    S["right"] = dict(k=_keys([(bang[i] + rng.uniform(-3, 3)) % 360.0 for i in src], rng), d=rd, src=src)
    for j in range(K):
        n = points + n_right
        rot = rng.uniform(0, 360)
        d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        ang = rng.uniform(0, 360, n)
        copies = rng.permutation(points)[:(7 * points) // 10]
        at = rng.permutation(n)[:len(copies)]
        for i, o in zip(copies, at):
            d[o] = _copy(rng, bd[i])
            if o % 10:
                ang[o] = (bang[i] - rot + rng.uniform(-3, 3)) % 360.0
        c = dict(kind="real", k=_keys(ang, rng), d=d, fv=SC.bow(d, nodes), partners=[], src=[])
        c["mpW"], c["mpS"] = (rng.random(n) < 0.8).astype(np.uint8), (rng.random(n) < 0.7).astype(np.uint8)
        S["cands"].append(c)
    return S


_cache = {}


def scene(nodes=6):
    """make_scene, built once per process; the tests leave it unchanged."""
    if nodes not in _cache:
        _cache[nodes] = make_scene(nodes)
    return _cache[nodes]
