"""The loop body of LoopClosing::SearchAndFuse (LoopClosing.cc:2631-2707) on the small object model of tests/fuse_rule_model.py, for the
replay of the SEARCH-AND-FUSE RULE of include/orbhip.h.  A helper, not a conftest.

What differs from SearchInNeighbors' loop body (fuse_rule_model.World.fuse_body):
  * inside call t an empty keypoint gets AddObservation / AddMapPoint at once, an occupied one is only RECORDED in vpReplacePoint
    (ORBmatcher.cc:1768-1782); after the call every recorded point is replaced INTO the searched one, pRep->Replace(vpMapPoints[i])
    (:2654-2665), in index order;
  * validity is !isBad() && !spAlreadyFound.count(pMP), with spAlreadyFound = pKF->GetMapPoints() taken once at entry of call t (:1680,
    :1692): a point the call itself adds to the keyframe stays valid for its later entries in the list.

replay_scene() puts the objects around the scene of tests/fuse_sim3_keyframes_scene.py; run_sequential() is the reference's loop - the
search of target t from the LIVE state, then the body -, run_one_call() the rule: every row from the state at loop entry, the live test
of iteration t, and a search of target t on the subset of points whose descriptor no longer is the uploaded one."""
import copy

import numpy as np

import fuse_sim3_keyframes_scene as SS
from fuse_rule_model import KeyFrame, World

ORDER = (0, 1, 2, 6, 3)       # the targets of the replay, in the loop's order
HAND = 0                      # position in ORDER of the target in which the hand-made point H is replaced into ...
HAND_LATER = 4                # ... and of the later target whose answer for it changes
TH = 4.0


def replay_scene(oracle, seed=5):
    """(S, world, points, kfs): S = the scene restricted to ORDER with the hand-made keypoint added to its last target, world = the
    initial objects, points = the list vpMapPoints, kfs[t] = KeyFrame of target t of S.  S["twice"] = (i, j): points[i] is points[j];
    S["shared"] = (a, b, t, k): points a and b both answer the EMPTY keypoint k of target t; S["hand"]: the hand-made case."""
    rng = np.random.default_rng(seed)
    S0 = SS.scene()
    S = SS.subset(S0, ORDER, np.arange(S0["nP"]))
    S["targets"] = [copy.deepcopy(tg) for tg in S["targets"]]
    S["mpdesc"], S["valid"] = S["mpdesc"].copy(), S["valid"].copy()
    for key in ("Xw", "normal", "max_dist", "min_dist"):
        S[key] = S[key].copy()
    tg = S["targets"]
    row = [SS.oracle_row(oracle, S, t, TH)[1] for t in range(len(ORDER))]
    plain = lambda i, t: S["group"][i] == 0 and row[t][i] >= 0 and S["valid"][t][i]
    # A pointer listed twice: entry j becomes entry i (the same object: one position, one descriptor, one answer)
    i2 = next(i for i in range(S["nP"]) if plain(i, 1))
    j2 = next(j for j in range(i2 + 1, S["nP"]) if S["group"][j] == 0)
    for key in ("Xw", "normal", "mpdesc", "max_dist", "min_dist"):
        S[key][j2] = S[key][i2]
    S["valid"][:, j2] = S["valid"][:, i2]
    S["twice"] = (i2, j2)
    # Two points that answer one keypoint of target 2, which is left empty below: b takes a's position and a descriptor 2 bits from a's
    a2 = next(i for i in range(S["nP"]) if plain(i, 2) and i not in (i2, j2))
    b2 = next(j for j in range(a2 + 1, S["nP"]) if S["group"][j] == 0 and j not in (i2, j2))
    for key in ("Xw", "normal", "max_dist", "min_dist"):
        S[key][b2] = S[key][a2]
    S["mpdesc"][b2] = SS.FS._flip(S["mpdesc"][a2], 2, rng)
    S["valid"][:, b2] = S["valid"][:, a2]
    S["shared"] = (a2, b2, 2, int(row[2][a2]))
    row = [SS.oracle_row(oracle, S, t, TH)[1] for t in range(len(ORDER))]
    assert row[2][b2] == row[2][a2] == S["shared"][3] and row[1][j2] == row[1][i2] >= 0

    W = World(oracle.distinctive_descriptor)
    nbg = 6
    for b in range(nbg):                                          # background keyframes, ids 100..: they only hold observed descriptor rows
        W.kfs[100 + b] = KeyFrame(100 + b, [])
    kfs = {}
    for t in range(len(ORDER)):
        W.kfs[t] = kfs[t] = KeyFrame(t, list(tg[t]["d"]))

    def background(mp, count, base):
        for b in rng.permutation(nbg)[:count]:
            kf = W.kfs[100 + int(b)]
            W.observe(mp, kf, kf.add_row(SS.FS._flip(base, int(rng.integers(0, 14)), rng)))

    points = []
    for i in range(S["nP"]):
        if i == j2:
            points.append(points[i2])
            continue
        mp = W.new_point(S["mpdesc"][i])
        background(mp, int(rng.integers(1, 5)), S["mpdesc"][i])
        points.append(mp)
    # the keyframes' own points: behind 45 % of the keypoints a foreign point, behind 10 % a point of the list
    for t in range(len(ORDER)):
        for k in range(len(tg[t]["k"])):
            if (t, k) == S["shared"][2:]:
                continue
            r = rng.random()
            if r < 0.45:
                q = W.new_point(tg[t]["d"][k])
                background(q, int(rng.integers(0, 6)), tg[t]["d"][k])
                W.observe(q, kfs[t], k)
            elif r < 0.55:
                j = points[int(rng.integers(0, len(points)))]
                if not j.in_keyframe(kfs[t]) and j is not points[a2] and j is not points[b2]:
                    W.observe(j, kfs[t], k)
    # The hand-made case.  H answers keypoint k of target HAND, which holds Q: Q->Replace(H) after call HAND.  H brings two rows (its
    # descriptor D and a random one), Q three rows equal to D' = D with 40 bits flipped, and row k comes with the replacement: of the six
    # rows D' has the least median distance, H's descriptor becomes D'.  The later target has keypoint m1 (near D) and, added here at m1's
    # pixel and octave, m2 (near D'): the loop-entry row says m1, the search at the start of that iteration says m2.
    special = {i2, j2, a2, b2}
    free = [i for i in range(S["nP"]) if i not in special and plain(i, HAND) and plain(i, HAND_LATER)]
    h = free[0]
    H, D = points[h], S["mpdesc"][h].copy()
    for k_ in list(H.obs):
        kf = W.kfs[k_]
        for i_ in H.obs[k_]:
            if i_ != -1:
                kf.table[i_] = None
    H.obs, H.nobs = {}, 0
    W.observe(H, W.kfs[100], W.kfs[100].add_row(D))
    W.observe(H, W.kfs[102], W.kfs[102].add_row(rng.integers(0, 256, 32, dtype=np.uint8)))
    Dp = SS.FS._flip(D, 40, rng)
    k = int(row[HAND][h])
    old = kfs[HAND].table[k]
    if old is not None:                                           # whoever held k leaves it
        del old.obs[kfs[HAND].id]
        old.nobs -= 1
    Q = W.new_point(Dp)
    for b in (101, 103, 105):
        W.observe(Q, W.kfs[b], W.kfs[b].add_row(Dp))
    W.observe(Q, kfs[HAND], k)
    tb = tg[HAND_LATER]
    m1 = int(row[HAND_LATER][h])
    tb["k"] = np.concatenate([tb["k"], tb["k"][m1:m1 + 1]])
    tb["d"] = np.concatenate([tb["d"], SS.FS._flip(Dp, 3, rng)[None]])
    kfs[HAND_LATER].add_row(tb["d"][-1])
    S["hand"] = dict(point=h, m1=m1, m2=len(tb["k"]) - 1)
    for t in range(len(ORDER)):                                   # H meets only the two targets of the case
        if t not in (HAND, HAND_LATER):
            S["valid"][t][h] = 0
    # validity at loop entry is the live test on the initial objects
    S["valid"] = np.array([_valid(points, kfs[t], S["valid"][t]) for t in range(len(ORDER))], np.uint8)
    return S, W, points, kfs


def _valid(points, kf, row_valid):
    """valid of one Fuse call at its entry: !isBad() && !spAlreadyFound.count(pMP) (ORBmatcher.cc:1680, :1692), under the scene's own row."""
    found = {p.id for p in kf.table if p is not None and not p.bad}            # KeyFrame::GetMapPoints
    return np.array([bool(row_valid[i]) and not mp.bad and mp.id not in found for i, mp in enumerate(points)], np.uint8)


def _body(W, points, kf, valid, row):
    """ORBmatcher.cc:1768-1782 for every entry of the list, then LoopClosing.cc:2654-2665.  Returns nFused."""
    replace = [None] * len(points)
    n = 0
    for i, mp in enumerate(points):
        if not valid[i] or row[i] < 0:
            continue
        other = kf.table[int(row[i])]
        if other is not None:
            if not other.bad:
                replace[i] = other
        else:
            W.add_observation(mp, kf, int(row[i]))
            kf.table[int(row[i])] = mp
        n += 1
    for i, rep in enumerate(replace):
        if rep is not None:
            W.replace(rep, points[i])
            W.replaced_kf += 1
    return n


def _descs(points):
    return np.array([mp.desc for mp in points], np.uint8)


def run_sequential(S, W, points, kfs, search):
    """The reference's loop.  search(t, valid [nP], mpdesc [nP][32]) -> bestIdx [nP] of target t.  Returns nFused per target."""
    nfused = []
    for t in range(len(S["targets"])):
        valid = _valid(points, kfs[t], S["valid"][t])
        nfused.append(_body(W, points, kfs[t], valid, search(t, valid, _descs(points))))
    return nfused


def run_one_call(S, W, points, kfs, rows0, search, log=None):
    """The SEARCH-AND-FUSE RULE.  rows0 [T][nP]: bestIdx from the state at loop entry (S["valid"], S["mpdesc"]).  log (a dict) receives
    `dirty`, the (target, point) pairs that were searched again, and `changed`, those whose answer differs from rows0."""
    nfused, dirty_log, changed = [], [], []
    for t in range(len(S["targets"])):
        valid = _valid(points, kfs[t], S["valid"][t])
        assert not np.any(valid & ~S["valid"][t].astype(bool))                # validity only shrinks
        row = np.array(rows0[t], np.int32)
        dirty = np.array([valid[i] and mp.desc.tobytes() != S["mpdesc"][i].tobytes() for i, mp in enumerate(points)], np.uint8)
        if dirty.any():
            again = search(t, dirty, _descs(points))
            for i in np.nonzero(dirty)[0]:
                dirty_log.append((t, int(i)))
                if again[i] != row[i]:
                    changed.append((t, int(i)))
                row[i] = again[i]
        nfused.append(_body(W, points, kfs[t], valid, row))
    if log is not None:
        log["dirty"], log["changed"] = dirty_log, changed
    return nfused
