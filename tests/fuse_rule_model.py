"""A small model of the objects LocalMapping::SearchInNeighbors' Fuse loop works on (LocalMapping.cc:989-1000, ORBmatcher.cc:1622-1645,
MapPoint.cc:141-166 and :249-301), for the replay of the FUSE RULE of include/orbhip.h.  A helper, not a conftest.

  MapPoint  observations {keyframe id: [left index, right index]}, nObs, a bad flag, a descriptor.  AddObservation and Replace follow
            MapPoint.cc; ComputeDistinctiveDescriptors goes through `distinctive` (oracle.distinctive_descriptor) over the observed rows,
            in the order of the observation map (std::map: here by keyframe id).
  KeyFrame  descriptor rows, mvuRight, NLeft (-1: one camera) and the per-keyframe point table.

replay_scene() puts them around the scene of tests/fuse_keyframes_scene.py; run_sequential() is the reference's loop - the search of
target t from the LIVE state, then the bookkeeping -, run_one_call() the rule: every row from the state at loop entry, the live test in
front of each entry, and a search of target t on the subset of points whose descriptor no longer is the uploaded one."""
import copy

import numpy as np

import fuse_keyframes_scene as FS

ORDER = (0, 1, 2, 6, 3)       # the targets of the replay: 2 and 6 are the two images of one rig keyframe, consecutive
HAND = 0                      # position in ORDER of the target in which the hand-made point gains observations ...
HAND_LATER = 4                # ... and of the later target whose answer for it changes


class MapPoint:
    def __init__(self, mid, desc):
        self.id, self.obs, self.nobs, self.bad, self.desc = mid, {}, 0, False, np.array(desc, np.uint8)

    def in_keyframe(self, kf):
        return kf.id in self.obs


class KeyFrame:
    def __init__(self, kid, desc, ur=None, n_left=-1):
        self.id, self.desc, self.n_left = kid, [np.array(d, np.uint8) for d in desc], n_left
        self.ur = [-1.0] * len(self.desc) if ur is None else [float(u) for u in ur]
        self.table = [None] * len(self.desc)

    def add_row(self, d, ur=-1.0):
        self.desc.append(np.array(d, np.uint8)); self.ur.append(float(ur)); self.table.append(None)
        return len(self.desc) - 1


class World:
    def __init__(self, distinctive):
        self.kfs, self.mps, self.distinctive = {}, [], distinctive
        self.replaced_searched = self.replaced_kf = 0           # Replace calls: the searched point loses / the keyframe's point loses
        self.kf_side_survivors = set()

    def new_point(self, desc):
        mp = MapPoint(len(self.mps), desc)
        self.mps.append(mp)
        return mp

    def add_observation(self, mp, kf, idx):                      # MapPoint.cc:141-166
        ind = mp.obs.get(kf.id, [-1, -1])
        ind[1 if kf.n_left != -1 and idx >= kf.n_left else 0] = idx
        mp.obs[kf.id] = ind
        mp.nobs += 2 if kf.n_left == -1 and kf.ur[idx] >= 0 else 1

    def observe(self, mp, kf, idx):                              # initial state: observation and table entry together
        self.add_observation(mp, kf, idx)
        kf.table[idx] = mp

    def compute_distinctive(self, mp):                           # MapPoint.cc:350-436
        if mp.bad or not mp.obs:
            return
        rows = [self.kfs[k].desc[i] for k in sorted(mp.obs) for i in mp.obs[k] if i != -1]
        if rows:
            mp.desc = rows[self.distinctive(np.array(rows, np.uint8))].copy()

    def replace(self, loser, winner):                            # loser->Replace(winner), MapPoint.cc:249-301
        if loser.id == winner.id:
            return
        obs, loser.obs, loser.bad = loser.obs, {}, True
        for k in sorted(obs):
            kf = self.kfs[k]
            if not winner.in_keyframe(kf):
                for i in obs[k]:
                    if i != -1:
                        kf.table[i] = winner
                        self.add_observation(winner, kf, i)
            else:
                for i in obs[k]:
                    if i != -1:
                        kf.table[i] = None
        self.compute_distinctive(winner)

    def fuse_body(self, mp, kf, best_idx, in_list):              # ORBmatcher.cc:1625-1645
        other = kf.table[best_idx]
        if other is not None:
            if not other.bad:
                if other.nobs > mp.nobs:
                    self.replace(mp, other)
                    self.replaced_searched += 1
                    if other.id in in_list:
                        self.kf_side_survivors.add(other.id)
                else:
                    self.replace(other, mp)
                    self.replaced_kf += 1
        else:
            self.add_observation(mp, kf, best_idx)
            kf.table[best_idx] = mp

    def state(self):
        return ([(mp.bad, sorted((k, tuple(v)) for k, v in mp.obs.items()), mp.nobs, mp.desc.tobytes()) for mp in self.mps],
                {k: [None if p is None else p.id for p in kf.table] for k, kf in self.kfs.items()})


def replay_scene(oracle, seed=5):
    """(S, world, points, kf_of): S = the scene restricted to ORDER with the hand-made keypoint added to its last target, world = the
    initial objects, points = the list vpMapPointMatches, kf_of[t] = (KeyFrame, index offset) of target t of S."""
    rng = np.random.default_rng(seed)
    S0 = FS.scene()
    S = FS.subset(S0, ORDER, np.arange(S0["nP"]))
    S["targets"] = [copy.deepcopy(tg) for tg in S["targets"]]
    W = World(oracle.distinctive_descriptor)
    nbg = 6
    for b in range(nbg):                                          # background keyframes, ids 100..: they only hold observed descriptor rows
        W.kfs[100 + b] = KeyFrame(100 + b, [])
    tg = S["targets"]
    kf_of = {}
    for t, o in enumerate(ORDER):
        if o == 6:                                                # the right image of the rig keyframe made for target 2
            kf_of[t] = (kf_of[ORDER.index(2)][0], len(tg[ORDER.index(2)]["k"]))
            continue
        desc = list(tg[t]["d"]) + (list(tg[ORDER.index(6)]["d"]) if o == 2 else [])
        ur = None if tg[t]["ur"] is None else tg[t]["ur"]
        W.kfs[t] = KeyFrame(t, desc, ur, n_left=len(tg[t]["k"]) if o == 2 else -1)
        kf_of[t] = (W.kfs[t], 0)

    def background(mp, count, base):
        for b in rng.permutation(nbg)[:count]:
            kf = W.kfs[100 + int(b)]
            W.observe(mp, kf, kf.add_row(FS._flip(base, int(rng.integers(0, 14)), rng)))

    points = []
    for i in range(S["nP"]):
        mp = W.new_point(S["mpdesc"][i])
        background(mp, int(rng.integers(1, 5)), S["mpdesc"][i])
        points.append(mp)
    # the keyframes' own points: behind 45 % of the keypoints a foreign point, behind 10 % a point of the list
    for t in range(len(ORDER)):
        kf, off = kf_of[t]
        for k in range(len(tg[t]["k"])):
            r = rng.random()
            if r < 0.45:
                q = W.new_point(tg[t]["d"][k])
                background(q, int(rng.integers(0, 6)), tg[t]["d"][k])
                W.observe(q, kf, off + k)
            elif r < 0.55:
                j = points[int(rng.integers(0, len(points)))]
                if not j.in_keyframe(kf):
                    W.observe(j, kf, off + k)
    # The hand-made case.  H is seen by target HAND at keypoint k, which holds Q with nObs(Q) = nObs(H) = 4: Q->Replace(H).  H brings two
    # rows (its descriptor D and a random one, in stereo keyframes: 2 observations each), Q three rows equal to D' = D with 40 bits flipped:
    # of the six rows D' has the least median distance, H's descriptor becomes D'.  The later target has keypoint m1 (a copy of D) and,
    # added here at m1's pixel and octave, m2 (a copy of D'): the loop-entry row says m1, the search at H's turn says m2.
    row_a, row_b = FS.oracle_row(oracle, S, HAND, 3.0)[1], FS.oracle_row(oracle, S, HAND_LATER, 3.0)[1]
    free = [i for i in range(S["nP"]) if S["group"][i] == 0 and row_a[i] >= 0 and row_b[i] >= 0 and S["valid"][HAND][i] and S["valid"][HAND_LATER][i]]
    h = free[0]
    H, D = points[h], S["mpdesc"][h].copy()
    for k_ in list(H.obs):                                        # H's own history: two stereo observations
        kf = W.kfs[k_]
        for i_ in H.obs[k_]:
            if i_ != -1:
                kf.table[i_] = None
    H.obs, H.nobs = {}, 0
    W.observe(H, W.kfs[100], W.kfs[100].add_row(D, 5.0))
    W.observe(H, W.kfs[102], W.kfs[102].add_row(rng.integers(0, 256, 32, dtype=np.uint8), 5.0))
    Dp = FS._flip(D, 40, rng)
    kfa, offa = kf_of[HAND]
    k = int(row_a[h])
    old = kfa.table[offa + k]
    if old is not None:                                           # whoever held k leaves it
        del old.obs[kfa.id]
        old.nobs -= 1
    Q = W.new_point(Dp)
    for b in (101, 103, 105):
        W.observe(Q, W.kfs[b], W.kfs[b].add_row(Dp))
    W.observe(Q, kfa, offa + k)
    assert H.nobs == 4 and Q.nobs == 4
    tb = tg[HAND_LATER]
    m1 = int(row_b[h])
    tb["k"] = np.concatenate([tb["k"], tb["k"][m1:m1 + 1]])
    tb["d"] = np.concatenate([tb["d"], FS._flip(Dp, 3, rng)[None]])
    kfb, _ = kf_of[HAND_LATER]
    kfb.add_row(tb["d"][-1])
    S["hand"] = dict(point=h, m1=m1, m2=len(tb["k"]) - 1)
    for t in range(len(ORDER)):                                   # H meets only the two targets of the case
        if t not in (HAND, HAND_LATER):
            S["valid"][t][h] = 0
    # validity at loop entry is the live test on the initial objects
    S["valid"] = np.array([[0 if (mp.bad or mp.in_keyframe(kf_of[t][0])) else int(S["valid"][t][i]) for i, mp in enumerate(points)]
                           for t in range(len(ORDER))], np.uint8)
    return S, W, points, kf_of


def _live(mp, kf, row_valid):
    return bool(row_valid) and not mp.bad and not mp.in_keyframe(kf)


def run_sequential(S, W, points, kf_of, search):
    """The reference's loop.  search(t, valid [nP], mpdesc [nP][32]) -> bestIdx [nP] of target t.  Returns nFused per target."""
    in_list = {mp.id for mp in points}
    nfused = []
    for t in range(len(S["targets"])):
        kf, off = kf_of[t]
        valid = np.array([_live(mp, kf, S["valid"][t][i]) for i, mp in enumerate(points)], np.uint8)
        row = search(t, valid, np.array([mp.desc for mp in points], np.uint8))
        n = 0
        for i, mp in enumerate(points):
            if valid[i] and row[i] >= 0:
                assert _live(mp, kf, 1)                           # nothing in front of i's turn takes a valid point away
                W.fuse_body(mp, kf, off + int(row[i]), in_list)
                n += 1
        nfused.append(n)
    return nfused


def run_one_call(S, W, points, kf_of, rows0, search, log=None):
    """The FUSE RULE.  rows0 [T][nP]: bestIdx from the state at loop entry (S["valid"], S["mpdesc"]).  log (a dict) receives `dirty`, the
    (target, point) pairs that were searched again, and `changed`, those whose answer differs from rows0."""
    in_list = {mp.id for mp in points}
    nfused = []
    dirty_log, changed = [], []
    for t in range(len(S["targets"])):
        kf, off = kf_of[t]
        row = np.array(rows0[t], np.int32)
        dirty = np.array([_live(mp, kf, S["valid"][t][i]) and mp.desc.tobytes() != S["mpdesc"][i].tobytes() for i, mp in enumerate(points)], np.uint8)
        if dirty.any():
            again = search(t, dirty, np.array([mp.desc for mp in points], np.uint8))
            for i in np.nonzero(dirty)[0]:
                dirty_log.append((t, int(i)))
                if again[i] != row[i]:
                    changed.append((t, int(i)))
                row[i] = again[i]
        n = 0
        for i, mp in enumerate(points):
            if _live(mp, kf, S["valid"][t][i]) and row[i] >= 0:
                W.fuse_body(mp, kf, off + int(row[i]), in_list)
                n += 1
        nfused.append(n)
    if log is not None:
        log["dirty"], log["changed"] = dirty_log, changed
    return nfused
