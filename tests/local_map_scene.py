"""Scenes for Tracking::UpdateLocalMap and KeyFrame::UpdateConnections: worlds of tests/update_local_map_model.py with a frame and a list of
targets.  build(name, order) makes a fresh world (the model stamps and rewires its objects); order = "identity" | "reversed" | an int
seed says how the keyframes' addresses are ordered against their slots (RANK RULE, include/orbhip.h).

Small scenes are built by hand for one case each (tests/test_local_map_abi.py asserts on the model's trace that the case is there);
the shape scenes exercise the sizes at which the kernels change their path."""
import numpy as np

import update_local_map_model as LM


def _ptrs(G, order):
    if order == "identity":
        return np.arange(G)
    if order == "reversed":
        return np.arange(G)[::-1]
    return np.random.RandomState(int(order)).permutation(G)


def _scene(world, frame, inertial=False, last_kf=-1, targets=()):
    return dict(world=world, frame_point=np.asarray(frame, np.int32), inertial=inertial, last_kf=last_kf, targets=list(targets))


def tie_bad(order):
    """Keyframes 1 and 2 tie for the most votes (rank decides); keyframe 3 is voted and bad; point 0 sits in two slots; point 5 is bad and
    sits in a slot; point 2 lies twice in keyframe 1's rows; the last-listed keyframe shares a point with an earlier one."""
    W = LM.World(5, 8, _ptrs(5, order))
    for g, p in [(0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (3, 1), (0, 6), (4, 7), (0, 5), (3, 3), (2, 3), (1, 3)]:
        W.observe(g, p)
    W.observe(1, 2, rows=2)
    W.observe(2, 2)
    W.kfs[2].mvpMapPoints.insert(1, None)
    W.kfs[3].bad = True
    W.pts[5].bad = True
    return _scene(W, [0, -1, 1, 0, 5, 2], targets=[0, 1, 2, 3, 4])


def first_n(n, order):
    """n voted keyframes (slots 0..n-1, one frame point each), and behind them, for voted keyframe 0: neighbours [a voted one, a bad one,
    X], children {a bad one, a voted one, C1, C2}, a BAD parent.  n = 80: the first trip of the expansion appends X, the first good child in
    set order and the bad parent, and the list ends at 83."""
    G = n + 6
    W = LM.World(G, n + 4, _ptrs(G, order))
    for g in range(n):
        W.observe(g, g)
    X, B, C1, C2, CB, PB = (W.kfs[n + i] for i in range(6))
    B.bad = CB.bad = PB.bad = True
    for j, kf in enumerate((X, B, C1, C2, CB, PB)):                  # their own points, so that the local points differ
        W.observe(kf.slot, n + (j % 4))
    for kf in W.kfs[:n]:                                              # every voted keyframe has the same surroundings: whichever is first in
        kf.mvpOrderedConnectedKeyFrames = [W.kfs[(kf.slot + 1) % n], B, X]   # rank order takes them
        kf.mspChildrens = {CB, W.kfs[(kf.slot + 2) % n], C1, C2}
        kf.mpParent = PB
    return _scene(W, list(range(n)))


def parent_break(order):
    """Five voted keyframes.  The first in rank order has an unmarked parent: its break ends the expansion, although every later keyframe
    has an unmarked neighbour that the loop would have added."""
    W = LM.World(12, 12, _ptrs(12, order))
    for g in range(5):
        W.observe(g, g)
        W.observe(g, 5)
    for g in range(5, 12):
        W.observe(g, g)
    for g in range(5):
        W.kfs[g].mvpOrderedConnectedKeyFrames = [W.kfs[5 + g]]
        W.kfs[g].mpParent = W.kfs[10]
    W.kfs[11].mspChildrens = set()
    return _scene(W, [0, 1, 2, 3, 4, 5])


def tail(order, to_marked):
    """Inertial: the temporal walk from last_kf = 7 goes 7 -> 6 -> 5 and then either meets the voted keyframe 1 (marked: the walk stands
    still) or runs off the end (-1)."""
    W = LM.World(8, 8, _ptrs(8, order))
    for g in range(3):
        W.observe(g, g)
    for g in range(3, 8):
        W.observe(g, g)
        W.observe(g, 0)                                               # point 0 is not in the frame: they get no vote
    for g in (7, 6):
        W.kfs[g].mPrevKF = W.kfs[g - 1]
    W.kfs[5].mPrevKF = W.kfs[1] if to_marked else None
    W.kfs[1].mPrevKF = W.kfs[4]
    return _scene(W, [1, 2], inertial=True, last_kf=7)


def connections(order):
    """Target 0: weights 15 with keyframes 1 and 3 (a tie that rank orders), 14 with keyframe 2, and observers that do not count: itself,
    the bad keyframe 4, keyframe 5 of another map.  Point 60 lies twice in target 0's rows and once in keyframe 1's (a rig): 0 -> 1 weighs 15,
    1 -> 0 weighs 14.  Target 6 shares at most 3 points with anyone (the fallback pair).  Target 7 holds only a bad point and a NULL (the empty
    counter)."""
    W = LM.World(9, 80, _ptrs(9, order))
    for p in range(13):
        W.observe(0, p); W.observe(1, p)
    W.observe(0, 60, rows=2); W.observe(1, 60)
    for p in range(13, 27):
        W.observe(0, p); W.observe(2, p)
    for p in range(27, 42):
        W.observe(0, p); W.observe(3, p)
    for p in range(0, 20):
        W.observe(4, p); W.observe(5, p)
    W.kfs[4].bad = True
    W.kfs[5].map = 1
    for p in range(42, 45):
        W.observe(6, p); W.observe(8, p)
    W.observe(6, 45); W.observe(1, 45)
    W.observe(7, 46); W.observe(2, 46)
    W.pts[46].bad = True
    W.kfs[7].mvpMapPoints.append(None)
    return _scene(W, [0, 42], targets=[0, 1, 2, 3, 6, 7, 8])


def _pick(r, G, k):
    """k distinct keyframes out of G, in drawing order."""
    k = min(int(k), G)
    if 4 * k >= G:
        return [int(g) for g in r.choice(G, size=k, replace=False)]
    got = {}
    while len(got) < k:
        for g in r.randint(G, size=k):
            if len(got) < k:
                got[int(g)] = True
    return list(got)


def random_world(seed, G, P, order, obs=(1, 6), frame_n=60, frame_pool=None, long_lists=(), big_kf=None, empty_kf=None, p_bad_kf=0.1, p_bad_pt=0.05,
                 inertial=False, n_targets=4):
    """A seeded random world.  obs = (lo, hi): observers per point; long_lists: exact observer counts for the first points; big_kf =
    (slot, rows): pad that keyframe's rows to `rows`; empty_kf: a keyframe without rows; frame_pool: the points the frame draws from."""
    r = np.random.RandomState(seed)
    W = LM.World(G, P, _ptrs(G, order))
    for p in range(P):
        k = long_lists[p] if p < len(long_lists) else r.randint(obs[0], obs[1] + 1)
        for g in _pick(r, G, k):
            if g != empty_kf:
                W.observe(int(g), p, rows=2 if r.rand() < 0.03 else 1)
    for kf in W.kfs:
        kf.bad = bool(r.rand() < p_bad_kf)
        kf.map = int(r.rand() < 0.05)
        for j in sorted(r.choice(len(kf.mvpMapPoints) + 1, size=min(3, len(kf.mvpMapPoints) + 1), replace=False))[::-1]:
            if kf.slot != empty_kf:                                   # the empty keyframe stays without a single row, NULL rows included
                kf.mvpMapPoints.insert(int(j), None)
        kf.mvpOrderedConnectedKeyFrames = [W.kfs[g] for g in _pick(r, G, r.randint(0, 13)) if g != kf.slot]
        kf.mspChildrens = {W.kfs[g] for g in _pick(r, G, r.randint(0, 4)) if g != kf.slot}
        kf.mpParent = W.kfs[int(r.randint(G))] if r.rand() < 0.6 and G > 1 else None
        kf.mPrevKF = W.kfs[kf.slot - 1] if kf.slot > 0 else None
    for mp in W.pts:
        mp.bad = bool(r.rand() < p_bad_pt)
    if big_kf is not None:
        kf = W.kfs[big_kf[0]]
        kf.bad = False                                                # it has to reach the local list: a bad keyframe comes in as a parent only
        kf.mvpMapPoints = (kf.mvpMapPoints + [W.pts[int(p)] if p >= 0 else None for p in r.randint(-1, P, size=big_kf[1])])[:big_kf[1]]
    if empty_kf is not None:                                          # the keyframe without rows is everybody's first neighbour
        W.kfs[empty_kf].bad = False
        for kf in W.kfs:
            if kf.slot != empty_kf:
                kf.mvpOrderedConnectedKeyFrames.insert(0, W.kfs[empty_kf])
    pool = np.arange(P) if frame_pool is None else np.asarray(frame_pool)
    frame = np.where(r.rand(frame_n) < 0.3, -1, pool[r.randint(len(pool), size=frame_n)]) if frame_n else np.zeros(0, np.int32)
    return _scene(W, frame, inertial=inertial, last_kf=G - 1 if inertial else -1, targets=_pick(r, G, n_targets))


def voted(n, order):
    """Exactly n voted keyframes out of n + 40: the frame holds one point per keyframe 0..n-1 that only this keyframe observes."""
    S = random_world(100 + n, n + 40, n + 200, order, frame_n=0, p_bad_kf=0.0)
    W = S["world"]
    for mp in W.pts[:n]:
        mp.obs, mp.bad = {}, False
    for g in range(n):
        W.pts[g].obs[W.kfs[g]] = True
    S["frame_point"] = np.arange(n, dtype=np.int32)
    return S


def rows(order):
    """Keyframe 3 has 15 360 rows and is voted (the frame's first slot holds a live point that it observes), so it stands in the first list
    with the expansion's keyframes behind it; keyframe 5 has no row at all, is every keyframe's first neighbour and so enters the list, and
    is a target like all the others."""
    S = random_world(21, 12, 500, order, big_kf=(3, 15360), empty_kf=5, frame_n=80, n_targets=12)
    W = S["world"]
    seen = next(mp for mp in W.pts if W.kfs[3] in mp.obs and not mp.bad)
    S["frame_point"][0] = seen.idx
    return S


CASES = {
    "tie_bad": tie_bad,
    "first79": lambda o: first_n(79, o), "first80": lambda o: first_n(80, o), "first81": lambda o: first_n(81, o),
    "parent_break": parent_break,
    "tail_marked": lambda o: tail(o, True), "tail_end": lambda o: tail(o, False),
    "connections": connections,
    "random": lambda o: random_world(1, 40, 300, o, frame_n=90, inertial=True),
    "random_dense": lambda o: random_world(2, 30, 200, o, obs=(3, 20), frame_n=120, n_targets=30),
}
# the sizes at which a kernel changes its path (tests/test_gpu_local_map.py)
SHAPES = {
    "n1": lambda o: random_world(11, 20, 100, o, frame_n=1, p_bad_pt=0.0),
    "n63": lambda o: random_world(12, 20, 100, o, frame_n=63), "n64": lambda o: random_world(13, 20, 100, o, frame_n=64),
    "n65": lambda o: random_world(14, 20, 100, o, frame_n=65),
    "n15360": lambda o: random_world(15, 70, 4000, o, frame_n=15360, n_targets=65),
    "lists": lambda o: random_world(16, 140, 60, o, long_lists=(0, 1, 63, 64, 65, 129), frame_pool=np.arange(8), frame_n=40, p_bad_pt=0.0, n_targets=2),
    "g1": lambda o: random_world(17, 1, 30, o, obs=(0, 1), frame_n=20, n_targets=1), "g2": lambda o: random_world(18, 2, 30, o, obs=(0, 2), frame_n=20, n_targets=2),
    "g65": lambda o: random_world(19, 65, 400, o, frame_n=200, n_targets=65),
    "g16384": lambda o: random_world(20, 16384, 3000, o, obs=(1, 5), frame_n=300, n_targets=3),
    "voted1": lambda o: voted(1, o), "voted64": lambda o: voted(64, o), "voted65": lambda o: voted(65, o), "voted1025": lambda o: voted(1025, o),
    "rows": rows,
}
ALL = dict(CASES, **SHAPES)


def build(name, order="identity"):
    return ALL[name](order)
