"""A literal Python model of LocalMapping::KeyFrameCulling (LocalMapping.cc:1158-1310) under the non-inertial rule, over the flat scene
of orbm_culling_t.  Nothing is flattened while it runs: every map point keeps a real dict of observations, KeyFrame.SetBadFlag
(KeyFrame.cc:639-677), MapPoint.EraseObservation (MapPoint.cc:168-202) and MapPoint.SetBadFlag (MapPoint.cc:217-226) are written as the
reference writes them, and the loop runs one keyframe at a time in the list's order.

`product` and `erase` select deliberately WRONG neighbours of the statement, so that a scene can show it tells them apart:
product="double" multiplies redundant_th by nMPs in double; erase="per_row" subtracts once per row of the culled keyframe instead of
once per observation."""
import numpy as np


class MapPoint:
    def __init__(self, n_obs, bad):
        self.nObs, self.mbBad, self.mObservations = int(n_obs), bool(bad), {}

    def isBad(self):
        return self.mbBad

    def Observations(self):
        return self.nObs

    def GetObservations(self):
        return dict(self.mObservations)            # a copy, as the reference takes one under the lock (:1227)

    def EraseObservation(self, pKF):
        bBad = False
        if pKF in self.mObservations:                              # MapPoint.cc:173
            level, w = self.mObservations[pKF]
            self.nObs -= w                                         # :179-187
            del self.mObservations[pKF]                            # :189
            if self.nObs <= 2:                                     # :195
                bBad = True
        if bBad:
            self.SetBadFlag()

    def SetBadFlag(self):
        self.mbBad = True
        self.mObservations.clear()                                 # MapPoint.cc:223-225


class KeyFrame:
    def __init__(self, index, skip, th_depth, points, levels, depths):
        self.index, self.skip, self.mThDepth = index, bool(skip), np.float32(th_depth)
        self.mvpMapPoints, self.levels, self.mvDepth = points, levels, depths
        self.mbBad = False

    def SetBadFlag(self, per_row=False):
        again = {}                                                 # per_row only: what a second row of the same point subtracts again
        for pMP in self.mvpMapPoints:                              # KeyFrame.cc:670-677
            if pMP is not None:
                if per_row and id(pMP) in again and not pMP.isBad():
                    pMP.nObs -= again[id(pMP)]                     # the wrong neighbour: once per row
                    if pMP.nObs <= 2:
                        pMP.SetBadFlag()
                    continue
                if self in pMP.mObservations:
                    again[id(pMP)] = pMP.mObservations[self][1]
                pMP.EraseObservation(self)
        self.mbBad = True


def build(scene):
    """(keyframes, points) as objects.  An observer outside the list (obs_kf = -1) is a key of its own; a point that is bad on entry
    holds no observations (MapPoint::SetBadFlag cleared them)."""
    K, P = len(scene["row_start"]) - 1, len(scene["obs_start"]) - 1
    points = [MapPoint(scene["n_obs"][p], scene["bad"][p]) for p in range(P)]
    kfs = []
    for k in range(K):
        a, b = scene["row_start"][k], scene["row_start"][k + 1]
        rows = [points[p] if p >= 0 else None for p in scene["row_point"][a:b]]
        depth = None if scene.get("row_depth") is None else np.asarray(scene["row_depth"][a:b], np.float32)
        kfs.append(KeyFrame(k, scene["skip"][k], scene["th_depth"][k], rows, [int(v) for v in scene["row_level"][a:b]], depth))
    for p, pMP in enumerate(points):
        if pMP.mbBad:
            continue
        for e in range(scene["obs_start"][p], scene["obs_start"][p + 1]):
            kf = int(scene["obs_kf"][e])
            key = kfs[kf] if kf >= 0 else ("outside", e)
            assert key not in pMP.mObservations
            pMP.mObservations[key] = (int(scene["obs_level"][e]), int(scene["obs_w"][e]))
    return kfs, points


def counts(pKF, mono):
    """LocalMapping.cc:1204-1264 for one keyframe: (nMPs, nRedundantObservations)."""
    thObs = 3
    nRedundantObservations = nMPs = 0
    for i, pMP in enumerate(pKF.mvpMapPoints):
        if pMP is None or pMP.isBad():
            continue
        if not mono:
            if pKF.mvDepth[i] > pKF.mThDepth or pKF.mvDepth[i] < 0:
                continue
        nMPs += 1
        if pMP.Observations() > thObs:
            scaleLevel = pKF.levels[i]
            nObs = 0
            for pKFi, (scaleLeveli, _) in pMP.GetObservations().items():
                if pKFi is pKF:
                    continue
                if scaleLeveli <= scaleLevel + 1:
                    nObs += 1
                    if nObs > thObs:
                        break
            if nObs > thObs:
                nRedundantObservations += 1
    return nMPs, nRedundantObservations


def passes(nRed, th, nMPs, product="float"):
    if product == "double":
        return nRed > float(np.float32(th)) * nMPs
    return bool(np.float32(nRed) > np.float32(th) * np.float32(nMPs))    # :1266 as C evaluates it


def run(scene, erasable=None, applied=None, product="float", erase="once"):
    """The loop.  erasable [K] = !mbNotErase (None = all); applied(k) -> bool, when given, decides instead whether a passing keyframe is
    erased (the stepwise form's caller).  Returns dict(n_mps, n_red, culled, passing, n_obs, bad): passing = the unskipped keyframes
    that passed the test, in order."""
    kfs, points = build(scene)
    K = len(kfs)
    n_mps, n_red, culled, passing = np.zeros(K, np.int32), np.zeros(K, np.int32), np.zeros(K, np.uint8), []
    for k, pKF in enumerate(kfs):
        if pKF.skip or pKF.mbBad:                                  # :1200
            continue
        n_mps[k], n_red[k] = counts(pKF, bool(scene["mono"]))
        if passes(n_red[k], scene["redundant_th"], n_mps[k], product):
            passing.append(k)
            if applied(k) if applied is not None else (erasable is None or erasable[k]):
                pKF.SetBadFlag(per_row=erase == "per_row")
                culled[k] = 1
    return dict(n_mps=n_mps, n_red=n_red, culled=culled, passing=passing,
                n_obs=np.array([p.nObs for p in points], np.int32).reshape(-1), bad=np.array([p.mbBad for p in points], np.uint8).reshape(-1))
