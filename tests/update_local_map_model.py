"""A literal model of Tracking::UpdateLocalKeyFrames / UpdateLocalPoints (Tracking.cc:3559-3762) and KeyFrame::UpdateConnections with
AddConnection / UpdateBestCovisibles (KeyFrame.cc:205-242, :407-530): real objects, a dict per std::map and a set per std::set, both
iterated in POINTER order (the `ptr` attribute), the reference's stamps.  Nothing here is shared with the library; flatten() turns a
world into the arrays of orbm_map_graph_t.

The functions also return a trace of what happened (which branch took which keyframe), so that the tests can assert, on the model alone,
that a scene holds the case it was built for."""
import numpy as np


class MapPoint:
    def __init__(self, idx):
        self.idx, self.bad, self.obs = idx, False, {}              # obs: KeyFrame -> True  (mObservations)
        self.mnTrackReferenceForFrame = 0

    def isBad(self):
        return self.bad


class KeyFrame:
    def __init__(self, slot, ptr, mnId=None, map_id=0):
        self.slot, self.ptr, self.mnId, self.map = slot, ptr, slot if mnId is None else mnId, map_id
        self.bad = False
        self.mvpMapPoints = []                                      # MapPoint or None
        self.mConnectedKeyFrameWeights = {}
        self.mvpOrderedConnectedKeyFrames, self.mvOrderedWeights = [], []
        self.mspChildrens, self.mpParent, self.mPrevKF = set(), None, None
        self.mbFirstConnection = True
        self.mnTrackReferenceForFrame = 0

    def isBad(self):
        return self.bad

    def GetBestCovisibilityKeyFrames(self, N):
        return list(self.mvpOrderedConnectedKeyFrames[:N])

    # KeyFrame.cc:205-218
    def AddConnection(self, pKF, weight):
        if pKF not in self.mConnectedKeyFrameWeights:
            self.mConnectedKeyFrameWeights[pKF] = weight
        elif self.mConnectedKeyFrameWeights[pKF] != weight:
            self.mConnectedKeyFrameWeights[pKF] = weight
        else:
            return
        self.UpdateBestCovisibles()

    # KeyFrame.cc:220-242
    def UpdateBestCovisibles(self):
        vPairs = [(w, kf) for kf, w in in_ptr_order(self.mConnectedKeyFrameWeights)]
        vPairs.sort(key=lambda wk: (wk[0], wk[1].ptr))
        lKFs, lWs = [], []
        for w, kf in vPairs:
            if not kf.isBad():
                lKFs.insert(0, kf)
                lWs.insert(0, w)
        self.mvpOrderedConnectedKeyFrames, self.mvOrderedWeights = lKFs, lWs


def in_ptr_order(d):
    """Iteration of a std::map<KeyFrame*, T> (items) or a std::set<KeyFrame*> (elements)."""
    if isinstance(d, dict):
        return sorted(d.items(), key=lambda kv: kv[0].ptr)
    return sorted(d, key=lambda kf: kf.ptr)


class World:
    def __init__(self, G, P, ptrs=None, init_kf_id=0):
        ptrs = list(range(G)) if ptrs is None else list(ptrs)
        self.kfs = [KeyFrame(g, 1000 + 16 * int(ptrs[g])) for g in range(G)]
        self.pts = [MapPoint(p) for p in range(P)]
        self.init_kf_id = init_kf_id

    def observe(self, g, p, rows=1):
        """Keyframe g observes point p: one entry of mObservations, `rows` rows of mvpMapPoints."""
        self.pts[p].obs[self.kfs[g]] = True
        self.kfs[g].mvpMapPoints.extend([self.pts[p]] * rows)


def update_local_keyframes(frame, frame_id, inertial, last_kf, no_parent_break=False):
    """Tracking.cc:3590-3762 with `frame` = mCurrentFrame.mvpMapPoints (a list that is changed in place).  Returns (mvpLocalKeyFrames,
    pKFmax, max, trace)."""
    tr = dict(nulled=[], voted_bad=[], first=0, neighbour=[], child=[], parent=[], parent_break_at=None, tail=[], tail_stop=None, tie=False)
    keyframeCounter = {}
    for i in range(len(frame)):
        pMP = frame[i]
        if pMP:
            if not pMP.isBad():
                for kf, _ in in_ptr_order(pMP.obs):
                    keyframeCounter[kf] = keyframeCounter.get(kf, 0) + 1
            else:
                frame[i] = None
                tr["nulled"].append(i)
    mx, pKFmax, local = 0, None, []
    for pKF, n in in_ptr_order(keyframeCounter):
        if pKF.isBad():
            tr["voted_bad"].append(pKF)
            continue
        if n > mx:
            mx, pKFmax = n, pKF
        local.append(pKF)
        pKF.mnTrackReferenceForFrame = frame_id
    tr["tie"] = sum(1 for kf, n in keyframeCounter.items() if n == mx and not kf.isBad()) > 1
    tr["first"] = end = len(local)
    for i in range(end):
        if len(local) > 80:
            break
        pKF = local[i]
        skipped = []
        for pNeighKF in pKF.GetBestCovisibilityKeyFrames(10):
            if not pNeighKF.isBad():
                if pNeighKF.mnTrackReferenceForFrame != frame_id:
                    local.append(pNeighKF)
                    pNeighKF.mnTrackReferenceForFrame = frame_id
                    tr["neighbour"].append((pKF, pNeighKF, tuple(skipped)))
                    break
                skipped.append("marked")
            else:
                skipped.append("bad")
        skipped = []
        for pChildKF in in_ptr_order(pKF.mspChildrens):
            if not pChildKF.isBad():
                if pChildKF.mnTrackReferenceForFrame != frame_id:
                    local.append(pChildKF)
                    pChildKF.mnTrackReferenceForFrame = frame_id
                    tr["child"].append((pKF, pChildKF, tuple(skipped)))
                    break
                skipped.append("marked")
            else:
                skipped.append("bad")
        pParent = pKF.mpParent
        if pParent:
            if pParent.mnTrackReferenceForFrame != frame_id:
                local.append(pParent)
                pParent.mnTrackReferenceForFrame = frame_id
                tr["parent"].append((pKF, pParent))
                if not no_parent_break:
                    tr["parent_break_at"] = i
                    break
    if inertial and len(local) < 80:
        tempKeyFrame = last_kf
        for i in range(20):
            if not tempKeyFrame:
                tr["tail_stop"] = "null"
                break
            if tempKeyFrame.mnTrackReferenceForFrame != frame_id:
                local.append(tempKeyFrame)
                tempKeyFrame.mnTrackReferenceForFrame = frame_id
                tr["tail"].append(tempKeyFrame)
                tempKeyFrame = tempKeyFrame.mPrevKF
            elif tr["tail_stop"] is None:
                tr["tail_stop"] = "marked"
    return local, pKFmax, mx, tr


def update_local_points(local, frame_id):
    """Tracking.cc:3559-3587.  Returns (mvpLocalMapPoints, for each of them the list position of the keyframe it was taken from)."""
    pts, taken_at = [], []
    for j in range(len(local) - 1, -1, -1):
        for pMP in local[j].mvpMapPoints:
            if not pMP:
                continue
            if pMP.mnTrackReferenceForFrame == frame_id:
                continue
            if not pMP.isBad():
                pts.append(pMP)
                taken_at.append(j)
                pMP.mnTrackReferenceForFrame = frame_id
    return pts, taken_at


def kf_counter(pKF):
    """KeyFrame.cc:409-439."""
    KFcounter = {}
    for pMP in list(pKF.mvpMapPoints):
        if not pMP:
            continue
        if pMP.isBad():
            continue
        for kf, _ in in_ptr_order(pMP.obs):
            if kf.mnId == pKF.mnId or kf.isBad() or kf.map != pKF.map:
                continue
            KFcounter[kf] = KFcounter.get(kf, 0) + 1
    return KFcounter


def update_connections(pKF, init_kf_id, th=15):
    """KeyFrame::UpdateConnections (KeyFrame.cc:407-530) on the live objects.  Returns (pKFmax, nmax) or None for an empty counter."""
    KFcounter = kf_counter(pKF)
    if not KFcounter:
        return None
    nmax, pKFmax, vPairs = 0, None, []
    for kf, n in in_ptr_order(KFcounter):
        if n > nmax:
            nmax, pKFmax = n, kf
        if n >= th:
            vPairs.append((n, kf))
            kf.AddConnection(pKF, n)
    if not vPairs:
        vPairs.append((nmax, pKFmax))
        pKFmax.AddConnection(pKF, nmax)
    vPairs.sort(key=lambda wk: (wk[0], wk[1].ptr))
    lKFs, lWs = [], []
    for w, kf in vPairs:
        lKFs.insert(0, kf)
        lWs.insert(0, w)
    pKF.mConnectedKeyFrameWeights = dict(KFcounter)
    pKF.mvpOrderedConnectedKeyFrames, pKF.mvOrderedWeights = lKFs, lWs
    if pKF.mbFirstConnection and pKF.mnId != init_kf_id:
        pKF.mpParent = pKF.mvpOrderedConnectedKeyFrames[0]
        pKF.mpParent.mspChildrens.add(pKF)
        pKF.mbFirstConnection = False
    return pKFmax, nmax


def apply_rows(world, pKF, row, th=15):
    """What the adapter's helper does with the one-call rows of pKF (conn_kf, conn_w, ord_kf, ord_w as slot / weight lists): the member's
    writes, in the member's order."""
    if len(row["conn_kf"]) == 0:
        return
    kfs = world.kfs
    any_pair = False
    for k, w in zip(row["conn_kf"], row["conn_w"]):                  # rank order: the order of the AddConnection calls (:455-469)
        if w >= th:
            kfs[k].AddConnection(pKF, int(w))
            any_pair = True
    if not any_pair:
        kfs[row["kf_max"]].AddConnection(pKF, int(row["nmax"]))
    pKF.mConnectedKeyFrameWeights = {kfs[k]: int(w) for k, w in zip(row["conn_kf"], row["conn_w"])}
    pKF.mvpOrderedConnectedKeyFrames = [kfs[k] for k in row["ord_kf"]]
    pKF.mvOrderedWeights = [int(w) for w in row["ord_w"]]
    if pKF.mbFirstConnection and pKF.mnId != world.init_kf_id:
        pKF.mpParent = pKF.mvpOrderedConnectedKeyFrames[0]
        pKF.mpParent.mspChildrens.add(pKF)
        pKF.mbFirstConnection = False


def connection_state(world):
    """Everything UpdateConnections can write, of every keyframe, as plain values."""
    return [(sorted((k.slot, w) for k, w in kf.mConnectedKeyFrameWeights.items()), [k.slot for k in kf.mvpOrderedConnectedKeyFrames],
             list(kf.mvOrderedWeights), kf.mpParent.slot if kf.mpParent else -1, sorted(k.slot for k in kf.mspChildrens), kf.mbFirstConnection)
            for kf in world.kfs]


def flatten(world):
    """The arrays of orbm_map_graph_t (include/orbhip.h) from the live objects."""
    kfs, pts = world.kfs, world.pts
    G = len(kfs)
    rank = np.empty(G, np.int32)
    rank[np.argsort([kf.ptr for kf in kfs], kind="stable")] = np.arange(G, dtype=np.int32)
    row_start, rows, child_start, childs = [0], [], [0], []
    best = np.full((G, 10), -1, np.int32)
    for kf in kfs:
        rows.extend(-1 if mp is None else mp.idx for mp in kf.mvpMapPoints)
        row_start.append(len(rows))
        childs.extend(c.slot for c in in_ptr_order(kf.mspChildrens))
        child_start.append(len(childs))
        b = kf.GetBestCovisibilityKeyFrames(10)
        best[kf.slot, :len(b)] = [k.slot for k in b]
    obs_start, obs = [0], []
    for mp in pts:
        obs.extend(k.slot for k, _ in in_ptr_order(mp.obs))
        obs_start.append(len(obs))
    i32 = lambda x: np.asarray(x, np.int32).reshape(-1)
    return dict(kf_rank=rank, kf_bad=np.array([kf.bad for kf in kfs], np.uint8), kf_map=i32([kf.map for kf in kfs]), kf_row_start=i32(row_start),
                row_point=i32(rows), kf_best=best.reshape(-1), kf_child_start=i32(child_start), kf_child=i32(childs),
                kf_parent=i32([kf.mpParent.slot if kf.mpParent else -1 for kf in kfs]),
                kf_prev=i32([kf.mPrevKF.slot if kf.mPrevKF else -1 for kf in kfs]), pt_bad=np.array([mp.bad for mp in pts], np.uint8),
                obs_start=i32(obs_start), obs_kf=i32(obs))


def run_local_map(world, frame_point, inertial, last_kf, frame_id=7, no_parent_break=False):
    """UpdateLocalMap on a world for a frame given as point indices (-1 = NULL).  Returns the entries' outputs as arrays, and the trace."""
    frame = [None if p < 0 else world.pts[p] for p in frame_point]
    local, pKFmax, mx, tr = update_local_keyframes(frame, frame_id, inertial, None if last_kf < 0 else world.kfs[last_kf], no_parent_break)
    pts, taken_at = update_local_points(local, frame_id)
    slot_bad = np.zeros(len(frame_point), np.uint8)
    slot_bad[tr["nulled"]] = 1
    tr["taken_at"] = taken_at
    return dict(local_kf=np.array([k.slot for k in local], np.int32), kf_max=pKFmax.slot if pKFmax else -1, max_votes=mx, slot_bad=slot_bad,
                local_point=np.array([p.idx for p in pts], np.int32)), tr


def connection_rows(world, targets, th=15):
    """What orbm_update_connections returns, from the model: for each target the counter in pointer order and the ordered lists, computed
    WITHOUT writing anything (the state at entry)."""
    out = []
    for t in targets:
        pKF = world.kfs[t]
        items = in_ptr_order(kf_counter(pKF))
        nmax, pKFmax, vPairs = 0, None, []
        for kf, n in items:
            if n > nmax:
                nmax, pKFmax = n, kf
            if n >= th:
                vPairs.append((n, kf))
        if items and not vPairs:
            vPairs.append((nmax, pKFmax))
        vPairs.sort(key=lambda wk: (wk[0], wk[1].ptr))
        vPairs.reverse()
        out.append(dict(conn_kf=np.array([k.slot for k, _ in items], np.int32), conn_w=np.array([n for _, n in items], np.int32),
                        ord_kf=np.array([k.slot for _, k in vPairs], np.int32), ord_w=np.array([w for w, _ in vPairs], np.int32),
                        kf_max=pKFmax.slot if pKFmax else -1, nmax=nmax))
    return out
