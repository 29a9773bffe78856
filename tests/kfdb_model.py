"""A literal Python restatement of KeyFrameDatabase.cc:39-98 (add, erase, clear, clearMap), :620-811 (DetectNBestCandidates),
:814-926 (DetectRelocalizationCandidates) and ScoringObject.cpp:23-68 (L1Scoring::score).

One object per keyframe carrying the members, a real list per word, the lists walked as the reference walks them.  Python floats stand
for the doubles; np.float32 stands wherever the reference holds a float (si, accScore, 0.75f * best, max * 0.8f).  It shares no code
with csrc/orb_ref_kfdb.h and does not use the ORDER RULE of include/orbhip.h."""
import bisect

import numpy as np

F32 = np.float32


class KF:
    def __init__(self, tag, map_id, bow, covisibles=()):
        self.tag = tag
        self.map = map_id
        self.bow = [(int(i), float(v)) for i, v in zip(*bow)]      # DBoW2::BowVector: a std::map, ascending
        self.covisibles = list(covisibles)                          # GetBestCovisibilityKeyFrames(10): KF objects
        self.bad = False
        self.mnRelocQuery = 0
        self.mnRelocWords = 0
        self.mRelocScore = F32(0)          # the reference leaves it uninitialised (KeyFrame.cc:34, :52); the handle says 0
        self.mnPlaceRecognitionQuery = 0
        self.mnPlaceRecognitionWords = 0
        self.mPlaceRecognitionScore = F32(0)

    def best_covisibles(self, n):
        return self.covisibles[:n]


def l1_score(v1, v2, stats=None):
    """ScoringObject.cpp:23-68."""
    k1 = [i for i, _ in v1]
    k2 = [i for i, _ in v2]
    a = b = 0
    score = 0.0
    while a != len(v1) and b != len(v2):
        vi = v1[a][1]
        wi = v2[b][1]
        if v1[a][0] == v2[b][0]:
            term = abs(vi - wi) - abs(vi) - abs(wi)
            score += term
            if stats is not None:
                stats.append((vi, wi))
            a += 1
            b += 1
        elif v1[a][0] < v2[b][0]:
            a = bisect.bisect_left(k1, v2[b][0])     # v1.lower_bound
        else:
            b = bisect.bisect_left(k2, v1[a][0])     # v2.lower_bound
    score = -score / 2.0
    return score


class Database:
    def __init__(self, n_words):
        self.n_words = n_words
        self.inverted = [[] for _ in range(n_words)]     # mvInvertedFile

    def add(self, kf):                                   # :39-45
        for wid, _ in kf.bow:
            self.inverted[wid].append(kf)

    def erase(self, kf):                                 # :47-66
        for wid, _ in kf.bow:
            lst = self.inverted[wid]
            for k, other in enumerate(lst):
                if other is kf:
                    del lst[k]
                    break

    def clear(self):                                     # :68-72
        self.inverted = [[] for _ in range(self.n_words)]

    def clear_map(self, map_id):                         # :74-98
        for lst in self.inverted:
            k = 0
            while k < len(lst):
                if lst[k].map == map_id:
                    del lst[k]
                else:
                    k += 1

    # ---- DetectRelocalizationCandidates, :814-926 -----------------------------------------------------------------------------------
    def reloc_scored(self, query_id, bow, trace=None):
        """:816-871.  Returns lScoreAndMatch [(si, kf)], maxCommonWords, minCommonWords, len(lKFsSharingWords)."""
        sharing = []
        for wid, _ in bow:
            for kf in self.inverted[wid]:
                if kf.mnRelocQuery != query_id:
                    kf.mnRelocWords = 0
                    kf.mnRelocQuery = query_id
                    sharing.append(kf)
                kf.mnRelocWords += 1
        if trace is not None:
            trace["sharing"] = []
        if not sharing:
            return [], 0, 0, 0
        max_common = 0
        for kf in sharing:
            if kf.mnRelocWords > max_common:
                max_common = kf.mnRelocWords
        min_common = int(F32(max_common) * F32(0.8))
        scored = []
        for kf in sharing:
            if kf.mnRelocWords > min_common:
                st = [] if trace is not None else None
                si = F32(l1_score(bow, kf.bow, st))
                kf.mRelocScore = si
                scored.append((si, kf))
                if trace is not None:
                    trace.setdefault("pairs", {})[kf.tag] = st
        if trace is not None:
            trace["sharing"] = [(kf.tag, kf.mnRelocWords) for kf in sharing]
        return scored, max_common, min_common, len(sharing)

    def reloc_candidates(self, query_id, map_id, scored, trace=None):
        """:870-925 over lScoreAndMatch."""
        if not scored:
            return []
        acc_list = []
        best_acc = F32(0)
        for si, kf in scored:
            best = si
            acc = best
            best_kf = kf
            for kf2 in kf.best_covisibles(10):
                if kf2.mnRelocQuery != query_id:
                    if trace is not None:
                        trace.setdefault("skipped", []).append(kf2.tag)
                    continue
                acc = F32(acc + kf2.mRelocScore)
                if trace is not None:
                    trace.setdefault("added", []).append((kf.tag, kf2.tag))
                if kf2.mRelocScore > best:
                    best_kf = kf2
                    best = kf2.mRelocScore
            acc_list.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        min_retain = F32(F32(0.75) * best_acc)
        already = set()
        out = []
        for si, kf in acc_list:
            if si > min_retain:
                if kf.map != map_id:
                    continue
                if kf.tag not in already:
                    out.append(kf)
                    already.add(kf.tag)
        if trace is not None:
            trace["acc"] = [(a, k.tag) for a, k in acc_list]
            trace["min_retain"] = min_retain
        return out

    # ---- DetectNBestCandidates, :620-811 --------------------------------------------------------------------------------------------
    def place_scored(self, query_id, connected, bow, trace=None):
        """:627-711; connected: the KF objects of GetConnectedKeyFrames()."""
        sharing = []
        con = set(id(k) for k in connected)
        for wid, _ in bow:
            for kf in self.inverted[wid]:
                if kf.mnPlaceRecognitionQuery != query_id:
                    kf.mnPlaceRecognitionWords = 0
                    if id(kf) not in con:
                        kf.mnPlaceRecognitionQuery = query_id
                        sharing.append(kf)
                kf.mnPlaceRecognitionWords += 1
        if trace is not None:
            trace["sharing"] = []
        if not sharing:
            return [], 0, 0, 0
        max_common = 0
        for kf in sharing:
            if kf.mnPlaceRecognitionWords > max_common:
                max_common = kf.mnPlaceRecognitionWords
        min_common = int(F32(max_common) * F32(0.8))
        scored = []
        for kf in sharing:
            if kf.mnPlaceRecognitionWords > min_common:
                si = F32(l1_score(bow, kf.bow))
                kf.mPlaceRecognitionScore = si
                scored.append((si, kf))
        if trace is not None:
            trace["sharing"] = [(kf.tag, kf.mnPlaceRecognitionWords) for kf in sharing]
        return scored, max_common, min_common, len(sharing)

    def place_sorted(self, query_id, scored, trace=None):
        """:710-748 over lScoreAndMatch: lAccScoreAndMatch after list::sort(compFirst)."""
        if not scored:
            return []
        acc_list = []
        for si, kf in scored:
            best = si
            acc = best
            best_kf = kf
            for kf2 in kf.best_covisibles(10):
                if kf2.mnPlaceRecognitionQuery != query_id:
                    continue
                acc = F32(acc + kf2.mPlaceRecognitionScore)
                if kf2.mPlaceRecognitionScore > best:
                    best_kf = kf2
                    best = kf2.mPlaceRecognitionScore
            acc_list.append((acc, best_kf))
        if trace is not None:
            trace["acc_unsorted"] = [(a, k.tag) for a, k in acc_list]
        # list::sort is a stable merge sort; compFirst is a.first > b.first.  An insertion sort that moves an element left only past
        # strictly smaller ones is stable too and, unlike sorted(), says so in its own lines.
        out = []
        for item in acc_list:
            k = len(out)
            while k > 0 and item[0] > out[k - 1][0]:
                k -= 1
            out.insert(k, item)
        return out

    @staticmethod
    def place_take(sorted_acc, n_candidates, query_map, map_is_bad=lambda m: False):
        """:750-783, skipping a bad keyframe instead of spinning on it (:764-765)."""
        loop, merge, already = [], [], set()
        for _, kf in sorted_acc:
            if not (len(loop) < n_candidates or len(merge) < n_candidates):
                break
            if kf.bad:
                continue
            if kf.tag not in already:
                if query_map == kf.map and len(loop) < n_candidates:
                    loop.append(kf)
                elif query_map != kf.map and len(merge) < n_candidates and not map_is_bad(kf.map):
                    merge.append(kf)
                already.add(kf.tag)
        return loop, merge
