"""Seeded scenes for the keyframe database (orbd_* of include/orbhip.h): each scene is a script of add / erase / clear_map / set_map /
query steps over a synthetic vocabulary size (the database needs no vocabulary tree), and replay() runs a script on the literal model
of tests/kfdb_model.py and on a handle side by side, comparing every query result - doubles and floats by bit pattern, lists by order -
and, after every query, the four members of every live keyframe.

Steps:
  ("add", tag, map, (ids, vals), [covisible tags], init or None)   a tag that was erased may be added again: a new keyframe object
  ("erase", tag) ("clear_map", map) ("clear",) ("set_map", tag, map) ("bad", tag)
  ("reloc", query_id, (ids, vals), map)
  ("place", query_id, [connected tags], (ids, vals), query_map, n_candidates)
Covisibles are tags; an erased keyframe leaves every covisible list (as KeyFrame::SetBadFlag erases its connections)."""
import numpy as np

import kfdb_model as KM

N_WORDS = 4096
T = 1 << 40      # tags are not slot numbers


def bow(ids, vals):
    return (np.asarray(ids, np.uint32), np.asarray(vals, np.float64))


def rand_bow(rng, n, lo, hi, n_words=N_WORDS):
    """n distinct words of [lo, hi), ascending, with L1-normalised positive values (what the transform leaves)."""
    hi = min(hi, n_words)
    n = min(n, hi - lo)
    ids = np.sort(rng.choice(np.arange(lo, hi), size=n, replace=False)).astype(np.uint32)
    v = rng.random(n) + 0.05
    return ids, (v / v.sum()).astype(np.float64)


def flat(ids, v):
    return bow(list(ids), [v] * len(list(ids)))


def scene_order():
    q = flat([5, 10, 20, 30], 0.25)
    return [
        ("add", T + 1, 1, flat([10, 20], 0.5), [], None),
        ("add", T + 2, 1, flat([10, 30], 0.5), [], None),
        ("add", T + 3, 1, flat([5, 30], 0.5), [], None),      # added last, met first (word 5)
        ("reloc", 1, q, 1),
        ("erase", T + 1),
        ("add", T + 1, 1, flat([10, 20], 0.5), [], None),     # again: the end of the lists of words 10 and 20
        ("reloc", 2, q, 1),
    ]


def scene_gate():
    s = []
    w = list(range(100, 107))
    s.append(("add", T + 1, 1, flat(w[:5] + [900], 0.1), [], None))         # 5 of the first query
    s.append(("add", T + 2, 1, flat(w[:4] + [901], 0.1), [], None))         # 4 = minCommonWords of a maximum of 5: rejected
    s.append(("add", T + 3, 1, flat(w[:3] + [902], 0.1), [], None))
    s.append(("reloc", 1, flat(w[:5], 0.2), 1))
    s.append(("add", T + 4, 1, flat(w, 0.1), [], None))                     # 7 of the second query: 7 * 0.8f = 5.6 -> 5
    s.append(("add", T + 5, 1, flat(w[:6], 0.1), [], None))                 # 6 passes
    s.append(("reloc", 2, flat(w, 0.125), 1))                               # T+1 has 5 = minCommonWords: rejected
    return s


def scene_score():
    rng = np.random.default_rng(11)
    s = []
    for i in range(6):
        s.append(("add", T + i, 1, rand_bow(rng, 60, 0, 90), [], None))
    s.append(("reloc", 1, rand_bow(rng, 70, 0, 90), 1))
    s.append(("place", 2, [], rand_bow(rng, 70, 0, 90), 1, 3))
    return s


def scene_neighbours():
    q1 = flat(range(200, 210), 0.1)
    q2 = flat(range(100, 120), 0.05)
    S1, S2, N, M = T + 1, T + 2, T + 3, T + 4
    return [
        ("add", S1, 1, flat(range(100, 118), 0.02), [N, M, S2], None),             # 18 of q2: passes; low score
        ("add", S2, 1, flat(range(100, 120), 0.05), [S1], None),                   # all of q2, equal values: high score
        ("add", N, 1, flat(list(range(100, 103)) + list(range(200, 210)), 0.01), [], None),   # scored by q1; 3 of q2: listed, gated out
        ("add", M, 1, flat(range(300, 310), 0.1), [], None),                       # shares nothing with q2: not listed
        ("reloc", 11, q1, 1),
        ("reloc", 12, q2, 1),
    ]


def scene_maps():
    q = flat(range(100, 120), 0.05)
    return [
        ("add", T + 1, 2, flat(range(100, 120), 0.05), [], None),     # the other map: score 1.0, sets the threshold 0.75
        ("add", T + 2, 1, flat(range(100, 120), 0.045), [], None),    # 0.9: kept
        ("add", T + 3, 1, flat(range(100, 117), 0.04), [], None),     # 0.68: below 0.75, above 0.75 * 0.9
        ("reloc", 1, q, 1),
        ("set_map", T + 1, 1),                                         # a merge moves the keyframe
        ("reloc", 2, q, 1),
        ("clear_map", 1),
        ("reloc", 3, q, 1),
    ]


def scene_place():
    q = flat(range(100, 120), 0.05)
    K1, K2, H, G, Cn, B, X = T + 1, T + 2, T + 3, T + 4, T + 5, T + 6, (1 << 63) + 9
    return [
        ("add", K1, 1, flat(range(100, 120), 0.05), [Cn], None),      # Cn is connected to the query: never marked, so skipped here
        ("add", K2, 1, flat(range(100, 120), 0.05), [], None),        # the same accumulated score as K1: list order stays
        ("add", Cn, 1, flat(range(100, 120), 0.05), [], None),
        ("add", H, 1, flat(range(100, 120), 0.045), [G], None),       # listed after K1, K2; 0.9 + 0.9 sorts it first
        ("add", G, 1, flat(range(100, 120), 0.045), [], None),
        ("add", B, 1, flat(range(100, 120), 0.0475), [], None),
        ("add", X, 2, flat(range(100, 120), 0.046), [], None),        # the other map: a merge candidate
        ("bad", B),
        ("place", 77, [Cn], q, 1, 3),
        ("place", 78, [Cn, K2], q, 1, 1),
    ]


def scene_query_id():
    q = flat(range(100, 110), 0.1)
    return [
        ("add", T + 1, 1, flat(range(100, 110), 0.1), [], None),
        ("add", T + 2, 1, flat(range(105, 115), 0.1), [T + 1], None),
        ("reloc", 0, q, 1),                                            # fresh entries hold query id 0: nothing is listed
        ("place", 0, [], q, 1, 3),
        ("reloc", 5, q, 1),
        ("add", T + 3, 1, flat(range(100, 110), 0.09), [T + 1], None),
        ("reloc", 5, flat(range(100, 112), 0.08), 1),                  # the same id again: only the new keyframe is listed
        ("add", T + 4, 1, flat(range(100, 110), 0.1), [T + 1],
         dict(reloc_query=9, reloc_score=0.25, place_query=9, place_score=0.5)),      # PostLoad: members given
        ("reloc", 9, q, 1),
        ("place", 9, [], q, 1, 3),
    ]


def scene_empty():
    q = flat(range(100, 110), 0.1)
    e = bow([], [])
    return [
        ("reloc", 1, q, 1),                                            # an empty database
        ("place", 2, [], q, 1, 3),
        ("add", T + 1, 1, flat(range(100, 110), 0.1), [], None),
        ("add", T + 2, 1, e, [], None),                                # a keyframe without words
        ("reloc", 3, e, 1),                                            # an empty query
        ("place", 4, [], e, 1, 3),
        ("reloc", 5, flat(range(500, 510), 0.1), 1),                   # no shared word
        ("erase", T + 1),
        ("erase", T + 2),
        ("reloc", 6, q, 1),                                            # everything erased
        ("add", T + 1, 1, flat(range(100, 110), 0.1), [], None),
        ("clear",),
        ("reloc", 7, q, 1),
        ("add", T + 1, 1, flat(range(100, 110), 0.1), [], None),
        ("reloc", 8, q, 1),
    ]


def scene_random(seed, n_kf=40, n_steps=60, n_words=N_WORDS, span=160, lo=0, tag0=T + 100, qid0=0, clear_maps=True):
    """Random add / erase / re-add / clear_map / set_map / query steps over a narrow word range, so that lists are long."""
    rng = np.random.default_rng(seed)
    s, live, dead, qid = [], [], [], qid0
    tags = [tag0 + i for i in range(n_kf)]

    def add(t):
        cov = [int(x) for x in rng.choice(tags, size=int(rng.integers(0, min(12, len(tags)))), replace=False) if x != t]
        s.append(("add", t, int(rng.integers(1, 3)), rand_bow(rng, int(rng.integers(1, 70)), lo, lo + span, n_words), cov, None))
        live.append(t)

    for t in tags[:n_kf // 2]:
        add(t)
    fresh = tags[n_kf // 2:]
    for _ in range(n_steps):
        r = rng.random()
        if r < 0.2 and (fresh or dead):
            add(fresh.pop() if fresh and rng.random() < 0.6 or not dead else dead.pop(int(rng.integers(len(dead)))))
        elif r < 0.35 and live:
            t = live.pop(int(rng.integers(len(live))))
            dead.append(t)
            s.append(("erase", t))
        elif r < 0.38 and live:
            s.append(("set_map", live[int(rng.integers(len(live)))], int(rng.integers(1, 3))))
        elif r < 0.40 and clear_maps:
            s.append(("clear_map", "?"))          # resolved by replay: the map is read from the live objects
        else:
            qid += 1
            use = qid if rng.random() < 0.85 else max(qid - 1, qid0 + 1)     # sometimes the previous id again
            q = rand_bow(rng, int(rng.integers(1, 90)), lo, lo + span, n_words)
            if rng.random() < 0.5:
                s.append(("reloc", use, q, int(rng.integers(1, 3))))
            else:
                con = [int(x) for x in rng.choice(live, size=min(len(live), int(rng.integers(0, 5))), replace=False)] if live else []
                s.append(("place", use, con, q, int(rng.integers(1, 3)), 3))
    return s


SCENES = {
    "order": scene_order, "gate": scene_gate, "score": scene_score, "neighbours": scene_neighbours, "maps": scene_maps,
    "place": scene_place, "query_id": scene_query_id, "empty": scene_empty,
    "random1": lambda: scene_random(1), "random2": lambda: scene_random(2), "random3": lambda: scene_random(3, n_kf=24, n_steps=80, span=60),
}
NAMES = sorted(SCENES)


def bits(a, dtype):
    return np.asarray(a, dtype).view(np.uint32 if dtype == np.float32 else np.uint64).tolist()


class Replay:
    """Runs a script on the model and, when given, on a handle; compares at every query.  traces: one dict per query step (model only)."""

    def __init__(self, n_words=N_WORDS, db=None, host=True, shared=False, before_reloc=None):
        self.model = KM.Database(n_words)
        self.db, self.host = db, host
        self.shared = shared                # other threads use the handle too: its size is not this script's
        self.before_reloc = before_reloc    # called with (query_id, bow) before a reloc step; returns a check to run on the model's result
        self.kf = {}          # tag -> the live model object
        self.seq = {}         # tag -> add sequence number of the live object
        self.n_added = 0
        self.traces = []
        self.cov_tags = {}    # tag -> covisible tags as given

    def _resolve(self):
        self.stale = True           # the covisible objects are looked up when a query needs them

    def _resolve_now(self):
        if not getattr(self, "stale", False):
            return
        self.stale = False
        for t, k in self.kf.items():
            k.covisibles = [self.kf[c] for c in self.cov_tags[t] if c in self.kf]

    def covisibles_of(self, tag):
        return [k.tag for k in self.kf[tag].covisibles]

    def _check_members(self, what):
        if self.db is None:
            return
        assert self.shared or len(self.db) == len(self.kf), what
        for t, k in self.kf.items():
            m = self.db.members(t)
            got = (m["reloc_query"], m["place_query"], bits([m["reloc_score"]], np.float32), bits([m["place_score"]], np.float32))
            want = (k.mnRelocQuery, k.mnPlaceRecognitionQuery, bits([k.mRelocScore], np.float32), bits([k.mPlaceRecognitionScore], np.float32))
            assert got == want, "%s: members of %d: %r != %r" % (what, t, got, want)

    def _same_scored(self, got, scored, mx, mn, nl, what):
        assert [int(t) for t in got["tags"]] == [k.tag for _, k in scored], "%s: the scored list's order" % what
        assert bits(got["scores"], np.float32) == bits([s for s, _ in scored], np.float32), "%s: scores" % what
        assert (got["max_common"], got["min_common"], got["n_listed"]) == (mx, mn, nl), "%s: counts" % what

    def step(self, st, what=""):
        op = st[0]
        # a random script does not track what clear_map took: steps on a keyframe that is gone (or still there) are dropped
        if (op in ("erase", "set_map", "bad") and st[1] not in self.kf) or (op == "add" and st[1] in self.kf):
            return
        if op in ("reloc", "place"):
            self._resolve_now()
        if op == "place":
            st = st[:2] + ([c for c in st[2] if c in self.kf],) + st[3:]
        if op == "add":
            _, tag, map_id, b, cov, init = st
            k = KM.KF(tag, map_id, b)
            if init:
                k.mnRelocQuery, k.mRelocScore = init["reloc_query"], KM.F32(init["reloc_score"])
                k.mnPlaceRecognitionQuery, k.mPlaceRecognitionScore = init["place_query"], KM.F32(init["place_score"])
            self.kf[tag] = k
            self.cov_tags[tag] = list(cov)
            self.seq[tag] = self.n_added
            self.n_added += 1
            self.model.add(k)
            self._resolve()
            if self.db is not None:
                self.db.add(tag, map_id, b, init)
        elif op == "erase":
            k = self.kf.pop(st[1])
            self.model.erase(k)
            self._resolve()
            if self.db is not None:
                self.db.erase(st[1])
        elif op == "clear":
            self.model.clear()
            self.kf.clear()
            if self.db is not None:
                self.db.clear()
        elif op == "clear_map":
            m = st[1]
            if m == "?":
                m = sorted(self.kf.values(), key=lambda k: k.tag)[0].map if self.kf else 1
            self.model.clear_map(m)
            self.kf = {t: k for t, k in self.kf.items() if k.map != m}
            self._resolve()
            if self.db is not None:
                self.db.clear_map(m)
        elif op == "set_map":
            self.kf[st[1]].map = st[2]
            if self.db is not None:
                self.db.set_map(st[1], st[2])
        elif op == "bad":
            self.kf[st[1]].bad = True
        elif op == "reloc":
            _, qid, b, map_id = st
            tr = dict(op="reloc", query=b, seq=dict(self.seq), bows={t: k.bow for t, k in self.kf.items()})
            mb = [(int(i), float(v)) for i, v in zip(*b)]
            after = self.before_reloc(qid, b) if self.before_reloc else None
            scored, mx, mn, nl = self.model.reloc_scored(qid, mb, tr)
            if after:
                after(scored, mx, mn, nl, what)
            tr.update(scored=[(s, k.tag) for s, k in scored], max_common=mx, min_common=mn)
            if self.db is not None:
                got = (self.db.query_reloc_host if self.host else self.db.query_reloc)(qid, b)
                self._same_scored(got, scored, mx, mn, nl, what)
                cands = self.db.accumulate_reloc(qid, map_id, got, self.covisibles_of) if len(got["tags"]) else []
            want = self.model.reloc_candidates(qid, map_id, scored, tr)
            tr["candidates"] = [k.tag for k in want]
            if self.db is not None:
                assert cands == tr["candidates"], "%s: vpRelocCandidates" % what
            self.traces.append(tr)
            self._check_members(what)
        elif op == "place":
            _, qid, con, b, qmap, ncand = st
            tr = dict(op="place", query=b, seq=dict(self.seq), connected=list(con), bows={t: k.bow for t, k in self.kf.items()})
            mb = [(int(i), float(v)) for i, v in zip(*b)]
            scored, mx, mn, nl = self.model.place_scored(qid, [self.kf[c] for c in con], mb, tr)
            tr.update(scored=[(s, k.tag) for s, k in scored], max_common=mx, min_common=mn)
            srt = self.model.place_sorted(qid, scored, tr)
            tr["sorted"] = [(a, k.tag) for a, k in srt]
            loop, merge = self.model.place_take(srt, ncand, qmap)
            tr["loop"], tr["merge"] = [k.tag for k in loop], [k.tag for k in merge]
            if self.db is not None:
                got = (self.db.query_place_host if self.host else self.db.query_place)(qid, con, b)
                self._same_scored(got, scored, mx, mn, nl, what)
                if len(got["tags"]):
                    acc, best = self.db.accumulate_place(qid, got, self.covisibles_of)
                    assert best == [k.tag for _, k in srt] and bits(acc, np.float32) == bits([a for a, _ in srt], np.float32), \
                        "%s: lAccScoreAndMatch" % what
                    l2, m2 = self.db.take_n_best((acc, best), ncand, qmap, lambda t: self.kf[t].map, lambda t: self.kf[t].bad)
                    assert (l2, m2) == (tr["loop"], tr["merge"]), "%s: vpLoopCand / vpMergeCand" % what
                else:
                    assert not srt
            self.traces.append(tr)
            self._check_members(what)
        else:
            raise ValueError(op)

    def run(self, script, name=""):
        for i, st in enumerate(script):
            self.step(st, "%s step %d (%s)" % (name, i, st[0]))
        return self.traces
