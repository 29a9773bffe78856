"""Seeded scenes for LocalMapping::KeyFrameCulling (orbm_culling_t as a dict of numpy arrays, plus `erasable` or None): hand-made ones
that each hold one property of the loop, and random local maps of K = 1, 2, 8 and 101 keyframes.  tests/test_keyframe_culling_abi.py
asserts the properties on the model alone; the device tests compare every scene with the model."""
import numpy as np

OUT = -1          # an observer that is not in the list
FAR = 7           # a level that never qualifies against the rows' levels (0 .. 3)


class Builder:
    def __init__(self, K, mono=False, redundant_th=0.9, th_depth=40.0):
        self.K, self.mono, self.th = K, mono, redundant_th
        self.rows = [[] for _ in range(K)]            # (point, level, depth)
        self.points = []                              # dict(entries=[(kf, level, w)], n_obs, bad)
        self.skip, self.th_depth, self.erasable = np.zeros(K, np.uint8), np.full(K, th_depth, np.float32), None
        self.named = {}

    def point(self, entries, n_obs=None, bad=0, name=None):
        self.points.append(dict(entries=list(entries), n_obs=sum(w for _, _, w in entries) if n_obs is None else n_obs, bad=bad))
        if name:
            self.named[name] = len(self.points) - 1
        return len(self.points) - 1

    def row(self, k, p, level=0, depth=1.0):
        self.rows[k].append((p, level, depth))
        return len(self.rows[k]) - 1

    def redundant_point(self, k, level=0):
        """A point that keyframe k sees and four outside observers see at the same level: redundant for k whatever else is erased."""
        p = self.point([(k, level, 1)] + [(OUT, level, 1)] * 4)
        self.row(k, p, level)
        return p

    def plain_point(self, k, level=0):
        """Seen by k and three outside observers: it counts in nMPs, is never redundant and never turns bad."""
        p = self.point([(k, level, 1)] + [(OUT, level, 1)] * 3)
        self.row(k, p, level)
        return p

    def flat(self):
        row_start = np.cumsum([0] + [len(r) for r in self.rows]).astype(np.int32)
        allrows = [r for rows in self.rows for r in rows]
        obs_start = np.cumsum([0] + [len(p["entries"]) for p in self.points]).astype(np.int32)
        ent = [e for p in self.points for e in p["entries"]]
        col = lambda items, j, t: np.array([it[j] for it in items], t).reshape(-1)
        return dict(skip=self.skip.copy(), th_depth=self.th_depth.copy(), row_start=row_start, row_point=col(allrows, 0, np.int32),
                    row_level=col(allrows, 1, np.int32), row_depth=None if self.mono else col(allrows, 2, np.float32),
                    bad=np.array([p["bad"] for p in self.points], np.uint8).reshape(-1),
                    n_obs=np.array([p["n_obs"] for p in self.points], np.int32).reshape(-1), obs_start=obs_start,
                    obs_kf=col(ent, 0, np.int32), obs_level=col(ent, 1, np.int32), obs_w=col(ent, 2, np.uint8),
                    mono=int(self.mono), redundant_th=np.float32(self.th), erasable=self.erasable, named=dict(self.named))


def culled_to_kept():
    """Keyframe 0 passes and is erased.  Keyframe 1's ten points are redundant at loop entry only through keyframe 0's entry (one of
    exactly four hits): after the erase it has nRed = 0 and is kept."""
    B = Builder(2)
    for _ in range(10):
        B.redundant_point(0)
    for _ in range(10):
        p = B.point([(1, 0, 1), (0, 0, 1)] + [(OUT, 0, 1)] * 3)
        B.row(0, p)
        B.row(1, p)
    return B.flat()


def kept_to_culled():
    """Keyframe 0 passes (100 redundant of 110) and is erased; its ten other points go from three observations to two and turn bad.
    Keyframe 1 has 10 redundant of 20 at loop entry (kept); the ten bad points leave nMPs = 10: 10 > 0.9f * 10, culled."""
    B = Builder(2)
    for _ in range(100):
        B.redundant_point(0)
    for j in range(10):
        p = B.point([(0, 0, 1), (1, 0, 1), (OUT, 0, 1)], name="to_two_%d" % j)
        B.row(0, p)
        B.row(1, p)
    for _ in range(10):
        B.redundant_point(1)
    return B.flat()


def float_product():
    """nMPs = 10, nRed = 9 at 0.9f: 9 > 0.9f * 10.f is false (the product rounds to 9), 9 > (double)0.9f * 10 is true."""
    B = Builder(1)
    for _ in range(9):
        B.redundant_point(0)
    B.plain_point(0)
    return B.flat()


def erase_cases():
    """Keyframe 0 (80 redundant points) is erased; its further rows hold the points that the erase has to treat one by one.  Keyframe 1
    sees them all afterwards; keyframe 2 is skipped although it would pass; keyframe 3 passes but is not erasable, so keyframe 4, which
    leans on keyframe 3's entries, stays redundant and is culled; keyframe 5 has no rows."""
    B = Builder(6)
    for _ in range(80):
        B.redundant_point(0)
    twice = B.point([(0, 0, 1)] + [(OUT, 0, 1)] * 3, name="two_rows")            # n_obs 4, held by two rows of keyframe 0: stays at 3
    B.row(0, twice), B.row(0, -1), B.row(0, twice)
    special = [twice,
               B.point([(0, 0, 1), (OUT, 0, 1), (OUT, 0, 1)], name="to_two"),                  # 3 -> 2: bad
               B.point([(0, 0, 2), (OUT, 0, 1), (OUT, 0, 1)], name="w2_to_two"),               # 4 -> 2 by a weight-2 entry: bad
               B.point([(0, 0, 2)] + [(OUT, 0, 1)] * 3, name="w2_to_three"),                   # 5 -> 3: stays
               B.point([(0, 0, 1)] + [(OUT, 0, 2)] * 2 + [(OUT, 0, 1)] * 2, name="w2_others"),   # 7 -> 6, four hits left
               B.point([(OUT, 0, 1)] * 5, name="no_entry_of_0"),                               # a row of 0 without an entry of 0
               B.point([(0, 0, 1)] + [(OUT, 0, 1)] * 5, bad=1, name="bad_on_entry")]
    for p in special[1:]:
        B.row(0, p)
    for p in special:
        B.row(1, p)
    for _ in range(3):
        B.plain_point(1)
    for _ in range(12):
        B.redundant_point(2)
    B.skip[2] = 1
    for _ in range(10):
        B.redundant_point(3)
    for _ in range(10):
        p = B.point([(4, 0, 1), (3, 0, 1)] + [(OUT, 0, 1)] * 3)
        B.row(3, p), B.row(4, p)
    B.erasable = np.ones(6, np.uint8)
    B.erasable[3] = 0
    return B.flat()


ENTRY_COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 129)
FOURTH_AT = (3, 63, 64, 128)


def list_cases():
    """One keyframe whose rows hold points with 0 .. 129 entries: the fourth qualifying entry at positions 3, 63, 64 and 128 (redundant)
    and the same lists with three qualifying entries (not redundant); levels at row_level + 1 (a hit) and + 2 (none); the keyframe's own
    entry as one of four qualifying ones (three hits); depth exactly at th_depth, above it and negative; n_obs of 3 with a full list."""
    B = Builder(2, th_depth=35.0)
    k, lv = 0, 2
    for n in ENTRY_COUNTS:
        p = B.point([(OUT, FAR, 1)] * n, n_obs=max(n, 5), name="n%d_none" % n)
        B.row(k, p, lv)
        if n >= 4:
            p = B.point([(OUT, lv, 1)] * n, n_obs=n, name="n%d_all" % n)
            B.row(k, p, lv)
    for at in FOURTH_AT:
        n = at + 1
        for hits, tag in ((4, "hit"), (3, "miss")):
            ent = [(OUT, FAR, 1)] * n
            for j in ([0, 1, 2] + [at])[4 - hits:]:
                ent[j] = (OUT, lv, 1)
            B.row(k, B.point(ent, n_obs=n, name="fourth_at_%d_%s" % (at, tag)), lv)
        ent = [(OUT, FAR, 1)] * 129                      # behind `at` further hits: the early stop changes nothing
        for j in (0, 1, 2, at, 128):
            ent[j] = (OUT, lv, 1)
        B.row(k, B.point(ent, n_obs=129, name="fourth_at_%d_long" % at), lv)
    B.row(k, B.point([(k, lv, 1)] + [(OUT, lv + 1, 1)] * 4, name="level_plus_1"), lv)
    B.row(k, B.point([(k, lv, 1)] + [(OUT, lv + 1, 1)] * 3 + [(OUT, lv + 2, 1)], name="level_plus_2"), lv)
    B.row(k, B.point([(OUT, lv, 1)] * 3 + [(k, lv, 1)], name="own_is_fourth"), lv)
    B.row(k, B.point([(OUT, lv, 1)] * 3 + [(k, lv, 1), (1, lv, 1)], name="own_and_four"), lv)
    B.row(k, B.point([(OUT, lv, 1)] * 6, n_obs=3, name="n_obs_3"), lv)
    for name, depth in (("at_th_depth", 35.0), ("above_th_depth", np.nextafter(np.float32(35.0), np.float32(99.0))), ("negative_depth", -0.5),
                        ("zero_depth", 0.0)):
        B.row(k, B.point([(k, lv, 1)] + [(OUT, lv, 1)] * 4, name=name), lv, depth)
    B.row(k, -1, lv)
    for _ in range(6):
        B.redundant_point(1)
    return B.flat()


def mono_scene():
    """mono != 0 with row_depth = None: depths are not read."""
    B = Builder(3, mono=True)
    for _ in range(12):
        B.redundant_point(0)
    for _ in range(8):
        p = B.point([(1, 0, 1), (0, 0, 1)] + [(OUT, 0, 1)] * 3)
        B.row(0, p), B.row(1, p)
    for _ in range(9):
        B.redundant_point(2)
    B.plain_point(2)
    return B.flat()


def random_map(seed, K, P, views=7, window=12, outside=2, empty_rows=0.3, skip_first=True, redundant_th=0.9, wide=None):
    """A local map: every point is seen by about `views` keyframes of a window of the list and by up to `outside` observers outside it;
    a keyframe's rows are its points in random order between rows without a point.  About a fifth of the observations are stereo
    (weight 2), some points are bad, some depths lie beyond th_depth.  wide = (k, rows): keyframe k gets rows up to that number."""
    rng = np.random.RandomState(seed)
    B = Builder(K, redundant_th=redundant_th)
    per_kf = [[] for _ in range(K)]
    for p in range(P):
        c = rng.randint(0, K)
        cand = np.arange(max(0, c - window // 2), min(K, c + window // 2 + 1))
        if wide is not None and p < wide[1] * 6 // 10 and wide[0] not in cand:
            cand = np.append(cand, wide[0])
        kfs = rng.choice(cand, size=min(len(cand), max(1, views + rng.randint(-3, 4))), replace=False)
        if wide is not None and p < wide[1] * 6 // 10 and wide[0] not in kfs:
            kfs = np.append(kfs, wide[0])
        base = rng.randint(0, 3)
        ent = [(int(k), int(base + rng.randint(0, 3)), 2 if rng.rand() < 0.2 else 1) for k in kfs]
        ent += [(OUT, int(base + rng.randint(0, 3)), 1) for _ in range(rng.randint(0, outside + 1))]
        order = rng.permutation(len(ent))
        idx = B.point([ent[j] for j in order], bad=int(rng.rand() < 0.03))
        for k, level, _ in ent:
            if k >= 0:
                per_kf[k].append((idx, level))
    for k in range(K):
        rows = [(p, lv, float(rng.choice([1.0, 5.0, 39.0, 40.0, 41.0, 80.0, -1.0], p=[.3, .3, .2, .1, .04, .03, .03]))) for p, lv in per_kf[k]]
        rows += [(-1, int(rng.randint(0, 4)), 1.0)] * int(len(rows) * empty_rows)
        if wide is not None and k == wide[0]:
            rows += [(-1, 0, 1.0)] * max(0, wide[1] - len(rows))
            rows = rows[:wide[1]]
        B.rows[k] = [rows[j] for j in rng.permutation(len(rows))]
    if skip_first and K > 1:
        B.skip[0] = 1                                  # GetInitKFid()
    if K > 4:
        B.skip[K // 2] = 1                             # isBad()
        B.erasable = (rng.rand(K) > 0.1).astype(np.uint8)
    return B.flat()


_scenes = {}


def scenes():
    """name -> scene, built once and left unchanged."""
    if not _scenes:
        _scenes.update(culled_to_kept=culled_to_kept(), kept_to_culled=kept_to_culled(), float_product=float_product(),
                       erase_cases=erase_cases(), list_cases=list_cases(), mono=mono_scene(),
                       k1=random_map(11, 1, 60, outside=7, skip_first=False, redundant_th=0.3),
                       k2=random_map(12, 2, 150, views=2, outside=6, skip_first=False, redundant_th=0.3),
                       k8=random_map(13, 8, 500, views=6, outside=3, redundant_th=0.5), k101=random_map(14, 101, 3000, views=9, window=14),
                       wide=random_map(15, 3, 12000, views=3, outside=5, skip_first=False, redundant_th=0.5, wide=(1, 15360)))
    return _scenes


def arrays(scene):
    """The scene without what is not part of orbm_culling_t."""
    return {k: v for k, v in scene.items() if k not in ("erasable", "named")}
