"""One seeded scene of map points for orbm_update_map_points (MapPoint::ComputeDistinctiveDescriptors + MapPoint::UpdateNormalAndDepth for all
map points of a keyframe, LocalMapping.cc:1040-1053).

A point is a dict of `desc` [n, 32] uint8, `centre` [n, 3] float32, `in_desc` [n] uint8 - one row per (keyframe, camera) entry in the
reference's walk order - and `pos` [3], `ref_centre` [3], `ref_scale`, `ref_max_scale` (the layout of pkg.pack_map_points).  The entries'
descriptors are a per-point base row with a per-entry share of flipped bits, so that the medians differ between rows; the camera centres
lie 1-6 m from the point.  NAMED gives the index of every hand-made point:
  n0 .. n1024      entry counts 0, 1, 2, 3, 63, 64, 65, 129 and 1024 (the kernel's register form ends at 64, its tiles at multiples of 64)
  none_flagged     every in_desc 0: best -1, the normal still computed
  behind_unflagged entry 0 is the cleanest row but unflagged, so the choice among ALL rows would be 0 and the kept row lies behind it
  long_partial     a 200-entry group with a third of the rows unflagged (the tiled form's flags)
  twins            rows 2 and 5 are the same clean row among noisy ones: both have the least median, the first wins
  all_equal        six equal rows: best 0
  rig              a keyframe's two cameras as two adjacent entries, centres 0.11 m apart
  in_centre        pos equals the centre of entry 1 exactly: 1/0, 0*inf, NaN in all three components
  tiny_tie         98 entries in the plane z = 0 around a point in the origin, one of them 147 * 2^-149 below it at distance 1: the z sum
                   is that subnormal, and its mean 1.5 * 2^-149 is a tie, which (float)((double)v * (1.0 / 98)) rounds down (the double
                   reciprocal is below 1/98) and a float division v / 98 rounds to even, up
Everything else is random: 3-12 entries, 10 % of the entries unflagged, 10 % rig pairs."""
import numpy as np

SEED = 20240611
N_RANDOM = 280
SIZES = (0, 1, 2, 3, 63, 64, 65, 129, 1024)
SCALES = np.array([np.float32(1.2) ** k for k in range(8)], np.float32)   # mvScaleFactors of an 8-level, 1.2 pyramid (float powers)
NAMED = {}
_scene = None


def _rows(rng, n, noise):
    """n rows around one base row; row e has each bit flipped with probability noise[e]."""
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    flips = np.packbits(rng.random((n, 256)) < np.asarray(noise, np.float64).reshape(n, 1), axis=1)
    return (base[None, :] ^ flips).astype(np.uint8)


def _point(rng, n, unflag=0.1, noise=None):
    pos = rng.uniform(-5, 5, 3).astype(np.float32)
    dirs = rng.normal(size=(n, 3))
    dirs /= np.maximum(np.linalg.norm(dirs, axis=1, keepdims=True), 1e-9)
    centre = (pos.astype(np.float64) - dirs * rng.uniform(1, 6, (n, 1))).astype(np.float32)
    e = 0
    while e + 1 < n:                                               # rig pairs: the second camera of the same keyframe
        if rng.random() < 0.1:
            centre[e + 1] = centre[e] + rng.normal(size=3).astype(np.float32) * np.float32(0.06)
            e += 2
        else:
            e += 1
    ref = int(rng.integers(0, n)) if n else 0
    ref_centre = centre[ref].copy() if n else rng.uniform(-5, 5, 3).astype(np.float32)
    return dict(desc=_rows(rng, n, rng.uniform(0.01, 0.2, n) if noise is None else noise), centre=centre,
                in_desc=(rng.random(n) >= unflag).astype(np.uint8), pos=pos, ref_centre=ref_centre,
                ref_scale=SCALES[int(rng.integers(0, 8))], ref_max_scale=SCALES[7])


def scene():
    """The list of points, built once and never changed by a test."""
    global _scene
    if _scene is not None:
        return _scene
    rng = np.random.default_rng(SEED)
    pts = []

    def add(name, pt):
        NAMED[name] = len(pts)
        pts.append(pt)

    for n in SIZES:
        add("n%d" % n, _point(rng, n))
    pt = _point(rng, 7)
    pt["in_desc"][:] = 0
    add("none_flagged", pt)
    pt = _point(rng, 6, noise=[0.0, 0.15, 0.03, 0.15, 0.15, 0.15])
    pt["in_desc"][:] = 1
    pt["in_desc"][0] = 0
    add("behind_unflagged", pt)
    pt = _point(rng, 200, unflag=0.33)
    pt["in_desc"][0] = 0
    add("long_partial", pt)
    pt = _point(rng, 8, noise=[0.2, 0.2, 0.0, 0.2, 0.2, 0.0, 0.2, 0.2])
    pt["in_desc"][:] = 1
    add("twins", pt)
    pt = _point(rng, 6, noise=[0.0] * 6)
    pt["in_desc"][:] = 1
    add("all_equal", pt)
    pt = _point(rng, 4)
    pt["centre"][2] = pt["centre"][1] + np.array([0.11, 0.0, 0.0], np.float32)
    add("rig", pt)
    pt = _point(rng, 5)
    pt["centre"][1] = pt["pos"]
    add("in_centre", pt)
    pt = _point(rng, 98)
    pt["pos"][:] = 0
    pt["centre"][:, 2] = 0
    pt["centre"][40] = [-1.0, 0.0, -147 * 2.0 ** -149]
    pt["ref_centre"] = pt["centre"][3].copy()
    add("tiny_tie", pt)
    for _ in range(N_RANDOM):
        pts.append(_point(rng, int(rng.integers(3, 13))))
    order = rng.permutation(len(pts))                              # the hand-made points lie between the random ones
    where = np.argsort(order)
    for k in NAMED:
        NAMED[k] = int(where[NAMED[k]])
    _scene = [pts[i] for i in order]
    return _scene
