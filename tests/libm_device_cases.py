"""Input sets for the scalar functions the kernels restate by hand (csrc/orb_sincos.h, csrc/orb_atan2f.h, fast_atan2_deg of
csrc/orb_kernels.h): tests/test_libm_device_cases.py checks what each set holds and runs the host builds over it, and
tests/test_gpu_libm_device.py runs the device builds over it.  A helper, not a conftest: deterministic (fixed seeds), built once per
process, returned read-only.  Nothing here looks at the product; the extractor's angles come from the oracle's fastAtan2 (oracle/orb_oracle.c).

Every set is float32; the unary ones are built as bit patterns.  sincos() stays inside the replica's domain |x| < 120."""
import numpy as np

import ref_camera_cases as RC

f32, u32 = np.float32, np.uint32
SIGN = 0x80000000
INF = 0x7f800000
ULPS = 4096                                                  # half width of a window around a threshold

ATANF_BREAKPOINTS = (0x31000000, 0x3ee00000, 0x3f300000, 0x3f980000, 0x401c0000, 0x4c000000, 0x3f800000)   # tests/test_libm_replicas.py
SINCOS_TOP12 = (0x398, 0x3f4)                                # orb_sincos.h: |x| < 2^-12 returns early, top12 < top12(pi / 4) skips the reduction
ATAN2F_SPECIAL = (0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 1e-40, -1e-40, 3.4e38, -3.4e38, 1e-30, 2.5, 2.0 ** 61, -2.0 ** -61)   # tests/test_libm_replicas.py
ATAN2F_KS = (-62, -61, -60, -59, -58, 58, 59, 60, 61, 62)    # e_atan2f.c branches at k > 60 and k < -60
FAST_ATAN2_SMALL = 256                                       # every integer pair of [-256, 256]^2

_cache = {}


def _once(key, make):
    if key not in _cache:
        out = make()
        for a in (out if isinstance(out, tuple) else (out,)):
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def bits(x):
    return int(np.array([x], f32).view(u32)[0])


def _window(b, r=ULPS):
    """The magnitudes within r ulps of the magnitude b (bit patterns, sign bit clear)."""
    return np.arange(max(b - r, 0), b + r + 1, dtype=np.int64)


def _both_signs(mag):
    mag = np.asarray(mag, np.int64)
    return np.concatenate([mag, mag | SIGN])


def _floats(patterns):
    return np.concatenate([np.asarray(p, np.int64) for p in patterns]).astype(u32).view(f32)


# ---- comparing results ------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    """Elementwise: equal bit patterns (the sign of zero included), or both NaN."""
    return (a.view(u32) == b.view(u32)) | (np.isnan(a) & np.isnan(b))


def mismatch(what, inputs, got, want, names):
    """None where got equals want everywhere, else a message with the first mismatching input and both outputs as bits."""
    bad = np.flatnonzero(~same_bits(got, want))
    if len(bad) == 0:
        return None
    i = bad[0]
    arg = ", ".join("%r (0x%08x)" % (float(a[i]), a.view(u32)[i]) for a in inputs)
    return "%s: %s != %s on %d of %d inputs, first at [%d]: input %s -> %s 0x%08x, %s 0x%08x" % (
        what, names[0], names[1], len(bad), len(got), i, arg, names[0], got.view(u32)[i], names[1], want.view(u32)[i])


# ---- fast_atan2_deg ----------------------------------------------------------------------------------------------------------------------
def fast_atan2_small():
    """(y, x): every integer pair (m01, m10) of [-256, 256]^2 as floats: (0, 0), both axes, every |y| == |x| tie."""
    def make():
        v = np.arange(-FAST_ATAN2_SMALL, FAST_ATAN2_SMALL + 1, dtype=f32)
        y, x = np.meshgrid(v, v, indexing="ij")
        return y.ravel().copy(), x.ravel().copy()
    return _once("fast-small", make)


def fast_atan2():
    """(y, x) for fast_atan2_deg: moments, that is integers as floats.  fast_atan2_small(), 4 million seeded pairs up to +-2^24, and
    |y| == |x| and |y| == |x| +- 1 at magnitudes 2^20 .. 2^24 in every sign combination."""
    def make():
        rng = np.random.default_rng(20241)
        ys, xs = fast_atan2_small()
        ry, rx = rng.integers(-2 ** 24, 2 ** 24 + 1, (2, 4_000_000))
        v = np.concatenate([rng.integers(2 ** 20, 2 ** 24, 10_000), [2 ** 24 - 1, 2 ** 23, 2 ** 20]])
        ty, tx = [], []
        for d in (0, 1, -1):
            for sy in (1, -1):
                for sx in (1, -1):
                    ty.append(sy * (v + d))
                    tx.append(sx * v)
        return (np.concatenate([ys, ry.astype(f32), np.concatenate(ty).astype(f32)]),
                np.concatenate([xs, rx.astype(f32), np.concatenate(tx).astype(f32)]))
    return _once("fast", make)


# ---- cosf / sinf -------------------------------------------------------------------------------------------------------------------------
def extractor_angles():
    """The arguments ORBextractor.cc:111 passes: f32(a) * f32(CV_PI / 180) for every 4001st float a of [0, 360], 360.0f itself and the
    angles the oracle's fastAtan2 returns on fast_atan2_small()."""
    def make():
        from oracle import oracle_py as oracle
        y, x = fast_atan2_small()
        deg = np.unique(oracle.apply_binary(oracle.lib().orc_fast_atan2, y, x))
        a = np.concatenate([np.arange(0, bits(360.0) + 1, 4001, dtype=np.int64).astype(u32).view(f32), [f32(360.0)], deg]).astype(f32)
        assert a.min() >= 0 and a.max() <= 360
        return a * f32(np.pi / 180.0)
    return _once("angles", make)


def sincos():
    """x for cosf / sinf: every 251st float of [-3.2, 6.3]; +-4096 ulps around k * pi / 4, k = -4 .. 8, and around the two top12
    thresholds in both signs; +-0; denormals; extractor_angles()."""
    def make():
        pats = [np.arange(0, bits(6.3) + 1, 251, dtype=np.int64), np.arange(0, bits(3.2) + 1, 251, dtype=np.int64) | SIGN]
        for k in range(-4, 9):
            w = _window(bits(abs(k) * np.pi / 4))
            pats.append(_both_signs(w) if k == 0 else w | SIGN if k < 0 else w)
        for t in SINCOS_TOP12:
            pats.append(_both_signs(_window(t << 20)))
        pats.append(_both_signs([0]))
        pats.append(_both_signs(np.concatenate([np.arange(1, 0x800000, 4099), [0x7fffff]])))
        x = np.concatenate([_floats(pats), extractor_angles()])
        assert np.all(np.abs(x) < 120)
        return x
    return _once("sincos", make)


def sincos_quadrant(x):
    """(reduced, n): which inputs go through reduce_fast of orb_sincos.h, and its n for them (0 elsewhere)."""
    x = np.asarray(x, f32)
    reduced = ((x.view(u32) >> 20) & 0x7ff) >= SINCOS_TOP12[1]
    r = x.astype(np.float64) * float.fromhex("0x1.45f306dc9c883p+23")
    n = (np.trunc(r).astype(np.int64) + 0x800000) >> 24
    return reduced, np.where(reduced, n, 0)


# ---- atanf -------------------------------------------------------------------------------------------------------------------------------
NANS = (0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fbfffff, 0x7fffffff, 0xffffffff, 0x7fc12345)


def atanf():
    """x for atanf: every 173rd non-negative float and its negative, +-4096 ulps around the seven breakpoints of s_atanf.c in both signs,
    every 1021st denormal, +-inf, NaNs."""
    def make():
        pats = [_both_signs(np.arange(0, INF + 1, 173, dtype=np.int64))]
        pats += [_both_signs(_window(b)) for b in ATANF_BREAKPOINTS]
        pats.append(_both_signs(np.concatenate([np.arange(1, 0x800000, 1021), [0x7fffff]])))
        pats.append(_both_signs([INF]))
        pats.append(NANS)
        return _floats(pats)
    return _once("atanf", make)


# ---- atan2f ------------------------------------------------------------------------------------------------------------------------------
def atan2f_k(y, x):
    """k = (iy - ix) >> 23 of e_atan2f.c."""
    iy = (np.asarray(y, f32).view(u32) & 0x7fffffff).astype(np.int64)
    ix = (np.asarray(x, f32).view(u32) & 0x7fffffff).astype(np.int64)
    return (iy - ix) >> 23


def atan2f_m(y, x):
    """m = 2 * sign(x) + sign(y) of e_atan2f.c."""
    return ((np.asarray(y, f32).view(u32) >> 31) & 1) | ((np.asarray(x, f32).view(u32) >> 30) & 2)


def _signed(iy, ix):
    """Magnitude bit patterns in all four sign combinations."""
    iy, ix = np.asarray(iy, np.int64), np.asarray(ix, np.int64)
    return (np.concatenate([iy, iy | SIGN, iy, iy | SIGN]), np.concatenate([ix, ix, ix | SIGN, ix | SIGN]))


def atan2f_special():
    """(y, x): the 14 x 14 special-value table."""
    def make():
        s = np.array(ATAN2F_SPECIAL, f32)
        y, x = np.meshgrid(s, s, indexing="ij")
        return y.ravel().copy(), x.ravel().copy()
    return _once("atan2f-special", make)


def atan2f_exponent_gaps():
    """(y, x) with k = (iy - ix) >> 23 equal to each of ATAN2F_KS, 2000 pairs per k in each of the four sign combinations: normal x and
    y with random significands."""
    def make():
        rng = np.random.default_rng(20242)
        ys, xs = [], []
        for k in ATAN2F_KS:
            lo, hi = (((2 - k) << 23), 0x7f000000) if k < 0 else (0x00800000, 0x7f000000 - ((k + 1) << 23))
            ix = rng.integers(lo, hi, 2000)
            iy = ix + (k << 23) + rng.integers(0, 1 << 23, 2000)
            assert iy.min() >= 0x00800000 and iy.max() < INF
            sy, sx = _signed(iy, ix)
            ys.append(sy)
            xs.append(sx)
        return _floats(ys), _floats(xs)
    return _once("atan2f-gaps", make)


def _pow2_pairs(rng, n, gap_lo, gap_hi):
    """n pairs of normal floats y, x > 0 with random significands and exponent(y) - exponent(x) in [gap_lo, gap_hi]."""
    gap = rng.integers(gap_lo, gap_hi + 1, n)
    ey = rng.integers(np.maximum(-126, gap - 126), np.minimum(127, 127 + gap) + 1)       # both exponents inside [-126, 127]
    ex = ey - gap
    assert ex.min() >= -126 and ex.max() <= 127
    iy = ((ey + 127) << 23) | rng.integers(0, 1 << 23, n)
    ix = ((ex + 127) << 23) | rng.integers(0, 1 << 23, n)
    return iy, ix


def atan2f_tiny_quotients():
    """(y, x), x > 0, k < -60, the quotient y / x a denormal: 10 000 pairs of normal operands 2^-128 .. 2^-148 apart, 2000 with a denormal
    y over x in [1, 2^20), each with both signs of y."""
    def make():
        rng = np.random.default_rng(20243)
        iy, ix = _pow2_pairs(rng, 10_000, -148, -128)
        dy = rng.integers(1, 0x800000, 2000)
        dx = rng.integers(0x3f800000, 0x49800000, 2000)
        iy, ix = np.concatenate([iy, dy]), np.concatenate([ix, dx])
        return _floats([iy, iy | SIGN]), _floats([ix, ix])
    return _once("atan2f-tiny", make)


def atan2f_underflows():
    """(y, x), x > 0, k < -60, the quotient y / x rounds to zero: 10 000 pairs 2^-152 .. 2^-250 apart, both signs of y."""
    def make():
        rng = np.random.default_rng(20244)
        iy, ix = _pow2_pairs(rng, 10_000, -250, -152)
        return _floats([iy, iy | SIGN]), _floats([ix, ix])
    return _once("atan2f-underflow", make)


def camera_arguments():
    """(y, x): the two calls of KannalaBrandt8::project (KannalaBrandt8.cpp:31-32), psi = atan2f(Y, X) and
    theta = atan2f(sqrtf(X * X + Y * Y), Z), over the points of tests/ref_camera_cases.py for every camera."""
    def make():
        P = np.concatenate([RC.projection_points(name)["X"] for name in RC.CAMERAS]).astype(f32)
        X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
        return np.concatenate([Y, np.sqrt(X * X + Y * Y)]), np.concatenate([X, Z])
    return _once("atan2f-camera", make)


def atan2f():
    """(y, x) for atan2f: the special-value table; per scale 0.5, 10, 1000 a million raw bit-pattern pairs (all magnitudes, zeros,
    infinities, NaNs, denormals) and a million pairs uniform in [-scale, scale]; the exponent gaps; the denormal and the vanishing
    quotients; 10 000 pairs of denormals in each sign combination; x == 1.0f against every 40009th float; the camera arguments."""
    def make():
        ys, xs = zip(atan2f_special(), atan2f_exponent_gaps(), atan2f_tiny_quotients(), atan2f_underflows(), camera_arguments())
        ys, xs = list(ys), list(xs)
        for seed, scale in ((1, 0.5), (2, 10.0), (3, 1000.0)):
            rng = np.random.default_rng(seed)
            raw = rng.integers(0, 1 << 32, (2, 1_000_000), dtype=np.uint64).astype(u32).view(f32)
            uni = rng.uniform(-scale, scale, (2, 1_000_000)).astype(f32)
            ys += [raw[0], uni[0]]
            xs += [raw[1], uni[1]]
        rng = np.random.default_rng(20245)
        dy, dx = _signed(rng.integers(1, 0x800000, 10_000), rng.integers(1, 0x800000, 10_000))
        ys.append(_floats([dy]))
        xs.append(_floats([dx]))
        y1 = _floats([_both_signs(np.arange(0, INF + 1, 40009, dtype=np.int64))])
        ys.append(y1)
        xs.append(np.ones_like(y1))
        return np.concatenate(ys).astype(f32), np.concatenate(xs).astype(f32)
    return _once("atan2f", make)
