"""CPU: the input sets of tests/libm_device_cases.py hold what they claim, and on every one of them the HOST build of the replicas
(orbx_ref_*, the source the kernels compile) equals this host's glibc bit for bit - the host pinning of tests/test_libm_replicas.py and
tests/test_sincos.py extended to the edge sets (exponent gaps of 58 .. 62, denormal and vanishing quotients, denormal pairs, NaNs) that
the random sweeps there do not reach.  The oracle's fastAtan2, which the kernels' fast_atan2_deg is compared with on the device, is held
to the accuracy OpenCV documents for cv::fastAtan2 (about 0.3 degrees) against numpy's float64 arctan2.
tests/test_gpu_libm_device.py runs the device builds over the same sets."""
import numpy as np

import libm_device_cases as D

f32, u32 = np.float32, np.uint32


def member(w, su):
    """Elementwise: w[i] is in the sorted array su."""
    return su[np.minimum(np.searchsorted(su, w), len(su) - 1)] == w


def has_window(su, centre_bits, r=D.ULPS):
    """Every float within r ulps of the one with the (signed) bit pattern centre_bits is in the sorted bit patterns su."""
    mag = centre_bits & 0x7fffffff
    w = (np.arange(max(mag - r, 0), mag + r + 1, dtype=np.int64) | (centre_bits & D.SIGN)).astype(u32)
    return bool(member(w, su).all())


# ---- what the sets hold ------------------------------------------------------------------------------------------------------------------
def test_sincos_set():
    x = D.sincos()
    u = x.view(u32)
    su = np.sort(u)
    assert 8_000_000 < len(x) < 10_000_000 and np.all(np.abs(x) < 120) and not np.isnan(x).any()
    assert f32(-3.2) <= x.min() <= f32(-3.19) and f32(6.29) <= x.max() <= f32(6.3)
    for k in range(-4, 9):
        assert has_window(su, D.bits(k * np.pi / 4)), k
    for t in D.SINCOS_TOP12:
        assert has_window(su, t << 20) and has_window(su, (t << 20) | D.SIGN), hex(t)
    assert su[0] == 0 and member(np.array([D.SIGN], u32), su).all()
    mag = u & 0x7fffffff
    assert np.count_nonzero((mag > 0) & (mag < 0x800000) & (u < D.SIGN)) >= 1000 and np.count_nonzero((mag > 0) & (mag < 0x800000) & (u >= D.SIGN)) >= 1000
    top12 = (u >> 20) & 0x7ff
    early, poly = top12 < D.SINCOS_TOP12[0], (top12 >= D.SINCOS_TOP12[0]) & (top12 < D.SINCOS_TOP12[1])     # the two early returns
    assert np.count_nonzero(early) >= 10_000 and np.count_nonzero(poly) >= 10_000
    reduced, n = D.sincos_quadrant(x)
    assert np.count_nonzero(reduced) >= 300_000 and sorted(set(n[reduced].tolist())) == [-2, -1, 0, 1, 2, 3, 4]
    for q in range(4):
        assert np.count_nonzero(reduced & ((n & 3) == q)) >= 50_000, q
    assert np.count_nonzero(reduced & (x < 0)) >= 100_000 and np.count_nonzero(reduced & (x > 0)) >= 100_000
    a = D.extractor_angles()
    assert len(a) > 280_000 and a.min() == 0 and a.max() == f32(360.0) * f32(np.pi / 180.0) and member(a.view(u32), su).all()


def test_atanf_set():
    x = D.atanf()
    u = x.view(u32)
    su = np.sort(u)
    assert 2 * (D.INF // 173) < len(x) < 2 * (D.INF // 173) + 200_000
    assert member(np.arange(0, D.INF + 1, 173, dtype=np.int64).astype(u32), su).all()
    for b in D.ATANF_BREAKPOINTS:
        assert has_window(su, b) and has_window(su, b | D.SIGN), hex(b)
    mag = u & 0x7fffffff
    assert np.count_nonzero((mag > 0) & (mag < 0x800000)) >= 2 * 8000
    assert member(np.array([D.INF, D.INF | D.SIGN], u32), su).all()
    assert np.count_nonzero(np.isnan(x)) == len(D.NANS) and np.count_nonzero(np.isnan(x) & (u >= D.SIGN)) >= 2
    for lo, hi in zip((0,) + D.ATANF_BREAKPOINTS[:6], D.ATANF_BREAKPOINTS[:6] + (D.INF + 1,)):      # every interval of the reduction, both signs
        assert np.count_nonzero((mag >= lo) & (mag < hi) & (u < D.SIGN)) >= 4000 and np.count_nonzero((mag >= lo) & (mag < hi) & (u >= D.SIGN)) >= 4000


def test_atan2f_set():
    y, x = D.atan2f()
    assert 6_000_000 < len(y) == len(x) < 8_000_000
    num = ~(np.isnan(y) | np.isnan(x))
    assert np.count_nonzero(~num) >= 1000                       # raw bit patterns: NaN operands
    m, k = D.atan2f_m(y, x), D.atan2f_k(y, x)
    for q in range(4):
        assert np.count_nonzero(num & (m == q)) >= 1_000_000, q
    finite = num & np.isfinite(y) & np.isfinite(x) & (y != 0) & (x != 0) & (x != 1)                # the inputs that reach the test of k
    for kk in D.ATAN2F_KS:
        for q in range(4):
            assert np.count_nonzero(finite & (k == kk) & (m == q)) >= 2000, (kk, q)
    assert np.count_nonzero(finite & (k > 62)) >= 1000 and np.count_nonzero(finite & (k < -62) & (x < 0)) >= 1000
    with np.errstate(under="ignore", over="ignore", divide="ignore", invalid="ignore"):
        q = np.abs(y / x)
    far = finite & (x > 0) & (k < -60)
    denormal = far & (q > 0) & (q < f32(2.0 ** -126))
    vanishing = far & (q == 0)
    assert np.count_nonzero(denormal & (y > 0)) >= 100 and np.count_nonzero(denormal & (y < 0)) >= 100
    assert np.count_nonzero(vanishing & (y > 0)) >= 100 and np.count_nonzero(vanishing & (y < 0)) >= 100
    ty, tx = D.atan2f_tiny_quotients()
    with np.errstate(under="ignore"):
        tq = np.abs(ty / tx)
    assert np.count_nonzero((tq > 0) & (tq < f32(2.0 ** -126))) >= 20_000 and np.all(tx > 0) and np.all(D.atan2f_k(ty, tx) < -60)
    uy, ux = D.atan2f_underflows()
    with np.errstate(under="ignore"):
        assert len(uy) == 20_000 and np.all(uy / ux == 0) and np.all(ux > 0) and np.all(uy != 0)
    tiny = f32(2.0 ** -126)
    both = num & (np.abs(y) < tiny) & (np.abs(x) < tiny) & (y != 0) & (x != 0)
    for q in range(4):
        assert np.count_nonzero(both & (m == q)) >= 10_000, q
    assert np.count_nonzero(x == 1) >= 100_000 and np.count_nonzero((x == 1) & (y < 0)) >= 50_000
    sy, sx = D.atan2f_special()
    assert len(sy) == 14 * 14 and np.array_equal(y[:196].view(u32), sy.view(u32)) and np.array_equal(x[:196].view(u32), sx.view(u32))
    cy, cx = D.camera_arguments()
    assert len(cy) >= 2 * 4000
    key = lambda a, b: (a.view(u32).astype(np.uint64) << np.uint64(32)) | b.view(u32)
    assert np.isin(key(cy, cx), key(y, x)).all()


def test_fast_atan2_set():
    y, x = D.fast_atan2()
    assert 4_000_000 < len(y) == len(x) < 5_000_000
    assert np.array_equal(y, np.rint(y)) and np.array_equal(x, np.rint(x)) and np.abs(y).max() == 2 ** 24 and np.abs(x).max() <= 2 ** 24
    n = 2 * D.FAST_ATAN2_SMALL + 1
    sy, sx = D.fast_atan2_small()
    assert len(sy) == n * n and len(set(zip(sy.tolist(), sx.tolist()))) == n * n and np.abs(sy).max() == np.abs(sx).max() == D.FAST_ATAN2_SMALL
    assert np.array_equal(y[:n * n], sy) and np.array_equal(x[:n * n], sx)
    ay, ax = np.abs(y), np.abs(x)
    assert np.count_nonzero(ax > ay) >= 2_000_000 and np.count_nonzero(ax < ay) >= 2_000_000          # both branches
    assert np.count_nonzero((y == 0) & (x == 0)) >= 1 and np.count_nonzero((y == 0) & (x != 0)) >= 2 * D.FAST_ATAN2_SMALL
    assert np.count_nonzero((x == 0) & (y != 0)) >= 2 * D.FAST_ATAN2_SMALL
    for sgy in (1, -1):
        for sgx in (1, -1):
            quad = (np.sign(y) == sgy) & (np.sign(x) == sgx)
            assert np.count_nonzero(quad & (ay == ax) & (ax <= D.FAST_ATAN2_SMALL)) >= D.FAST_ATAN2_SMALL        # the ties
            for d in (0, 1, -1):
                assert np.count_nonzero(quad & (ay == ax + d) & (ax >= 2 ** 20)) >= 10_000, (sgy, sgx, d)


# ---- the host builds on them -------------------------------------------------------------------------------------------------------------
def test_host_cosf_sinf_equal_glibc(pkg, oracle):
    L, O, x = pkg.load(), oracle.lib(), D.sincos()
    for name in ("cosf", "sinf"):
        msg = D.mismatch(name, (x,), oracle.apply_unary(getattr(L, "orbx_ref_" + name), x), oracle.apply_unary(getattr(O, "orc_libm_" + name), x), ("host build", "glibc"))
        assert msg is None, msg


def test_host_atanf_equals_glibc(pkg, oracle):
    x = D.atanf()
    msg = D.mismatch("atanf", (x,), oracle.apply_unary(pkg.load().orbx_ref_atanf, x), oracle.apply_unary(oracle.lib().orc_libm_atanf, x), ("host build", "glibc"))
    assert msg is None, msg


def test_host_atan2f_equals_glibc(pkg, oracle):
    y, x = D.atan2f()
    msg = D.mismatch("atan2f", (y, x), oracle.apply_binary(pkg.load().orbx_ref_atan2f, y, x), oracle.apply_binary(oracle.lib().orc_libm_atan2f, y, x),
                   ("host build", "glibc"))
    assert msg is None, msg


def test_oracle_fast_atan2_within_documented_accuracy(oracle):
    """cv::fastAtan2 is documented as accurate to about 0.3 degrees.  The oracle's restatement against degrees(arctan2) in float64, as
    an angle difference modulo 360, on every pair of the set but (0, 0), where the angle is undefined (fastAtan2 returns 0)."""
    y, x = D.fast_atan2()
    got = oracle.apply_binary(oracle.lib().orc_fast_atan2, y, x)
    assert got.min() >= 0 and got.max() <= 360 and not np.isnan(got).any()
    zero = (y == 0) & (x == 0)
    assert np.all(got[zero] == 0) and 1 <= np.count_nonzero(zero) < 100
    want = np.degrees(np.arctan2(y.astype(np.float64), x.astype(np.float64))) % 360.0
    err = np.abs((got.astype(np.float64) - want + 180.0) % 360.0 - 180.0)[~zero]
    i = int(np.argmax(err))
    assert err[i] <= 0.3, "worst error %.4f degrees at (y, x) = (%r, %r)" % (err[i], y[~zero][i], x[~zero][i])
