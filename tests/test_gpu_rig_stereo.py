"""Frame::ComputeStereoFishEyeMatches on the device (orbm_stereo_fisheye_matches_batch_device, orbm_stereo_fisheye_matches): the
device builds of the restated arithmetic against their host evaluations (which tests/test_tanf_replica.py and
tests/test_rig_stereo_math.py compare with libm and with the numpy model), and the batch call against tests/rig_stereo_model.py, bit
for bit in every output, at both output layouts, without the counters, and through the per-frame form."""
import ctypes as C

import numpy as np
import pytest

import rig_stereo_model as M

pytestmark = pytest.mark.gpu
f32 = np.float32

CAP = 2112
MONO = (3, 5)                                            # monoLeft, monoRight: nonzero and different
LAPPING = ((0, 5), (7, 1), (33, 70), (300, 2050))        # (left, right) lapping rows per frame: an empty side; fewer than two train rows;
#                                                          ranges ending inside a 32-row tile and a 64-query block; a train range across
#                                                          the 2048-row super-block (and a second workgroup of 256 queries)
ISENT, FSENT = 12345, -777.25


@pytest.fixture(scope="module")
def matcher(pkg):
    m = pkg.ORBmatcher(0.8, True)
    yield m
    m.close()


# ---- device arithmetic ---------------------------------------------------------------------------------------------------------------
def test_tanf_device_equals_host(pkg):
    import torch
    bits = lambda x: int(np.array([x], f32).view(np.uint32)[0])
    hpi = np.pi / 2
    pats = [np.arange(0, bits(2.0) + 1, 19997, dtype=np.uint32), np.arange(bits(120.0), 0x7f800000, 39989, dtype=np.uint32)]
    for p in (np.pi / 4, 3 * np.pi / 4, hpi, 0.6744, hpi - 0.6744, hpi + 0.6744, 2.0 ** -13, hpi - 2.0 ** -13, 2.0, 119.0, 120.0, 811.62, 1e6, 1e20,
              3.0e38):                                      # from 120 on the reduction is the integer one
        pats.append(np.arange(bits(p) - 4096, bits(p) + 4097, dtype=np.uint32))
    pats = np.concatenate(pats)
    pats = np.concatenate([pats, pats | np.uint32(0x80000000), np.array([0, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 1, 0x42f00000], np.uint32)])
    x = pats.view(f32)
    d_x = torch.from_numpy(x.copy()).cuda()
    d_y = torch.zeros_like(d_x)
    assert pkg.load().orbx_tanf_device(C.c_void_p(d_x.data_ptr()), len(x), C.c_void_p(d_y.data_ptr()), None) == 0
    torch.cuda.synchronize()
    got = d_y.cpu().numpy().view(np.uint32)
    host = pkg.load().orbx_ref_tanf
    want = np.array(list(map(host, x.tolist())), f32).view(np.uint32)
    nan = lambda u: (u & 0x7fffffff) > 0x7f800000
    bad = np.flatnonzero((got != want) & ~(nan(got) & nan(want)))
    assert len(bad) == 0, (len(bad), x[bad[:5]], got[bad[:5]], want[bad[:5]])


def test_triangulate_device_equals_host(pkg):
    import torch
    kp1, kp2, s1, s2 = M.synthetic_pairs(4000)
    depth, p3d = pkg.fisheye_triangulate(kp1, kp2, s1, s2, M.TLR, M.CAM1, M.CAM2, p3d_fill=FSENT)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = [t(kp1), t(kp2), t(s1), t(s2)]
    d_depth, d_p3d = t(np.full(len(kp1), FSENT, f32)), t(np.full((len(kp1), 3), FSENT, f32))
    assert pkg.fisheye_triangulate_device(len(kp1), *[a.data_ptr() for a in d], M.TLR, M.CAM1, M.CAM2, d_depth.data_ptr(), d_p3d.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (depth > 0).sum() > 1000 and (depth == -1).sum() > 1000
    assert d_depth.cpu().numpy().view(np.uint32).tolist() == depth.view(np.uint32).tolist()
    assert np.array_equal(d_p3d.cpu().numpy().view(np.uint32), p3d.view(np.uint32))


# ---- the batch call against the model ------------------------------------------------------------------------------------------------
def make_frames(pkg):
    """Four rig frames written directly (no extraction).  A left lapping row q has a partner right lapping row: its descriptor with
    0-10 flipped bits and the right keypoint of a synthetic rig pair, so most pairs pass the ratio test and the triangulation decides.
    Added: left rows with a random descriptor (the ratio test fails), exact duplicates among the train rows (d0 == d1: it fails),
    groups of left rows copied from one right row with the keypoint of its partner (several accepted left keypoints share a right
    one: the last in left order must stay in mvRightToLeftMatch)."""
    rng = np.random.default_rng(77)
    kp1, kp2, _, _ = M.synthetic_pairs(400, seed=5)
    s0 = M.LEVEL_SIGMA2[0]                                        # accepted at the strictest gate: accepted at every octave
    sure = [i for i in range(40) if M.triangulate_matches(M.CAM1, M.CAM2, kp1[i], kp2[i], M.TLR, s0, s0)[2] == M.ACCEPT]
    frames = []
    for f, (lapL, lapR) in enumerate(LAPPING):
        nL, nR = MONO[0] + lapL, MONO[1] + lapR
        kL, kR = np.zeros(nL, pkg.KP_DTYPE), np.zeros(nR, pkg.KP_DTYPE)
        dL, dR = rng.integers(0, 256, (nL, 32), dtype=np.uint8), rng.integers(0, 256, (nR, 32), dtype=np.uint8)
        for k, n in ((kL, nL), (kR, nR)):
            k["x"], k["y"] = rng.uniform(0, 512, n).astype(f32), rng.uniform(0, 512, n).astype(f32)
            k["octave"] = rng.integers(0, 8, n)
        npart = min(lapL, lapR)
        rows = rng.permutation(lapR)[:npart]                      # right lapping row of left lapping row q < npart
        if lapR > 2048:                                           # two partners behind the first 2048 train rows, on pairs that triangulate
            rows[:2] = (lapR - 1, 2048)
            rows[2:] = [j for j in rng.permutation(2048)[: npart - 2]]
        for q in range(npart):
            li, rj = MONO[0] + q, MONO[1] + int(rows[q])
            pair = int(sure[q]) if lapR > 2048 and q < 2 else int(rng.integers(0, len(kp1)))
            kL["x"][li], kL["y"][li] = kp1[pair]
            kR["x"][rj], kR["y"][rj] = kp2[pair]
            d = dL[li].copy()
            flip = rng.permutation(256)[: int(rng.integers(0, 11))]
            np.bitwise_xor.at(d, flip >> 3, (1 << (flip & 7)).astype(np.uint8))
            dR[rj] = d
        if npart >= 30:
            free = np.setdiff1d(np.arange(lapR), rows)
            for q in 2 + rng.permutation(npart - 2)[: npart // 8]:   # no partner: a random descriptor (rows 0 and 1 stay as they are)
                dL[MONO[0] + q] = rng.integers(0, 256, 32, dtype=np.uint8)
            for q, j in zip(2 + rng.permutation(npart - 2)[: npart // 10], free):   # the partner's row twice among the train rows
                dR[MONO[1] + int(j)] = dR[MONO[1] + int(rows[q])]
            for g in range(max(2, npart // 12)):                  # three left rows on one right row
                src = int(rng.integers(2, npart))
                for q in 2 + rng.permutation(npart - 2)[:3]:
                    if q != src:
                        dL[MONO[0] + q] = dR[MONO[1] + int(rows[src])]
                        kL[MONO[0] + q] = kL[MONO[0] + src]
        frames.append(dict(kL=kL, dL=dL, kR=kR, dR=dR, nL=nL, nR=nR))
    return frames


@pytest.fixture(scope="module")
def problem(pkg):
    """The frames and the model's results: computed once, shared, never modified."""
    frames = make_frames(pkg)
    for F in frames:
        F["E"] = M.stereo_fisheye_matches(F["kL"], F["dL"], MONO[0], F["kR"], F["dR"], MONO[1], M.LEVEL_SIGMA2, M.TLR, M.CAM1, M.CAM2,
                                          p3d=np.full((F["nL"], 3), FSENT, f32))
    return frames


def test_model_conditions(problem):
    """What the comparisons below need, judged from the model alone."""
    for F, (lapL, lapR) in zip(problem, LAPPING):
        l2r, r2l, depth, p3d, (nm, nd) = F["E"]
        print("lapping (%d, %d): nMatches %d, descMatches %d" % (lapL, lapR, nm, nd))
        if lapL == 0 or lapR < 2:
            assert nm == nd == 0 and (l2r == -1).all() and (r2l == -1).all()
    assert any(F["E"][4][0] < F["E"][4][1] for F in problem)                  # a frame where the triangulation rejects
    big = problem[3]["E"]
    assert big[4][0] > 50 and big[4][1] < LAPPING[3][0]                       # matches, and ratio-test failures
    shared = np.bincount(big[0][big[0] >= 0], minlength=problem[3]["nR"])
    assert (shared >= 2).sum() >= 2                                           # several accepted left keypoints on one right one
    for j in np.flatnonzero(shared >= 2):
        assert big[1][j] == np.flatnonzero(big[0] == j).max()                 # ... and the last in left order holds it
    assert (big[0][big[0] >= 0] >= 2048 + MONO[1]).any()                      # a match beyond the first train super-block


def run_batch(pkg, matcher, frames, out_stride, counters=True):
    import torch
    n = len(frames)
    kL, kR = np.zeros((n, CAP), pkg.KP_DTYPE), np.zeros((n, CAP), pkg.KP_DTYPE)
    dL, dR = np.full((n, CAP, 32), 0xA5, np.uint8), np.full((n, CAP, 32), 0x5A, np.uint8)
    cL, cR = np.zeros((n, 2), np.int32), np.zeros((n, 2), np.int32)
    for f, F in enumerate(frames):
        kL[f, :F["nL"]], dL[f, :F["nL"]], cL[f] = F["kL"], F["dL"], (F["nL"], MONO[0])
        kR[f, :F["nR"]], dR[f, :F["nR"]], cR[f] = F["kR"], F["dR"], (F["nR"], MONO[1])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8) if a.dtype == pkg.KP_DTYPE else np.ascontiguousarray(a)).cuda()
    D = [t(kL), t(dL), t(cL), t(kR), t(dR), t(cR)]
    l2r = torch.full((n, out_stride), ISENT, dtype=torch.int32, device="cuda")
    r2l = torch.full((n, out_stride), ISENT, dtype=torch.int32, device="cuda")
    depth = torch.full((n, out_stride), FSENT, dtype=torch.float32, device="cuda")
    p3d = torch.full((n, out_stride, 3), FSENT, dtype=torch.float32, device="cuda")
    nm = torch.full((n, 2), ISENT, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    st.synchronize()
    torch.cuda.synchronize()
    matcher.stereo_fisheye_matches_batch_device(n, *[a.data_ptr() for a in D], CAP, M.LEVEL_SIGMA2, M.TLR, M.CAM1, M.CAM2, out_stride, l2r.data_ptr(),
                                                r2l.data_ptr(), depth.data_ptr(), p3d.data_ptr(), nm.data_ptr() if counters else None, stream=st.cuda_stream)
    st.synchronize()
    return [a.cpu().numpy() for a in (l2r, r2l, depth, p3d, nm)]


def check_frame(got, F, counters=True):
    l2r, r2l, depth, p3d, nm = got
    E = F["E"]
    nL, nR = F["nL"], F["nR"]
    assert np.array_equal(l2r[:nL], E[0]) and (l2r[nL:] == ISENT).all()
    assert np.array_equal(r2l[:nR], E[1]) and (r2l[nR:] == ISENT).all()
    assert depth[:nL].view(np.uint32).tolist() == E[2].view(np.uint32).tolist() and (depth[nL:] == f32(FSENT)).all()
    assert np.array_equal(p3d[:nL].view(np.uint32), E[3].view(np.uint32)) and (p3d[nL:] == f32(FSENT)).all()   # unmatched entries keep the caller's values
    assert tuple(nm) == (E[4] if counters else (ISENT, ISENT))


@pytest.mark.parametrize("out_stride,counters", [(CAP, True), (2 * CAP, True), (CAP + 5, False)], ids=["stride-cap", "stride-2cap", "no-counters"])
def test_batch_equals_model(pkg, matcher, problem, out_stride, counters):
    got = run_batch(pkg, matcher, problem, out_stride, counters)
    for f, F in enumerate(problem):
        check_frame([a[f] for a in got], F, counters)


def test_per_frame_form_equals_model(pkg, matcher, problem):
    for F in problem:
        l2r, r2l, depth, p3d, nm = matcher.ComputeStereoFishEyeMatches(F["kL"], F["dL"], MONO[0], F["kR"], F["dR"], MONO[1], M.LEVEL_SIGMA2, M.TLR, M.CAM1,
                                                                        M.CAM2, p3d=np.full((F["nL"], 3), FSENT, f32))
        E = F["E"]
        assert np.array_equal(l2r, E[0]) and np.array_equal(r2l, E[1]) and depth.view(np.uint32).tolist() == E[2].view(np.uint32).tolist()
        assert np.array_equal(p3d.view(np.uint32), E[3].view(np.uint32)) and nm == E[4]
    # an octave outside the pyramid on a lapping keypoint: refused here (a non-match in the batch form)
    F = problem[2]
    kL = F["kL"].copy()
    kL["octave"][MONO[0] + 1] = 8
    with pytest.raises(ValueError):
        matcher.ComputeStereoFishEyeMatches(kL, F["dL"], MONO[0], F["kR"], F["dR"], MONO[1], M.LEVEL_SIGMA2, M.TLR, M.CAM1, M.CAM2)
    kL["octave"][MONO[0] + 1], kL["octave"][0] = F["kL"]["octave"][MONO[0] + 1], -4        # a monocular keypoint's octave is never read
    assert matcher.ComputeStereoFishEyeMatches(kL, F["dL"], MONO[0], F["kR"], F["dR"], MONO[1], M.LEVEL_SIGMA2, M.TLR, M.CAM1, M.CAM2)[4] == F["E"][4]


def test_octave_outside_pyramid_is_a_non_match(pkg, matcher, problem):
    F = dict(problem[2])
    E = F["E"]
    hit = int(np.flatnonzero(E[0] >= 0)[0])
    kL = F["kL"].copy()
    kL["octave"][hit] = 9
    G = dict(F, kL=kL)
    G["E"] = M.stereo_fisheye_matches(kL, F["dL"], MONO[0], F["kR"], F["dR"], MONO[1], M.LEVEL_SIGMA2, M.TLR, M.CAM1, M.CAM2, p3d=np.full((F["nL"], 3), FSENT, f32))
    assert G["E"][0][hit] == -1 and G["E"][4][0] == E[4][0] - 1
    got = run_batch(pkg, matcher, [G], CAP)
    check_frame([a[0] for a in got], G)


def test_refusals_with_a_handle(pkg, matcher, problem):
    """The library's own refusals: nothing is launched, the outputs stay as they were.  nframes == 0 returns 0."""
    import torch
    L = pkg.load()
    buf = torch.full((4096,), ISENT, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    sig, T, c1, c2 = M.LEVEL_SIGMA2.copy(), np.ascontiguousarray(M.TLR), M.CAM1.copy(), M.CAM2.copy()
    d = C.c_void_p(buf.data_ptr())
    names = ["m", "nframes", "keysL", "descL", "countsL", "keysR", "descR", "countsR", "cap", "sig", "nlevels", "Tlr", "c1", "c2", "out_stride", "l2r", "r2l",
             "depth", "p3d", "nm", "stream"]
    good = dict(m=matcher.m, nframes=1, keysL=d, descL=d, countsL=d, keysR=d, descR=d, countsR=d, cap=8, sig=p(sig), nlevels=8, Tlr=p(T), c1=p(c1), c2=p(c2),
                out_stride=8, l2r=d, r2l=d, depth=d, p3d=d, nm=None, stream=None)
    call = lambda **kw: L.orbm_stereo_fisheye_matches_batch_device(*[dict(good, **kw)[k] for k in names])
    bad = [dict(m=None)] + [{k: None} for k in ("keysL", "descL", "countsL", "keysR", "descR", "countsR", "sig", "Tlr", "c1", "c2", "l2r", "r2l", "depth", "p3d")]
    bad += [dict(nframes=-1), dict(nframes=65536), dict(cap=0), dict(cap=-1), dict(cap=pkg.FISHEYE_MAX_KEYPOINTS // 2 + 1, out_stride=pkg.FISHEYE_MAX_KEYPOINTS),
            dict(out_stride=7), dict(nlevels=0), dict(nlevels=17)]
    for c in bad:
        assert call(**c) == pkg.E_ARG, c
    assert call(nframes=0) == 0
    torch.cuda.synchronize()
    assert bool((buf == ISENT).all())
