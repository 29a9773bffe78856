"""orbx_compute_stereo_matches_batch_device: Frame::ComputeStereoMatches (Frame.cc:901-1079) for batches of frame pairs that never
leave the device - row table, descriptor search, SAD refinement and the median filter (as a rank selection) in three kernels.

Reference everywhere: the CPU oracle, per frame, bit patterns of mvuRight and mvDepth, plus d_nstereo.  The conditions that keep a
run from passing on empty results or on a filter that never fires come from the numpy model (tests/stereo_model.py)."""
import ctypes as C

import numpy as np
import pytest

import stereo_model as SM
from conftest import TUMVI

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-777.25)
_ref = {}


def reference(oracle, cfg, imgL, imgR, mb, mbf):
    """Oracle extraction of both images (lapping area {0, 0}) and its ComputeStereoMatches."""
    key = (tuple(sorted(cfg.items())), imgL.shape, imgL.tobytes(), imgR.tobytes(), float(mb), float(mbf))
    if key not in _ref:
        o = oracle.OracleExtractor(**cfg)
        _, kL, dL = o.extract(imgL, (0, 0))
        _, kR, dR = o.extract(imgR, (0, 0))
        uR, z = o.compute_stereo_matches(imgL, imgR, kL, dL, kR, dR, mb, mbf)
        _ref[key] = (kL, dL, kR, dR, uR, z)
    return _ref[key]


class Batch:
    pass


def run_batch(pkg, exL, exR, pairs, mb, mbf, cap_extra=0, stream=None, nstereo=True, nframes=None):
    """Extract the left and the right images of `pairs` as two batches and run the new call on `stream` (a torch stream or None =
    the current one); one synchronise at the end.  Returns the downloaded arrays."""
    import torch
    n = len(pairs)
    H, W = pairs[0][0].shape
    dev = torch.device("cuda", 0)
    st = stream if stream is not None else torch.cuda.current_stream()
    B = Batch()
    with torch.cuda.stream(st):
        d_L = torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev)
        d_R = torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev)
        cap = max(exL.configure(H, W, n), exR.configure(H, W, n)) + cap_extra
        mk = lambda: (torch.zeros((n, cap, 7), dtype=torch.float32, device=dev), torch.zeros((n, cap, 32), dtype=torch.uint8, device=dev),
                      torch.zeros((n, 2), dtype=torch.int32, device=dev))
        kL, dL, cL = mk()
        kR, dR, cR = mk()
        uR = torch.full((n, cap), float(SENTINEL), dtype=torch.float32, device=dev)
        z = torch.full((n, cap), float(SENTINEL), dtype=torch.float32, device=dev)
        ns = torch.full((n,), -5, dtype=torch.int32, device=dev)
        s = st.cuda_stream
        exL.extract_batch_device(d_L.data_ptr(), H, W, W, H * W, n, kL.data_ptr(), dL.data_ptr(), cL.data_ptr(), cap, (0, 0), stream=s)
        exR.extract_batch_device(d_R.data_ptr(), H, W, W, H * W, n, kR.data_ptr(), dR.data_ptr(), cR.data_ptr(), cap, (0, 0), stream=s)
        nf = n if nframes is None else nframes
        exL.compute_stereo_matches_batch_device(exR, nf, kL.data_ptr(), dL.data_ptr(), cL.data_ptr(), kR.data_ptr(), dR.data_ptr(), cR.data_ptr(),
                                                cap, mb, mbf, uR.data_ptr(), z.data_ptr(), ns.data_ptr() if nstereo else None, stream=s)
    B.dev = (d_L, d_R, kL, dL, cL, kR, dR, cR, uR, z, ns)     # kept alive until the caller has synchronised
    B.cap, B.n, B.nf = cap, n, nf
    return B


def download(pkg, B):
    import torch
    torch.cuda.synchronize()
    d_L, d_R, kL, dL, cL, kR, dR, cR, uR, z, ns = B.dev
    B.cL, B.cR = cL.cpu().numpy(), cR.cpu().numpy()
    B.kL = kL.cpu().numpy().view(np.uint8).reshape(B.n, B.cap, 28)
    B.kR = kR.cpu().numpy().view(np.uint8).reshape(B.n, B.cap, 28)
    B.dL, B.dR = dL.cpu().numpy(), dR.cpu().numpy()
    B.uR, B.z, B.ns = uR.cpu().numpy(), z.cpu().numpy(), ns.cpu().numpy()
    return B


def check(pkg, oracle, cfg, B, pairs, mb, mbf, nstereo=True):
    """Every frame of the batch against the oracle: the extraction (so that both sides match the same keypoints), the bits of
    mvuRight / mvDepth for i < n_left, the sentinel beyond, d_nstereo.  Returns the per-frame number of stereo matches."""
    counts = []
    for f, (imgL, imgR) in enumerate(pairs):
        kL, dL, kR, dR, uR, z = reference(oracle, cfg, imgL, imgR, mb, mbf)
        nL, nR = len(kL), len(kR)
        assert B.cL[f, 0] == nL and B.cR[f, 0] == nR, (f, B.cL[f], nL, B.cR[f], nR)
        assert B.kL[f, :nL].tobytes() == kL.tobytes() and B.kR[f, :nR].tobytes() == kR.tobytes()
        if f >= B.nf:
            assert (B.uR[f] == SENTINEL).all() and (B.z[f] == SENTINEL).all() and B.ns[f] == -5
            continue
        bad = np.nonzero(B.uR[f, :nL].view(np.uint32) != uR.view(np.uint32))[0]
        assert len(bad) == 0, "frame %d: %d of %d mvuRight differ, first %s" % (f, len(bad), nL, [(int(i), float(B.uR[f, i]), float(uR[i])) for i in bad[:4]])
        assert np.array_equal(B.z[f, :nL].view(np.uint32), z.view(np.uint32)), f
        assert (B.uR[f, nL:] == SENTINEL).all() and (B.z[f, nL:] == SENTINEL).all(), f
        want = int((uR >= 0).sum())
        assert want == int((z >= 0).sum())
        if nstereo:
            assert B.ns[f] == want, (f, B.ns[f], want)
        else:
            assert B.ns[f] == -5
        counts.append(want)
    return counts


def extractors(pkg, cfg):
    return pkg.ORBextractor(**cfg), pkg.ORBextractor(**cfg)


def eight_pairs(synth):
    if "eight" not in _ref:
        flat = SM.flat_image()
        _ref["eight"] = SM.scene_list(synth) + [SM.identical_pair(synth), (flat, flat)]
    return list(_ref["eight"])


def test_scene_list(pkg, oracle, synth):
    """1: one batch of 8 EuRoC pairs - six ordinary ones (disparities, noise, one row of misalignment), the identical pair, an empty
    pair.  The model's conditions: at least 500 matches remain and at least 20 are removed by the filter in every ordinary frame."""
    pairs = eight_pairs(synth)
    for imgL, imgR in pairs[:6]:
        o, lvL, lvR, sf, invsf, kL, dL, kR, dR = SM.oracle_inputs(oracle, SM.EUROC_STEREO, imgL, imgR)
        info = SM.compute_stereo_matches(lvL, lvR, sf, invsf, kL, dL, kR, dR, SM.MB, SM.MBF)[2]
        print("model: keypoints %d accepted %d removed %d remaining %d" % (len(kL), info["accepted"], info["removed"], info["remaining"]))
        assert info["remaining"] >= 500 and info["removed"] >= 20
    exL, exR = extractors(pkg, SM.EUROC_STEREO)
    B = download(pkg, run_batch(pkg, exL, exR, pairs, SM.MB, SM.MBF))
    counts = check(pkg, oracle, SM.EUROC_STEREO, B, pairs, SM.MB, SM.MBF)
    print("stereo matches per frame:", counts)
    assert min(counts[:6]) >= 500 and counts[6] == 0 and counts[7] == 0
    exL.close(); exR.close()


def test_identical_pair(pkg, oracle, synth):
    """2: right image = left image: every accepted match has SAD 0, the median is 0, thDist is 0, the filter resets them all."""
    pairs = [eight_pairs(synth)[k] for k in (0, 6, 2)]
    kL, dL, kR, dR, uR, z = reference(oracle, SM.EUROC_STEREO, *pairs[1], SM.MB, SM.MBF)
    assert len(kL) > 1000 and (uR == -1).all() and (z == -1).all()
    exL, exR = extractors(pkg, SM.EUROC_STEREO)
    B = download(pkg, run_batch(pkg, exL, exR, pairs, SM.MB, SM.MBF))
    counts = check(pkg, oracle, SM.EUROC_STEREO, B, pairs, SM.MB, SM.MBF)
    assert (B.uR[1, :len(kL)] == -1).all() and (B.z[1, :len(kL)] == -1).all() and B.ns[1] == 0
    assert counts[0] >= 500 and counts[2] >= 500
    exL.close(); exR.close()


def test_empty_side(pkg, oracle, synth):
    """3: a flat image (no keypoints) as left, as right and as both, between ordinary frames: all -1 there, neighbours unaffected."""
    flat = SM.flat_image()
    sc = eight_pairs(synth)
    pairs = [sc[0], (flat, sc[1][1]), sc[1], (sc[2][0], flat), (flat, flat), sc[3]]
    o = oracle.OracleExtractor(**SM.EUROC_STEREO)
    assert len(o.extract(flat, (0, 0))[1]) == 0
    exL, exR = extractors(pkg, SM.EUROC_STEREO)
    B = download(pkg, run_batch(pkg, exL, exR, pairs, SM.MB, SM.MBF))
    counts = check(pkg, oracle, SM.EUROC_STEREO, B, pairs, SM.MB, SM.MBF)
    assert counts[1] == counts[3] == counts[4] == 0 and min(counts[0], counts[2], counts[5]) >= 500
    assert B.cL[3, 0] > 1000 and (B.uR[3, :B.cL[3, 0]] == -1).all()
    exL.close(); exR.close()


def test_batch_equals_loop(pkg, oracle, synth):
    """4: the same batch through the existing per-frame entry point (host keypoints, host median filter) gives identical bits."""
    pairs = eight_pairs(synth)
    exL, exR = extractors(pkg, SM.EUROC_STEREO)
    B = download(pkg, run_batch(pkg, exL, exR, pairs, SM.MB, SM.MBF))
    total = 0
    for f in range(len(pairs)):
        nL, nR = int(B.cL[f, 0]), int(B.cR[f, 0])
        kL = B.kL[f, :nL].copy().view(pkg.KP_DTYPE).reshape(nL)
        kR = B.kR[f, :nR].copy().view(pkg.KP_DTYPE).reshape(nR)
        uR, z = exL.ComputeStereoMatches(exR, kL, B.dL[f, :nL], kR, B.dR[f, :nR], SM.MB, SM.MBF, frame_l=f, frame_r=f)
        assert np.array_equal(uR.view(np.uint32), B.uR[f, :nL].view(np.uint32)), f
        assert np.array_equal(z.view(np.uint32), B.z[f, :nL].view(np.uint32)), f
        assert int((uR >= 0).sum()) == B.ns[f]
        total += int(B.ns[f])
    assert total >= 3000
    exL.close(); exR.close()


@pytest.mark.parametrize("nframes,cap_extra,own_stream", [(1, 0, False), (3, 0, True), (8, 0, False), (3, 37, False), (8, 512, True), (1, 64, True)])
def test_layouts_and_launch_forms(pkg, oracle, synth, nframes, cap_extra, own_stream):
    """5: batches of 1, 3 and 8, cap equal to orbx_max_keypoints and larger, the current stream and a stream of the caller's;
    entries beyond the live count keep the sentinel (check())."""
    import torch
    pairs = eight_pairs(synth)[:nframes] if nframes != 3 else [eight_pairs(synth)[k] for k in (4, 6, 1)]
    exL, exR = extractors(pkg, SM.EUROC_STEREO)
    st = torch.cuda.Stream() if own_stream else None
    B = download(pkg, run_batch(pkg, exL, exR, pairs, SM.MB, SM.MBF, cap_extra=cap_extra, stream=st, nstereo=nframes != 3 or cap_extra == 0))
    assert B.cap == exL.max_keypoints() + cap_extra
    counts = check(pkg, oracle, SM.EUROC_STEREO, B, pairs, SM.MB, SM.MBF, nstereo=nframes != 3 or cap_extra == 0)
    assert max(counts) >= 500
    exL.close(); exR.close()


def test_back_to_back_and_partial(pkg, oracle, synth):
    """5: two calls back to back on the same handles with different batches (the scratch is reused, the second batch is smaller,
    then larger again), and a call for fewer frames than the handles' last batch: the frames beyond are not touched."""
    all_pairs = eight_pairs(synth)
    exL, exR = extractors(pkg, SM.EUROC_STEREO)
    b1 = run_batch(pkg, exL, exR, all_pairs[:5], SM.MB, SM.MBF)
    b2 = run_batch(pkg, exL, exR, [all_pairs[k] for k in (5, 2)], SM.MB, SM.MBF)
    b3 = run_batch(pkg, exL, exR, [all_pairs[k] for k in (3, 7, 0, 6, 5, 1, 4, 2)], SM.MB, SM.MBF, cap_extra=100)
    b4 = run_batch(pkg, exL, exR, all_pairs[:4], SM.MB, SM.MBF, nframes=2)
    for B, pairs in ((b1, all_pairs[:5]), (b2, [all_pairs[k] for k in (5, 2)]), (b3, [all_pairs[k] for k in (3, 7, 0, 6, 5, 1, 4, 2)]), (b4, all_pairs[:4])):
        counts = check(pkg, oracle, SM.EUROC_STEREO, download(pkg, B), pairs, SM.MB, SM.MBF)
        assert max(counts) >= 500
    exL.close(); exR.close()


@pytest.mark.parametrize("name,cfg,H,W", [("tumvi", TUMVI, 512, 512), ("levels3", dict(SM.EUROC_STEREO, nlevels=3), 480, 752),
                                          ("features300", dict(SM.EUROC_STEREO, nfeatures=300), 480, 752)])
def test_other_configurations(pkg, oracle, synth, name, cfg, H, W):
    """6: TUM-VI-like 512 x 512 with 1500 features, a 3-level pyramid, 300 features."""
    rng = np.random.default_rng(41)
    pairs = [SM.stereo_pair(synth, 7200 + k, d, H, W, noise_rng=rng if k == 1 else None, roll=k == 2) for k, d in enumerate((12, 33, 21))]
    exL, exR = extractors(pkg, cfg)
    B = download(pkg, run_batch(pkg, exL, exR, pairs, SM.MB, SM.MBF))
    counts = check(pkg, oracle, cfg, B, pairs, SM.MB, SM.MBF)
    print(name, "stereo matches per frame:", counts)
    assert min(counts) >= (100 if name == "features300" else 300)
    exL.close(); exR.close()


def test_fuzz_slice(pkg, oracle, synth):
    """6: 12 random cases in the shape of tests/fuzz_parity.py::fuzz_stereo (sizes 240-640 x 160-420, 3-8 levels, 300 / 800 / 1200
    features, mb, mbf, noise and row roll drawn as there), two or three per batch call - a batch shares size and settings, its
    frames differ in image, disparity, noise and roll, hence in keypoint count.  A configuration the extractor refuses is skipped;
    more than 2 skipped cases fail the test."""
    rng = np.random.default_rng(20261)
    skipped, done, matches, varied = 0, 0, 0, 0
    for group in (3, 2, 3, 2, 2):
        H, W = int(rng.integers(160, 420)), int(rng.integers(240, 640))
        cfg = dict(nfeatures=int(rng.choice([300, 800, 1200])), scaleFactor=1.2, nlevels=int(rng.integers(3, 9)), iniThFAST=20, minThFAST=7)
        mbf = float(rng.uniform(20.0, 80.0)); mb = mbf / float(rng.uniform(300.0, 500.0))
        pairs = []
        for _ in range(group):
            seed, disp = int(rng.integers(1, 1 << 30)), int(rng.integers(1, 60))
            noise, roll = rng.random() < 0.5, rng.random() < 0.3
            pairs.append(SM.stereo_pair(synth, seed, disp, H, W, noise_rng=rng if noise else None, roll=roll))
        try:
            exL, exR = extractors(pkg, cfg)
            B = run_batch(pkg, exL, exR, pairs, mb, mbf)
        except (pkg.OrbError, ValueError) as err:      # the documented geometry limits of orbx_configure
            print("refused %dx%d %s: %s" % (W, H, cfg, err))
            skipped += group
            continue
        counts = check(pkg, oracle, cfg, download(pkg, B), pairs, mb, mbf)
        varied += len(set(int(c) for c in B.cL[:, 0])) > 1          # the frames of a batch differ in keypoint count
        done += group
        matches += sum(counts)
        exL.close(); exR.close()
    print("fuzz slice: %d cases compared, %d skipped, %d stereo matches" % (done, skipped, matches))
    assert skipped <= 2 and done + skipped == 12 and matches >= 100 * done and varied >= 2


# ---- 7: the chained stereo step ----------------------------------------------------------------------------------------------
EUROC_STEREO_CAM = np.array([435.2046959714599, 435.2046959714599, 367.4517211914062, 252.2008514404297], np.float32)   # Examples/Stereo/EuRoC.yaml
EUROC_BF = np.float32(47.90639384423901)
CHAIN = ((7302, 40, (2, 2)), (7303, 58, (3, -2)), (7304, 25, (-2, 1)))


def chain_scene(synth, oracle, seed, disp, shift):
    H, W = 480, 752
    canvas = synth.make_frame(seed, H + 32, W + 96)
    crop = lambda ox, oy: np.ascontiguousarray(canvas[oy:oy + H, ox:ox + W])
    dx, dy = shift
    cur_l, cur_r, last_l = crop(16, 16), crop(16 + disp, 16), crop(16 + dx, 16 + dy)     # last (x, y) is seen at (x + dx, y + dy) now
    fx, fy, cx, cy = [float(v) for v in EUROC_STEREO_CAM]
    z = float(EUROC_BF) / disp
    o = oracle.OracleExtractor(**SM.EUROC_STEREO)
    _, k0, d0 = o.extract(last_l, (0, 0))
    t = np.array([dx * z / fx, dy * z / fy, 0.0])
    rng = np.random.default_rng(seed)
    far = rng.random(len(k0)) < 0.4                    # at 2z on the same ray of the current camera: right coordinate disp / 2 away
    u, v = k0["x"].astype(np.float64) + dx, k0["y"].astype(np.float64) + dy
    zc = np.where(far, 2 * z, z)
    Xc = np.stack([(u - cx) * zc / fx, (v - cy) * zc / fy, zc], axis=1)
    Xw = np.ascontiguousarray((Xc - t[None, :]).astype(np.float32))
    Tcw = np.eye(4, dtype=np.float32)
    Tcw[:3, 3] = t.astype(np.float32)
    has = (rng.random(len(k0)) < 0.8).astype(np.uint8)
    obs = (rng.random(len(k0)) < 0.9).astype(np.uint8)
    return dict(cur_l=cur_l, cur_r=cur_r, last_l=last_l, k0=k0, d0=d0, Xw=Xw, Tcw=Tcw, has=has, obs=obs, far=far)


def test_chained_stereo_step(pkg, oracle, synth):
    """7: extract left, extract right, stereo matches, last-frame search with u_right = d_uRight, on one stream with one synchronise.
    40 % of the map points sit at twice the stereo depth: they project onto their keypoint but their right coordinate is disp / 2
    away, so the gate of ORBmatcher.cc:2139-2146 rejects them when u_right is right and accepts them when it is all -1."""
    import torch
    H, W = 480, 752
    BOUNDS = (0.0, float(W), 0.0, float(H))
    mbf = float(EUROC_BF); mb = float(EUROC_BF / EUROC_STEREO_CAM[0])
    scenes = [chain_scene(synth, oracle, *c) for c in CHAIN]
    n = len(scenes)
    o = oracle.OracleExtractor(**SM.EUROC_STEREO)
    sf = np.ascontiguousarray(o.scale_factors, np.float32)
    # oracle side first: its own extraction, its own uRight, the search with and without it
    want = []
    for S in scenes:
        k1, d1, kR, dR, uR, z = reference(oracle, SM.EUROC_STEREO, S["cur_l"], S["cur_r"], mb, mbf)
        res = []
        for ur in (uR, np.full(len(k1), -1, np.float32)):
            OF = oracle.OracleFrame(k1["x"], k1["y"], k1["octave"], k1["angle"], d1, BOUNDS, sf, u_right=ur)
            nm = OF.search_by_projection_ff(S["has"], S["Xw"], S["d0"], S["k0"]["octave"], S["k0"]["angle"], S["Tcw"], np.eye(4, dtype=np.float32), 0,
                                            EUROC_STEREO_CAM, 7.0, mono=False, check_ori=True, mb=mb, mbf=mbf, qobs=S["obs"])
            res.append((nm, OF.slot.copy(), OF.slot_obs.copy()))
        differ = int((res[0][1] != res[1][1]).sum())
        print("oracle: %d matches with uRight, %d without, %d slots differ, %d stereo matches" % (res[0][0], res[1][0], differ, int((uR >= 0).sum())))
        assert res[0][0] >= 400 and differ >= 100
        want.append((res[0], k1, uR))
    dev = torch.device("cuda", 0)
    exL, exR, exP = pkg.ORBextractor(**SM.EUROC_STEREO), pkg.ORBextractor(**SM.EUROC_STEREO), pkg.ORBextractor(**SM.EUROC_STEREO)
    m = pkg.ORBmatcher(0.9, True)
    cap = exL.configure(H, W, n)
    assert exR.configure(H, W, n) == cap and exP.configure(H, W, n) == cap
    pad = lambda a: np.concatenate([a, np.zeros((cap - len(a),) + a.shape[1:], a.dtype)])
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_imgs = [t(np.stack([S[k] for S in scenes])) for k in ("cur_l", "cur_r", "last_l")]
        d_Xw, d_has, d_obs = t(np.stack([pad(S["Xw"]) for S in scenes])), t(np.stack([pad(S["has"]) for S in scenes])), t(np.stack([pad(S["obs"]) for S in scenes]))
        d_Tcw = t(np.stack([S["Tcw"].reshape(-1) for S in scenes]))
        d_Tlw = t(np.stack([np.eye(4, dtype=np.float32).reshape(-1)] * n))
        outs = []
        for ex, d_img in zip((exL, exR, exP), d_imgs):
            k = torch.zeros((n, cap, 7), dtype=torch.float32, device=dev)
            d = torch.zeros((n, cap, 32), dtype=torch.uint8, device=dev)
            c = torch.zeros((n, 2), dtype=torch.int32, device=dev)
            ex.extract_batch_device(d_img.data_ptr(), H, W, W, H * W, n, k.data_ptr(), d.data_ptr(), c.data_ptr(), cap, (0, 0), stream=st.cuda_stream)
            outs.append((k, d, c))
        (kL, dL, cL), (kR, dR, cR), (kP, dP, cP) = outs
        d_uR = torch.full((n, cap), float(SENTINEL), dtype=torch.float32, device=dev)
        d_z = torch.full((n, cap), float(SENTINEL), dtype=torch.float32, device=dev)
        exL.compute_stereo_matches_batch_device(exR, n, kL.data_ptr(), dL.data_ptr(), cL.data_ptr(), kR.data_ptr(), dR.data_ptr(), cR.data_ptr(), cap, mb, mbf,
                                                d_uR.data_ptr(), d_z.data_ptr(), None, stream=st.cuda_stream)
        d_slot = torch.full((n, cap), -1, dtype=torch.int32, device=dev)
        d_sobs = torch.zeros((n, cap), dtype=torch.uint8, device=dev)
        d_nm = torch.zeros((n,), dtype=torch.int32, device=dev)
        cur = pkg.FrameStruct(cap, kL.data_ptr(), dL.data_ptr(), d_uR.data_ptr(), *[C.c_float(b) for b in BOUNDS])
        last = pkg.LastFrameStruct(cap, d_has.data_ptr(), d_Xw.data_ptr(), dP.data_ptr(), kP.data_ptr(), d_obs.data_ptr(), d_Tcw.data_ptr(), d_Tlw.data_ptr())
        rc = m.L.orbm_search_by_projection_last_frame_batch_device(
            m.m, C.byref(cur), cap, C.c_void_p(cL.data_ptr()), 2, C.byref(last), cap, C.c_void_p(cP.data_ptr()), 2, n,
            sf.ctypes.data_as(C.c_void_p), len(sf), 0, EUROC_STEREO_CAM.ctypes.data_as(C.c_void_p), C.c_float(mb), C.c_float(mbf), C.c_float(7.0), 0, 1,
            C.c_void_p(d_slot.data_ptr()), C.c_void_p(d_sobs.data_ptr()), None, C.c_void_p(d_nm.data_ptr()), C.c_void_p(st.cuda_stream))
        assert rc == 0, m.L.orbm_last_error(m.m)
    torch.cuda.synchronize()          # the one synchronisation of the chain
    slot, sobs, nm, uRg, cPh = d_slot.cpu().numpy(), d_sobs.cpu().numpy(), d_nm.cpu().numpy(), d_uR.cpu().numpy(), cP.cpu().numpy()
    kPh = kP.cpu().numpy().view(np.uint8).reshape(n, cap, 28)
    for p, S in enumerate(scenes):
        (n_ref, slot_ref, sobs_ref), k1, uR = want[p]
        assert cPh[p, 0] == len(S["k0"]) and kPh[p, :len(S["k0"])].tobytes() == S["k0"].tobytes()
        assert np.array_equal(uRg[p, :len(k1)].view(np.uint32), uR.view(np.uint32))
        assert nm[p] == n_ref, (p, nm[p], n_ref)
        assert np.array_equal(slot[p, :len(k1)], slot_ref) and np.array_equal(sobs[p, :len(k1)], sobs_ref)
    m.close(); exL.close(); exR.close(); exP.close()


def test_refusals_with_live_handles(pkg, oracle, synth):
    """8: mismatched handles, nframes beyond the last batch, mb = 0, a cap below orbx_max_keypoints or above 65535, a missing array,
    and handles that have not extracted yet: ORBX_E_ARG (ValueError) with a message, nothing launched."""
    import torch
    pairs = eight_pairs(synth)[:2]
    exL, exR = extractors(pkg, SM.EUROC_STEREO)
    fresh = pkg.ORBextractor(**SM.EUROC_STEREO)
    B = run_batch(pkg, exL, exR, pairs, SM.MB, SM.MBF)
    torch.cuda.synchronize()
    d_L, d_R, kL, dL, cL, kR, dR, cR, uR, z, ns = B.dev
    before = (uR.clone(), z.clone())
    other_levels = pkg.ORBextractor(**dict(SM.EUROC_STEREO, nlevels=6))
    other_size = pkg.ORBextractor(**SM.EUROC_STEREO)
    for ex, (H, W) in ((other_levels, (480, 752)), (other_size, (400, 640))):
        img = torch.from_numpy(np.stack([synth.make_frame(5, H, W)] * 2)).cuda()
        cap2 = ex.configure(H, W, 2)
        k2, d2, c2 = torch.zeros((2, cap2, 7), device="cuda"), torch.zeros((2, cap2, 32), dtype=torch.uint8, device="cuda"), torch.zeros((2, 2), dtype=torch.int32, device="cuda")
        ex.extract_batch_device(img.data_ptr(), H, W, W, H * W, 2, k2.data_ptr(), d2.data_ptr(), c2.data_ptr(), cap2, (0, 0))
        torch.cuda.synchronize()
    good = dict(right=exR, nframes=2, d_keysL=kL.data_ptr(), d_descL=dL.data_ptr(), d_countsL=cL.data_ptr(), d_keysR=kR.data_ptr(), d_descR=dR.data_ptr(),
                d_countsR=cR.data_ptr(), cap=B.cap, mb=SM.MB, mbf=SM.MBF, d_uRight=uR.data_ptr(), d_depth=z.data_ptr(), d_nstereo=ns.data_ptr())
    cases = [dict(right=other_levels), dict(right=other_size), dict(right=fresh), dict(nframes=3), dict(nframes=0), dict(nframes=-1), dict(mb=0.0),
             dict(mb=-0.1), dict(cap=exL.max_keypoints() - 1), dict(cap=65536), dict(d_keysL=0), dict(d_descR=0), dict(d_countsR=0), dict(d_uRight=0),
             dict(d_depth=0)]
    for c in cases:
        with pytest.raises(ValueError) as ei:
            exL.compute_stereo_matches_batch_device(**dict(good, **c))
        assert "orbx_compute_stereo_matches_batch_device" in str(ei.value), (c, str(ei.value))
    with pytest.raises(ValueError):
        fresh.compute_stereo_matches_batch_device(**good)
    torch.cuda.synchronize()
    assert torch.equal(uR, before[0]) and torch.equal(z, before[1])
    exL.compute_stereo_matches_batch_device(**dict(good, cap=B.cap, d_nstereo=None))       # and the good call still works
    torch.cuda.synchronize()
    check(pkg, oracle, SM.EUROC_STEREO, download(pkg, B), pairs, SM.MB, SM.MBF)
    for e in (exL, exR, fresh, other_levels, other_size):
        e.close()
