"""numpy restatement of the bookkeeping orbx_compute_stereo_matches_batch_device adds to Frame::ComputeStereoMatches
(Frame.cc:901-1079), in the tradition of octree_model.py / resolve_model.py / local_map_model.py:

  (i)  the row table (vRowIndices, :911-928) as a CSR table of 8-row bands whose records carry the exact row range: the
       candidates of a left keypoint are the records of the band of its row that pass the exact row test;
  (ii) the median filter (:1065-1078) as a rank selection: the value at rank nDI / 2 of the ascending SADs found by two 256-bin
       histogram passes, then one threshold compare per match.

compute_stereo_matches() restates the member far enough to produce the pre-filter SADs, in the reference's fp32 expressions (numpy
float32 scalars keep every intermediate in fp32), and is checked bit for bit against oracle.OracleExtractor.compute_stereo_matches
in tests/test_stereo_model.py.  The GPU tests take their conditions (matches before the filter, matches the filter removes) from
here."""
import numpy as np

BAND = 8
TH_HIGH, TH_LOW = 100, 50
F = np.float32
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def row_ranges(kyR, octR, sf, rows):
    """minr / maxr of every right keypoint (:916-918)."""
    r = (F(2.0) * np.asarray(sf, F)[np.asarray(octR)]).astype(F)
    ky = np.asarray(kyR, F)
    maxr = np.ceil((ky + r).astype(F)).astype(np.int64)
    minr = np.floor((ky - r).astype(F)).astype(np.int64)
    return minr, maxr


def reference_row_table(kyR, octR, sf, rows):
    """vRowIndices as the reference builds it: row -> right indices in push (= index) order."""
    minr, maxr = row_ranges(kyR, octR, sf, rows)
    table = [[] for _ in range(rows)]
    for iR in range(len(minr)):
        for y in range(max(int(minr[iR]), 0), min(int(maxr[iR]), rows - 1) + 1):
            table[y].append(iR)
    return table


def band_table(kyR, octR, sf, rows, order_rng=None):
    """CSR over bands of BAND rows: (start[nbands + 1], rec_idx, rec_minr, rec_maxr).  A keypoint is entered in every band its clamped
    row range touches.  order_rng shuffles the records inside each band (the device fills them with atomics, in any order)."""
    minr, maxr = row_ranges(kyR, octR, sf, rows)
    nbands = (rows + BAND - 1) // BAND
    bands = [[] for _ in range(nbands)]
    for iR in range(len(minr)):
        lo, hi = max(int(minr[iR]), 0), min(int(maxr[iR]), rows - 1)
        if lo > hi:
            continue
        for b in range(lo // BAND, hi // BAND + 1):
            bands[b].append(iR)
    if order_rng is not None:
        for b in bands:
            order_rng.shuffle(b)
    start = np.zeros(nbands + 1, np.int64)
    for b in range(nbands):
        start[b + 1] = start[b] + len(bands[b])
    idx = np.array([i for b in bands for i in b], np.int64)
    return start, idx, minr[idx] if len(idx) else idx, maxr[idx] if len(idx) else idx


def band_candidates(table, row):
    """The right indices a left keypoint of this row looks at: its band's records after the exact row test (any order)."""
    start, idx, minr, maxr = table
    s, e = int(start[row // BAND]), int(start[row // BAND + 1])
    keep = (minr[s:e] <= row) & (row <= maxr[s:e])
    return idx[s:e][keep]


def max_bands_per_keypoint(sf, rows):
    """The host's bound on the number of bands one right keypoint can enter (sizes the record scratch)."""
    span = int(F(4.0) * F(max(sf))) + 4
    return min((rows + BAND - 1) // BAND, (span + 6) // BAND + 1)


def rank_select(sads):
    """Value at rank len(sads) // 2 of the ascending SADs by two 256-bin histogram passes (a SAD is below 2^16)."""
    sads = np.asarray(sads, np.int64)
    assert len(sads) > 0 and sads.min() >= 0 and sads.max() < 65536
    rank = len(sads) // 2
    h = np.bincount(sads >> 8, minlength=256)
    c = np.cumsum(h)
    hi = int(np.searchsorted(c, rank, side="right"))           # first bin whose cumulative count exceeds the rank
    rank -= int(c[hi] - h[hi])
    h2 = np.bincount(sads[(sads >> 8) == hi] & 255, minlength=256)
    lo = int(np.searchsorted(np.cumsum(h2), rank, side="right"))
    return (hi << 8) | lo


def filter_select(sads):
    """Mask of the matches the filter resets, by selection + threshold (the device's form)."""
    sads = np.asarray(sads, np.int64)
    if len(sads) == 0:
        return np.zeros(0, bool)
    thDist = F(1.5) * F(1.4) * F(rank_select(sads))
    return sads.astype(F) >= thDist


def filter_sort(sads):
    """The same mask as the reference computes it: sort the (sad, index) pairs, walk down from the end, stop at the first below."""
    sads = np.asarray(sads, np.int64)
    out = np.zeros(len(sads), bool)
    if len(sads) == 0:
        return out
    order = sorted(range(len(sads)), key=lambda i: (int(sads[i]), i))
    median = F(sads[order[len(order) // 2]])
    thDist = F(1.5) * F(1.4) * median
    for i in reversed(order):
        if F(sads[i]) < thDist:
            break
        out[i] = True
    return out


def _roundf(x):
    x = float(x)
    return F(np.trunc(x + (0.5 if x >= 0 else -0.5)))


def compute_stereo_matches(levelsL, levelsR, sf, invsf, keysL, descL, keysR, descR, mb, mbf, use_bands=True, order_rng=None):
    """Returns (uRight, depth, info).  info: sad (pre-filter best SAD per left keypoint or -1), accepted, removed, remaining,
    candidates (per left keypoint: the right indices looked at, sorted)."""
    sf, invsf = np.asarray(sf, F), np.asarray(invsf, F)
    rows = levelsL[0].shape[0]
    nL, nR = len(keysL), len(keysR)
    uRight, depth, sad = np.full(nL, -1, F), np.full(nL, -1, F), np.full(nL, -1, np.int64)
    kxR, kyR, octR = keysR["x"].astype(F), keysR["y"].astype(F), keysR["octave"].astype(np.int64)
    table = band_table(kyR, octR, sf, rows, order_rng) if use_bands else reference_row_table(kyR, octR, sf, rows)
    mb, mbf = F(mb), F(mbf)
    minD, maxD = F(0), mbf / mb
    thOrbDist = (TH_HIGH + TH_LOW) // 2
    dR = np.asarray(descR, np.uint8).reshape(nR, 32)
    dLall = np.asarray(descL, np.uint8).reshape(nL, 32)
    cands = []
    w = L = 5
    with np.errstate(all="ignore"):
        for iL in range(nL):
            uL, vL, levelL = F(keysL["x"][iL]), F(keysL["y"][iL]), int(keysL["octave"][iL])
            row = int(vL)
            cands.append(np.zeros(0, np.int64))
            if row < 0 or row >= rows:
                continue
            c = np.asarray(band_candidates(table, row) if use_bands else table[row], np.int64)
            cands[-1] = np.sort(c)
            if len(c) == 0:
                continue
            minU, maxU = uL - maxD, uL - minD
            if maxU < 0:
                continue
            c = c[(octR[c] >= levelL - 1) & (octR[c] <= levelL + 1)]
            c = c[(kxR[c] >= minU) & (kxR[c] <= maxU)]
            if len(c) == 0:
                continue
            dist = _POP[dR[c] ^ dLall[iL]].sum(axis=1)
            c, dist = c[dist < TH_HIGH], dist[dist < TH_HIGH]
            if len(c) == 0:
                continue
            key = int(((dist.astype(np.int64) << 16) | c).min())          # first minimum in iR order, whatever the order of c
            bestDist, bestIdxR = key >> 16, key & 0xffff
            if bestDist >= thOrbDist:
                continue
            uR0 = kxR[bestIdxR]
            scaleFactor = invsf[levelL]
            scaleduL, scaledvL, scaleduR0 = _roundf(uL * scaleFactor), _roundf(vL * scaleFactor), _roundf(uR0 * scaleFactor)
            IL, IR = levelsL[levelL], levelsR[levelL]
            lh, lw = IL.shape
            cuL, cvL, cuR = int(scaleduL), int(scaledvL), int(scaleduR0)
            if cvL - w < 0 or cvL + w + 1 > lh or cuL - w < 0 or cuL + w + 1 > lw:
                continue
            iniu, endu = scaleduR0 + F(L) - F(w), scaleduR0 + F(L) + F(w) + F(1)
            if iniu < 0 or endu >= F(lw) or cuR - L - w < 0:
                continue
            A = IL[cvL - w:cvL + w + 1, cuL - w:cuL + w + 1].astype(np.int64) - int(IL[cvL, cuL])
            sads = []
            for incR in range(-L, L + 1):
                B = IR[cvL - w:cvL + w + 1, cuR + incR - w:cuR + incR + w + 1].astype(np.int64) - int(IR[cvL, cuR + incR])
                sads.append(int(np.abs(A - B).sum()))
            bestSad, bestincR = 2147483647, 0
            for k, s in enumerate(sads):
                if F(s) < F(bestSad):
                    bestSad, bestincR = s, k - L
            if bestincR == -L or bestincR == L:
                continue
            dist1, dist2, dist3 = F(sads[L + bestincR - 1]), F(sads[L + bestincR]), F(sads[L + bestincR + 1])
            deltaR = (dist1 - dist3) / (F(2.0) * (dist1 + dist3 - F(2.0) * dist2))
            if deltaR < -1 or deltaR > 1:
                continue
            bestuR = sf[levelL] * (scaleduR0 + F(bestincR) + deltaR)
            disparity = uL - bestuR
            if disparity >= minD and disparity < maxD:
                if disparity <= 0:
                    disparity = F(0.01)
                    bestuR = F(np.float64(uL) - 0.01)
                depth[iL] = mbf / disparity
                uRight[iL] = bestuR
                sad[iL] = bestSad
    acc = np.nonzero(sad >= 0)[0]
    removed = filter_select(sad[acc])
    uRight[acc[removed]] = -1
    depth[acc[removed]] = -1
    info = dict(sad=sad, accepted=len(acc), removed=int(removed.sum()), remaining=int(len(acc) - removed.sum()), candidates=cands)
    return uRight, depth, info


def oracle_inputs(oracle, cfg, imgL, imgR):
    """Everything compute_stereo_matches needs, from the oracle's extraction of the two images (lapping area {0, 0}, Frame.cc:120-121)."""
    o = oracle.OracleExtractor(**cfg)
    _, kL, dL = o.extract(imgL, (0, 0))
    _, kR, dR = o.extract(imgR, (0, 0))
    nl = cfg["nlevels"]
    sf = np.array(o.e.mvScaleFactor[:nl], F)
    invsf = np.array(o.e.mvInvScaleFactor[:nl], F)
    return o, o.pyramid(imgL), o.pyramid(imgR), sf, invsf, kL, dL, kR, dR


# ---- the scene list of the issue, shared by the CPU and the GPU tests ------------------------------------------------
EUROC_STEREO = dict(nfeatures=1200, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7)   # Examples/Stereo/EuRoC.yaml
MB, MBF = 0.11, 47.9
DISPARITIES = (3, 17, 40, 58, 25, 9)


def stereo_pair(synth, seed, disp, H=480, W=752, noise_rng=None, roll=False):
    """Left and right image cut from one wider synthetic frame (tests/fuzz_parity.py::fuzz_stereo)."""
    big = synth.make_frame(seed, H, W + 64)
    imgL = np.ascontiguousarray(big[:, 0:W])
    imgR = np.ascontiguousarray(big[:, disp:disp + W])
    if noise_rng is not None:
        imgR = (imgR.astype(np.int32) + noise_rng.integers(-6, 7, imgR.shape)).clip(0, 255).astype(np.uint8)
    if roll:
        imgR = np.roll(imgR, 1, axis=0)
    return imgL, np.ascontiguousarray(imgR)


def scene_list(synth):
    """The six ordinary pairs: disparities 3, 17, 40, 58, 25, 9; odd frames with +-6 uniform noise on the right image; the
    disparity-25 frame with the right image rolled down by one row."""
    rng = np.random.default_rng(7000)
    out = []
    for f, disp in enumerate(DISPARITIES):
        out.append(stereo_pair(synth, 7000 + f, disp, noise_rng=rng if f % 2 == 1 else None, roll=disp == 25))
    return out


def identical_pair(synth):
    img = synth.make_frame(7100, 480, 752)
    return img, img.copy()


def flat_image(H=480, W=752):
    return np.full((H, W), 90, np.uint8)
