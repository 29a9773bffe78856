"""GPU parity of the fused projection search whose list builds run on the FP4 matrix product (serve_mfma of k_match_resolve<Key32,
true, true>; csrc/orb_mfma_util.h, "FP4 form").

The product is exact only if the hardware keeps the integers 2^18 + rank +- 1024 ... in f32 and if candidate and query fragments
share one permutation of the 256 descriptor bits, so the cases here are built from exact data rather than from extracted frames:
every Hamming distance 0..256 in one frame, every single bit position, the smallest and the largest key (rank 0, rank 2047,
distance 256), and the edges of the 32-keypoint tile, of a wavefront's share of the frame and of the 32- / 64-query chunk.
Every launch holds 33 or more small frame pairs (more than 32 query blocks: the batch is not split, engine 2 takes the fused
form, which check_fused asserts), runs with the three Hamming engines and must equal the CPU oracle's in-order loop.

The reference loop starts from bestDist = 256 and replaces it on a strictly smaller distance only (ORBmatcher.cc:99-120), and the
library accepts thresholds up to 255, so a candidate at distance 256 takes part in every list as the largest key but is never
matched: the query that is left with it alone must come back unmatched, on the device as in the oracle.  The every-distance
case therefore asserts the matched distances 0..255, each once and in query order, and that last query."""
import numpy as np
import pytest

from test_gpu_fused_footprint import SF, check_fused
from test_gpu_mfma import H, W, free_frame

pytestmark = pytest.mark.gpu

BOUNDS = (0.0, float(W), 0.0, float(H))       # 64 x 48 grid cells
HELD = 1 << 20                                # some earlier map point


def keypoints(pkg, x, y, rng):
    n = len(x)
    k = np.zeros(n, dtype=pkg.KP_DTYPE)
    k["x"] = np.asarray(x, np.float32); k["y"] = np.asarray(y, np.float32)
    k["octave"] = rng.integers(0, 8, n); k["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    return k


def random_xy(rng, n):
    return rng.uniform(20, W - 20, n), rng.uniform(20, H - 20, n)


def cell_centres(cells):
    """Centres of grid cells given in column-major order (cell = column * 48 + row): GetFeaturesInArea's enumeration order, so
    keypoints at increasing cells have increasing ranks.  Frame::PosInGrid rounds (Frame.cc:815-827), so cell c is centred on c
    cell widths from the origin."""
    cells = np.asarray(cells)
    return (cells // 48) * (W / 64.0), (cells % 48) * (H / 48.0)


def flip_bits(desc, positions):
    d = desc.copy()
    for b in positions:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def bit_order(rng):
    """All 256 bit positions, shuffled; the first 16 take one bit from either half of each of the eight 32-bit words."""
    head = np.array([32 * w + 16 * h + rng.integers(0, 16) for w in range(8) for h in range(2)])
    rng.shuffle(head)
    rest = np.setdiff1d(np.arange(256), head)
    rng.shuffle(rest)
    return np.concatenate([head, rest])


def same_queries(d, nq, obs=True):
    return dict(d=np.repeat(d[None, :], nq, 0), u=np.full(nq, W / 2, np.float32), v=np.full(nq, H / 2, np.float32),
                r=np.full(nq, 1.0e4, np.float32), lo=np.full(nq, -1, np.int32), hi=np.full(nq, -1, np.int32),
                flags=np.full(nq, 3 if obs else 1, np.uint8))


def every_distance_pair(pkg, rng, extra=6):
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    order = bit_order(rng)
    desc = [flip_bits(base, order[:j]) for j in range(257)]
    # a few more candidates, at distances 120 +- 20 from the base, each distance twice with the ladder's: the grid-walk order decides
    desc += [flip_bits(base, rng.permutation(256)[:100 + 8 * e]) for e in range(extra)]
    desc = np.stack(desc)
    perm = rng.permutation(len(desc))
    desc = desc[perm]
    k = keypoints(pkg, *random_xy(rng, len(desc)), rng)
    return free_frame(k, desc), same_queries(base, len(desc))


def test_every_distance_oracle_alone(pkg, oracle):
    """The construction does what the device test relies on (CPU only in effect: the oracle's loop, no launch)."""
    rng = np.random.default_rng(900)
    c, q = every_distance_pair(pkg, rng)
    from test_gpu_mfma import oracle_pair
    n, moq, bd, slot, _ = oracle_pair(oracle, c, q, BOUNDS, SF, 0.8, 255, False)
    nq = len(bd)
    assert n == nq - 1 and sorted(bd[:-1]) == sorted(list(range(256)) + [100 + 8 * e for e in range(6)])
    assert np.all(np.diff(bd[:-1]) >= 0)                       # in query order: every claim takes the nearest keypoint left
    assert moq[-1] == -1 and bd[-1] == 256                     # only the distance-256 keypoint is left: never a match
    assert len(set(moq[:-1])) == nq - 1


def test_every_distance(pkg, oracle, capfd, monkeypatch):
    """257 keypoints at the distances 0, 1, ..., 256 from one descriptor (flipped bits spread over all words and halves, positions
    shuffled) and a few more; as many identical open queries, no second-best test, the largest threshold.  The sequential claims
    hand the keypoints out in distance order, so every distance is a best distance once."""
    rng = np.random.default_rng(901)
    pairs = [every_distance_pair(pkg, rng) for _ in range(17)]          # 263 queries: two blocks per pair, 34 blocks
    cand, qry = [p[0] for p in pairs], [p[1] for p in pairs]
    ref = check_fused(pkg, oracle, capfd, monkeypatch, cand, qry, BOUNDS, SF, True, nnratio=0.8, th=255, second=False, min_total=17 * 262)
    for n, moq, bd, _, _ in ref:
        assert n == len(bd) - 1 and set(range(256)) <= set(bd[:-1].tolist()) and bd[-1] == 256 and moq[-1] == -1


def test_single_bit_sensitivity(pkg, oracle, capfd, monkeypatch):
    """256 keypoints that differ from the query in one bit each, every position once, and one at distance 0 that a map point with
    observations holds: every query must find distance 1 (a dropped bit would give 0, a bit counted twice 2), in grid-walk order."""
    rng = np.random.default_rng(902)
    cand, qry = [], []
    for p in range(33):
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        desc = np.stack([flip_bits(base, [b]) for b in range(256)] + [base])
        perm = rng.permutation(257)
        desc = desc[perm]
        c = free_frame(keypoints(pkg, *random_xy(rng, 257), rng), desc)
        held = int(np.nonzero(perm == 256)[0][0])
        c["slot"][held] = HELD; c["sobs"][held] = 1
        cand.append(c)
        qry.append(same_queries(base, 256))
    ref = check_fused(pkg, oracle, capfd, monkeypatch, cand, qry, BOUNDS, SF, True, nnratio=0.8, th=255, second=False, min_total=33 * 256)
    for n, moq, bd, _, _ in ref:
        assert n == 256 and np.all(bd == 1) and len(set(moq.tolist())) == 256


def test_key_extremes(pkg, oracle, capfd, monkeypatch):
    """2048-keypoint frames whose decisive keypoints sit in the first and in the last grid cell: rank 0 at distance 0 (the key 0),
    equal distances at ranks 2046 and 2047 (the lower rank first), and a distance-256 keypoint at rank 2047 (the largest key) that
    is all a query has left."""
    rng = np.random.default_rng(903)
    cand, qry = [], []
    for p in range(33):
        n = 2048
        x, y = random_xy(rng, n)
        desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        ia, ib, ic = sorted(rng.choice(n, 3, replace=False).tolist())      # ib < ic: both in the last cell, ranks 2046 and 2047
        x[ia], y[ia] = 1.0, 1.0
        cx, cy = cell_centres([63 * 48 + 47])                               # PosInGrid rounds: the last cell is centred here
        x[ib], y[ib] = cx[0], cy[0]
        x[ic], y[ic] = x[ib] + 1.0, y[ib] - 1.0
        q0 = desc[ia].copy()
        c = free_frame(keypoints(pkg, x, y, rng), desc)
        if p % 2 == 0:
            # ties at the last two ranks, each nearer than anything else; then the first rank at distance 0
            tie = rng.integers(0, 256, 32, dtype=np.uint8)
            desc[ib] = flip_bits(tie, [3, 77, 130]); desc[ic] = flip_bits(tie, [40, 201, 255])
            q = same_queries(tie, 5)
            q["d"][3] = q0; q["d"][4] = q0
        else:
            # everything held but rank 0 (distance 0) and rank 2047 (distance 256)
            desc[ic] = ~q0
            c["slot"][:] = HELD; c["sobs"][:] = 1
            c["slot"][[ia, ic]] = -1; c["sobs"][[ia, ic]] = 0
            q = same_queries(q0, 3)
        cand.append(c)
        qry.append(q)
    ref = check_fused(pkg, oracle, capfd, monkeypatch, cand, qry, BOUNDS, SF, True, nnratio=0.8, th=255, second=False, min_total=33)
    for p, (n, moq, bd, _, _) in enumerate(ref):
        if p % 2 == 0:
            assert bd[0] == 3 and bd[1] == 3 and moq[0] < moq[1] and bd[3] == 0
        else:
            assert n == 1 and bd[0] == 0 and list(moq[1:]) == [-1, -1] and list(bd[1:]) == [256, 256]


def test_tile_and_chunk_edges(pkg, oracle, capfd, monkeypatch):
    """256 keypoints at rank = their place in a column-major walk over cell centres, so each of the four wavefronts' shares is 64
    consecutive ranks; all are held except 0, 1, 31, 32 or 33 per share (no tile, one row, a tile less one, a full tile, a tile
    and one row), or except a single keypoint of the frame.  1, 32, 33, 64 and 65 queries: one or two query tiles, one or two
    chunks."""
    rng = np.random.default_rng(904)
    counts = (0, 1, 31, 32, 33)
    cand, qry = [], []
    cases = [(tuple(counts[(a + s) % 5] for s in range(4)), nq) for a in range(5) for nq in (1, 32, 33, 64, 65)]
    cases += [(tuple(1 if s == w else 0 for s in range(4)), nq) for w in range(4) for nq in (1, 65)]
    for usable, nq in cases:
        n = 256
        x, y = cell_centres(np.arange(n) * 12)
        perm = rng.permutation(n)                                          # keypoint perm[r] has rank r
        desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        k = keypoints(pkg, np.zeros(n), np.zeros(n), rng)
        k["x"][perm] = x.astype(np.float32); k["y"][perm] = y.astype(np.float32)
        c = free_frame(k, desc)
        c["slot"][:] = HELD; c["sobs"][:] = 1
        free = np.concatenate([perm[64 * s + rng.permutation(64)[:u]] for s, u in enumerate(usable)]).astype(np.int64)
        c["slot"][free] = -1; c["sobs"][free] = 0
        src = free[rng.integers(0, len(free), nq)]                          # queries near free keypoints: several ask for the same one
        qd = desc[src].copy(); qd[rng.random((nq, 32)) < 0.05] ^= 8
        q = same_queries(qd[0], nq)
        q["d"] = qd
        cand.append(c)
        qry.append(q)
    assert len(cand) >= 33
    check_fused(pkg, oracle, capfd, monkeypatch, cand, qry, BOUNDS, SF, True, nnratio=0.8, th=100, second=True, min_total=100)
