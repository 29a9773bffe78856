"""GPU parity of the fused projection search (k_match_resolve<Key32, true, true>) with its descriptors and candidate records in a
global-memory table of the matcher (d_cand) instead of LDS.

The table holds, per frame pair, the records and descriptors of its keypoints in sorted (cell, index) order at a stride of the
launch's frame stride (maxn).  The launches here use a frame stride equal to the largest frame (no padding), so a 2048-keypoint frame
really is a Key32 launch, and enough query blocks (npairs * blocks > 32) that the batch is not split into latency-mode slices: with
engine 2 every launch below takes the fused form, and each test checks that it did through the library's ORBHIP_PRINT_RESOLVE_LDS
line.  Covered: 1000- and 2048-keypoint frames and tile tails mixed in one launch, claimed occupants, equal distances (ties decided
by the grid-walk order), pairs with windowed queries that are not fused but run inside the fused launch (the wide and chunked forms,
whose refresh scans read the same table), and both sides of the Key32 bound that decides fused admission (2048 fused, 2049 not).
Every case runs with the three Hamming engines and must equal the CPU oracle's in-order loop."""
import ctypes as C
import re

import numpy as np
import pytest

from test_gpu_mfma import H, W, free_frame, open_queries, oracle_pair

pytestmark = pytest.mark.gpu

SF = np.array([1.2 ** i for i in range(8)], np.float32)
FORM = re.compile(r"orbhip: resolve maxn (\d+) fused (\d) dynamic LDS (\d+) bytes")


def run_batch_exact(pkg, m, cand, qry, bounds, nnratio, th, second):
    """As test_gpu_mfma.run_batch, but the frame stride is the largest frame and the query stride the largest query count."""
    import torch
    npairs = len(cand)
    capn = max(len(c["k"]) for c in cand)
    capq = max(len(q["u"]) for q in qry)
    kp = np.zeros((npairs, capn, 7), np.float32); de = np.zeros((npairs, capn, 32), np.uint8); cn = np.zeros((npairs, 2), np.int32)
    slot = np.full((npairs, capn), -1, np.int32); sobs = np.zeros((npairs, capn), np.uint8)
    qd = np.zeros((npairs, capq, 32), np.uint8); qn = np.zeros((npairs, 2), np.int32)
    u = np.zeros((npairs, capq), np.float32); v = np.zeros((npairs, capq), np.float32); r = np.zeros((npairs, capq), np.float32)
    lo = np.zeros((npairs, capq), np.int32); hi = np.zeros((npairs, capq), np.int32); fl = np.zeros((npairs, capq), np.uint8)
    for p, (c, q) in enumerate(zip(cand, qry)):
        n, nq = len(c["k"]), len(q["u"])
        kp[p, :n] = np.ascontiguousarray(c["k"]).view(np.float32).reshape(n, 7); de[p, :n] = c["d"]; cn[p, 0] = n
        slot[p, :n] = c["slot"]; sobs[p, :n] = c["sobs"]
        qd[p, :nq] = q["d"]; qn[p, 0] = nq
        u[p, :nq] = q["u"]; v[p, :nq] = q["v"]; r[p, :nq] = q["r"]; lo[p, :nq] = q["lo"]; hi[p, :nq] = q["hi"]; fl[p, :nq] = q["flags"]
    t = lambda a: torch.from_numpy(a).to("cuda")
    d = dict(kp=t(kp), de=t(de), cn=t(cn), slot=t(slot), sobs=t(sobs), qd=t(qd), qn=t(qn), u=t(u), v=t(v), r=t(r), lo=t(lo), hi=t(hi), fl=t(fl))
    moq = torch.full((npairs, capq), -7, dtype=torch.int32, device="cuda"); bd = torch.zeros((npairs, capq), dtype=torch.int32, device="cuda")
    nm = torch.zeros((npairs,), dtype=torch.int32, device="cuda")
    fs = pkg.FrameStruct(capn, d["kp"].data_ptr(), d["de"].data_ptr(), None, *bounds)
    qs = pkg.QueryStruct(capq, d["qd"].data_ptr(), d["u"].data_ptr(), d["v"].data_ptr(), d["r"].data_ptr(), d["lo"].data_ptr(), d["hi"].data_ptr(), None, d["fl"].data_ptr())
    rc = m.L.orbm_search_by_projection_batch_device(m.m, C.byref(fs), capn, C.c_void_p(d["cn"].data_ptr()), 2, C.byref(qs), capq,
                                                    C.c_void_p(d["qn"].data_ptr()), 2, npairs, C.c_float(nnratio), int(th), int(second),
                                                    C.c_void_p(d["slot"].data_ptr()), C.c_void_p(d["sobs"].data_ptr()), C.c_void_p(moq.data_ptr()),
                                                    C.c_void_p(bd.data_ptr()), C.c_void_p(nm.data_ptr()), None)
    assert rc == 0, m.L.orbm_last_error(m.m)
    torch.cuda.synchronize()
    moq_h, bd_h, nm_h, slot_h, sobs_h = moq.cpu().numpy(), bd.cpu().numpy(), nm.cpu().numpy(), d["slot"].cpu().numpy(), d["sobs"].cpu().numpy()
    return capn, [(int(nm_h[p]), moq_h[p, :len(qry[p]["u"])], bd_h[p, :len(qry[p]["u"])], slot_h[p, :len(cand[p]["k"])],
                   sobs_h[p, :len(cand[p]["k"])]) for p in range(npairs)]


def check_fused(pkg, oracle, capfd, monkeypatch, cand, qry, bounds, sf, fused, nnratio=0.8, th=100, second=True, min_total=1):
    """All three engines against the oracle; engine 2's launch must have taken the fused form iff `fused`."""
    assert len(cand) * ((max(len(q["u"]) for q in qry) + 255) // 256) > 32, "latency mode: the launch would not be fused"
    monkeypatch.setenv("ORBHIP_PRINT_RESOLVE_LDS", "1")
    ref = [oracle_pair(oracle, c, q, bounds, sf, nnratio, th, second) for c, q in zip(cand, qry)]
    for engine in (2, 1, 0):
        m = pkg.ORBmatcher(nnratio, True)
        try:
            m.set_hamming_engine(engine)
            capfd.readouterr()
            capn, got = run_batch_exact(pkg, m, cand, qry, bounds, nnratio, th, second)
            forms = FORM.findall(capfd.readouterr().err)
        finally:
            m.close()
        assert len(forms) == 1, forms
        assert int(forms[0][0]) == capn
        assert forms[0][1] == ("1" if engine == 2 and fused else "0"), (engine, forms)
        if forms[0][1] == "1":
            assert int(forms[0][2]) <= 31 * 1024        # 15 B per keypoint: 31 KB at 2048 keypoints
        for p, (g, r) in enumerate(zip(got, ref)):
            what = "engine %d pair %d (n=%d nq=%d)" % (engine, p, len(cand[p]["k"]), len(qry[p]["u"]))
            assert g[0] == r[0], what
            assert np.array_equal(g[1], r[1]) and np.array_equal(g[2], r[2]), what
            assert np.array_equal(g[3], r[3]) and np.array_equal(g[4], r[4]), what
    assert sum(r[0] for r in ref) >= min_total
    return ref


def random_frame(pkg, rng, n, groups=60, flip=0.03):
    kps = np.zeros(n, dtype=pkg.KP_DTYPE)
    kps["x"] = rng.uniform(1, W - 1, n).astype(np.float32); kps["y"] = rng.uniform(1, H - 1, n).astype(np.float32)
    kps["octave"] = rng.integers(0, 8, n); kps["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    base = rng.integers(0, 256, (groups, 32), dtype=np.uint8)
    desc = base[rng.integers(0, groups, n)].copy()            # few distinct descriptors: many equal distances
    desc[rng.random((n, 32)) < flip] ^= 4
    return kps, desc


def queries_from(kps, desc, rng, nq, radius=5.0e3):
    qi = rng.integers(0, len(kps), nq)
    qd = desc[qi].copy(); qd[rng.random((nq, 32)) < 0.02] ^= 16
    return dict(d=qd, u=kps["x"][qi], v=kps["y"][qi], r=np.full(nq, radius, np.float32), lo=np.full(nq, -1, np.int32),
                hi=np.full(nq, -1, np.int32), flags=np.full(nq, 3, np.uint8))


def occupy(c, rng, frac, obs_frac=0.6):
    occ = rng.random(len(c["slot"])) < frac
    c["slot"][occ] = 1 << 20
    c["sobs"][occ] = rng.random(int(occ.sum())) < obs_frac
    return c


def test_mixed_sizes_occupants_and_ties(pkg, oracle, capfd, monkeypatch):
    """1000- and 2048-keypoint frames and tile tails in one fused launch (table stride 2048), with claimed occupants and ties."""
    rng = np.random.default_rng(71)
    bounds = (0.0, float(W), 0.0, float(H))
    cand, qry = [], []
    for p, n in enumerate((1000, 2048, 1000, 2047, 999, 1001, 2048, 33, 1000, 2048, 1500)):
        kps, desc = random_frame(pkg, rng, n)
        cand.append(occupy(free_frame(kps, desc), rng, (0.0, 0.2, 0.5)[p % 3]))
        qry.append(queries_from(kps, desc, rng, min(900, 4 * n)))
    check_fused(pkg, oracle, capfd, monkeypatch, cand, qry, bounds, SF, True, nnratio=0.7, th=60, min_total=2000)


@pytest.mark.parametrize("n", [2048, 2049])
def test_key32_bound_both_sides(pkg, oracle, capfd, monkeypatch, n):
    """2048 keypoints (the largest fused frame: the largest table slab, every wavefront's compaction share full) and 2049 (64-bit
    keys, never fused), with occupants and ties on both sides."""
    rng = np.random.default_rng(72 + n)
    bounds = (0.0, float(W), 0.0, float(H))
    cand, qry = [], []
    for p in range(9):
        kps, desc = random_frame(pkg, rng, n, groups=40)
        cand.append(occupy(free_frame(kps, desc), rng, (0.0, 0.25, 0.5)[p % 3]))
        qry.append(queries_from(kps, desc, rng, 800))
    check_fused(pkg, oracle, capfd, monkeypatch, cand, qry, bounds, SF, n <= 2048, nnratio=0.8, th=80, min_total=1500)


def test_fused_beside_windowed_pairs(pkg, oracle, synth, capfd, monkeypatch):
    """Extracted frames in one fused launch: open pairs (fused), a pair whose windows are all small (the wide form) and a pair that
    mixes windowed and open queries (the chunked form); the last two read their candidates from the table as well."""
    from conftest import EUROC
    frames, offs = synth.make_stream(5300, 11)
    o = oracle.OracleExtractor(**EUROC)
    ext = [o.extract(f)[1:] for f in frames]
    sf = np.asarray(o.scale_factors, np.float32)
    rng = np.random.default_rng(73)
    bounds = (0.0, float(W), 0.0, float(H))
    cand, qry = [], []
    for p in range(10):
        k1, d1 = ext[p + 1]
        k0, d0 = ext[p]
        c = free_frame(k1, d1)
        if p % 2:
            c = occupy(c, rng, 0.3)
        q = open_queries(k0, d0, (offs[p][0] - offs[p + 1][0], offs[p][1] - offs[p + 1][1]))
        if p == 2:
            q["r"][:] = 15.0                                  # every window small: the wide form
        if p == 5:
            sel = rng.permutation(len(q["r"]))[:200]          # some windowed queries: not fused, chunked form
            q["r"][sel] = 30.0; q["lo"][sel] = 0; q["hi"][sel] = 4
        cand.append(c)
        qry.append(q)
    check_fused(pkg, oracle, capfd, monkeypatch, cand, qry, bounds, sf, True, min_total=1000)
