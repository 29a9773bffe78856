"""GPU: k_octree's code form (column / row tables, leaf histogram, count pyramid, rounds on the nodes alone, leaf map, hand-over to the
per-key rounds) against the oracle, key for key and in output order, on the cases of tests/octree_codes_cases.py (what each of them
reaches is asserted on the CPU by tests/test_octree_codes_model.py).  Every case runs as a 1-frame call (1024-thread workgroups) and
inside a 5-frame call (256-thread workgroups), with the tables and - through ORBHIP_OCTREE_TABLE_LIMIT, a bound for tests - in the
per-key form that a configuration takes whose tables do not fit; the library's ORBHIP_PRINT_EXTRACT_FORMS line names the form."""
import re

import numpy as np
import pytest

import octree_codes_cases as K
from test_gpu_batch_layouts import pack

pytestmark = pytest.mark.gpu

ROUNDS = re.compile(r"orbhip: extract nframes (\d+) .* octree (1024|256)/\S+ .* rounds (codes|keys) octLds (\d+)")
_ref = {}
_lds = {}


def reference(oracle, name, img, c):
    if name not in _ref:
        o = oracle.OracleExtractor(**c)
        mono, kps, desc = o.extract(img, (0, 1000))
        _ref[name] = dict(out=(mono, kps.tobytes(), desc.tobytes()), levels=K.level_reference(oracle, img, c))
    return _ref[name]


def batch_of(img, n):
    """The case's frame in the middle of its mirror images: the other workgroups of the launch have work of their own."""
    if n == 1:
        return [img], 0
    return [np.ascontiguousarray(f) for f in (img[:, ::-1], img[::-1], img, img[::-1, ::-1], img[:, ::-1])], 2


NAMES = ["flat", "one blob", "two blobs", "patch inside a cell", "patch across the first split lines", "patch across a root's split lines",
         "small N", "N above the keys", "one root", "two roots", "three roots", "empty root", "checkerboard", "squares", "noise 752x480"]


@pytest.mark.parametrize("form", ["codes", "keys"])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("name", NAMES)
def test_case(pkg, oracle, synth, capfd, monkeypatch, name, n, form):
    _, img, c = next(x for x in K.cases(synth) if x[0] == name)
    ref = reference(oracle, name, img, c)
    monkeypatch.setenv("ORBHIP_PRINT_EXTRACT_FORMS", "1")
    if form == "keys":
        monkeypatch.setenv("ORBHIP_OCTREE_TABLE_LIMIT", "0")
    else:
        monkeypatch.delenv("ORBHIP_OCTREE_TABLE_LIMIT", raising=False)
    frames, k = batch_of(img, n)
    H, W = img.shape
    stride = (W + 3) & ~3
    fs = H * stride
    e = pkg.ORBextractor(**c)
    try:
        cap = e.configure(H, W, n)
        import torch
        d_buf = torch.from_numpy(pack(frames, 0, stride, fs)).cuda()
        d_kps = torch.zeros((n, cap, 7), dtype=torch.int32, device="cuda")
        d_desc = torch.zeros((n, cap, 32), dtype=torch.uint8, device="cuda")
        d_cnt = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        capfd.readouterr()
        e.extract_batch_device(d_buf.data_ptr(), H, W, stride, fs, n, d_kps.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(), cap, (0, 1000),
                               stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        m = ROUNDS.findall(capfd.readouterr().err)
        assert len(m) == 1, m
        assert m[0][:3] == (str(n), "1024" if n == 1 else "256", form)
        _lds.setdefault((name, n), {})[form] = int(m[0][3])
        for l, lv in enumerate(ref["levels"]):
            assert np.array_equal(e.level_candidates(l, frame=k), lv["cand"]), "FAST candidates level %d" % l
            assert np.array_equal(e.level_keypoints(l, frame=k), lv["oct"]), "octree level %d" % l
        cnt = d_cnt.cpu().numpy()
        got = (int(cnt[k, 1]), d_kps[k, :int(cnt[k, 0])].cpu().numpy().tobytes(), d_desc[k, :int(cnt[k, 0])].cpu().numpy().tobytes())
        assert got == ref["out"], "keypoints and descriptors"
    finally:
        e.close()
    both = _lds[(name, n)]
    if len(both) == 2:
        # the tables take the place of the child counts; a configuration with few nodes gets a larger head region, a small one
        assert both["keys"] <= both["codes"] <= max(both["keys"], 32 * 1024)
        if c["nfeatures"] >= 1000:
            assert both["codes"] == both["keys"], "the tables must not change k_octree's LDS size where they fit beside the nodes"


@pytest.mark.parametrize("conf", ["euroc", "tumvi"])
def test_bench_configurations_keep_their_lds(pkg, synth, capfd, monkeypatch, conf):
    """At the bench's two configurations the code form is taken and k_octree's dynamic LDS is what the per-key form has."""
    from conftest import EUROC, TUMVI
    H, W, c = (480, 752, EUROC) if conf == "euroc" else (512, 512, TUMVI)
    monkeypatch.setenv("ORBHIP_PRINT_EXTRACT_FORMS", "1")
    img = synth.make_frame(5, H, W)
    seen = {}
    for form in ("codes", "keys"):
        if form == "keys":
            monkeypatch.setenv("ORBHIP_OCTREE_TABLE_LIMIT", "0")
        e = pkg.ORBextractor(**c)
        try:
            capfd.readouterr()
            out = e(img, None, (0, 1000))
            m = ROUNDS.findall(capfd.readouterr().err)
            assert m and all(x[2] == form for x in m), m
            seen[form] = (int(m[0][3]), out[0], out[1].tobytes(), out[2].tobytes())
        finally:
            e.close()
    assert seen["codes"] == seen["keys"]
