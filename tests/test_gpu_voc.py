"""GPU: the vocabulary transform behind Frame::ComputeBoW / KeyFrame::ComputeBoW on the device (orbv_transform,
orbv_transform_batch_device: k_voc_descend + k_voc_collect) against the literal model of tests/voc_model.py on the scenes of
tests/voc_scene.py, doubles by bit pattern; the batch form against the per-frame entry; the produced FeatureVector passed unchanged into
SearchByBoW and SearchForTriangulation; several host threads on one handle."""
import threading

import numpy as np
import pytest

import voc_model as VM
import voc_scene as VS
from conftest import EUROC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", VS.NAMES)
def test_device_form_equals_model(pkg, name):
    S = VS.scene(name)
    for weighting in VS.WEIGHTINGS:
        for scoring in VS.SCORINGS:
            voc, model = VS.vocabulary(pkg, name, weighting, scoring, device=0), VS.model(name, weighting, scoring)
            for levelsup in VS.levelsups(S["L"]):
                for n in VS.N_VALUES:
                    what = "%s weighting %d scoring %d levelsup %d n %d" % (name, weighting, scoring, levelsup, n)
                    VS.check_against_model(voc, model, S["queries"][:n], levelsup, what, transform="transform")


def test_largest_frame_and_handle_reuse(pkg):
    """n = ORBM_MAX_KEYPOINTS (16384 sort keys, 128 KiB of LDS) on the small tree, one more is refused; then the same handle on
    smaller and larger frames in turn: the workspace of a call says nothing about the next."""
    voc, model = VS.vocabulary(pkg, "flat", 0, 0, device=0), VS.model("flat", 0, 0)
    desc = VS.flat_big(15361)
    VS.check_against_model(voc, model, desc[:15360], 1, "n = 15360", transform="transform")
    with pytest.raises(ValueError):
        voc.transform(desc, 1)
    for n in (3, 8200, 0, 1, 4097, 64, 15360, 5):
        VS.check_against_model(voc, model, desc[:n], 0, "reuse n = %d" % n, transform="transform")


def _batch(pkg, voc, torch, d_desc, nframes, cap, d_n, n_stride, levelsup, descend_form=None):
    dev = d_desc.device
    z = lambda shape, dt: torch.full(shape, -3, dtype=dt, device=dev)
    out = dict(word=z((nframes, cap), torch.int32), node=z((nframes, cap), torch.int32), bow_id=z((nframes, cap), torch.int32),
               bow_val=z((nframes, cap), torch.float64), n_bow=z((nframes,), torch.int32), fv_node_id=z((nframes, cap), torch.int32),
               fv_start=z((nframes, cap + 1), torch.int32), fv_idx=z((nframes, cap), torch.int32), n_fv=z((nframes,), torch.int32))
    scratch = torch.zeros(max(pkg.ORBVocabulary.batch_scratch_bytes(nframes, cap), 4), dtype=torch.uint8, device=dev)
    voc.transform_batch_device(d_desc.data_ptr(), nframes, cap, d_n.data_ptr(), n_stride, levelsup, out["bow_id"].data_ptr(),
                               out["bow_val"].data_ptr(), out["n_bow"].data_ptr(), out["fv_node_id"].data_ptr(), out["fv_start"].data_ptr(),
                               out["fv_idx"].data_ptr(), out["n_fv"].data_ptr(), scratch.data_ptr(), d_word=out["word"].data_ptr(),
                               d_node=out["node"].data_ptr(), stream=0, descend_form=descend_form)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _frame_of(out, p, n):
    nb, nf = int(out["n_bow"][p]), int(out["n_fv"][p])
    start = out["fv_start"][p, :nf + 1]
    u = lambda a: a.view(np.uint32)
    return dict(word=u(out["word"][p, :n]), node=u(out["node"][p, :n]), bow_id=u(out["bow_id"][p, :nb]), bow_val=out["bow_val"][p, :nb],
                fv_node_id=u(out["fv_node_id"][p, :nf]), fv_start=start, fv_idx=out["fv_idx"][p, :int(start[nf])])


@pytest.mark.parametrize("name,weighting,scoring,levelsup", [("regular", 0, 0, 1), ("wide", 1, 5, 1), ("deep", 2, 0, 4)])
def test_batch_form_equals_per_frame_entry(pkg, name, weighting, scoring, levelsup):
    """Ragged live counts, among them 0, 1, the capacity, one above it (taken as the capacity) and a negative one (taken as 0);
    both descent kernels."""
    import torch
    dev = torch.device("cuda", 0)
    S = VS.scene(name)
    voc = VS.vocabulary(pkg, name, weighting, scoring, device=0)
    cap = 300
    counts = [0, 1, 65, 300, 257, 400, -5, 64]
    live = [min(max(c, 0), cap) for c in counts]
    B = len(counts)
    rng = np.random.default_rng(3)
    desc = S["queries"][rng.integers(0, 1000, (B, cap))]
    d_desc = torch.from_numpy(np.ascontiguousarray(desc)).to(dev)
    d_n = torch.tensor(counts, dtype=torch.int32, device=dev)
    want = [voc.transform(desc[p, :live[p]], levelsup) for p in range(B)]
    for form in (None, 0, 1):
        out = _batch(pkg, voc, torch, d_desc, B, cap, d_n, 1, levelsup, descend_form=form)
        for p in range(B):
            VM.same(_frame_of(out, p, live[p]), want[p], "form %s frame %d" % (form, p))


def test_batch_form_on_the_extractor_counts(pkg, synth):
    """orbx_extract_batch_device -> orbv_transform_batch_device with nothing between them: the extractor's descriptors where they lie
    and its d_counts [nframes][2] as the live counts (n_stride = 2)."""
    import torch
    B, H, W = 3, 240, 376
    frames, _ = synth.make_stream(77, B, H, W)
    dev = torch.device("cuda", 0)
    ex = pkg.ORBextractor(**EUROC)
    cap = ex.configure(H, W, B)
    d_img = torch.from_numpy(frames).to(dev)
    d_kps = torch.zeros((B, cap, 7), dtype=torch.float32, device=dev)
    d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    ex.extract_batch_device(d_img.data_ptr(), H, W, W, H * W, B, d_kps.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(), cap, (0, 1000), stream=0)
    voc = VS.vocabulary(pkg, "regular", 0, 0, device=0)
    out = _batch(pkg, voc, torch, d_desc, B, cap, d_cnt, 2, 1)
    cnt, desc = d_cnt.cpu().numpy(), d_desc.cpu().numpy()
    model = VS.model("regular", 0, 0)
    for p in range(B):
        n = int(cnt[p, 0])
        assert n > 100
        VM.same(_frame_of(out, p, n), voc.transform(desc[p, :n], 1), "frame %d" % p)
    VM.same(_frame_of(out, 0, int(cnt[0, 0])), model.transform(desc[0, :int(cnt[0, 0])], 1), "frame 0 against the model")


def test_chain_into_the_searches(pkg, oracle, synth):
    """Extracted descriptors -> transform -> the produced FeatureVector, unchanged, into SearchByBoW and SearchForTriangulation; the
    oracle's members get the MODEL's FeatureVector of the same descriptors."""
    frames, offs = synth.make_stream(3800, 2)
    ex = pkg.ORBextractor(**EUROC)
    (k0, d0), (k1, d1) = [ex(f, None, (0, 1000))[1:] for f in frames]
    sf = oracle.OracleExtractor(**EUROC).scale_factors
    sigma2 = (sf * sf).astype(np.float32)
    voc, model = VS.vocabulary(pkg, "regular", 0, 0, device=0), VS.model("regular", 0, 0)
    levelsup = 2                                                    # nodes of level 1: ten of them, as with ORBvoc's L = 6, levelsup = 4 a coarse level
    t0, t1 = voc.transform(d0, levelsup), voc.transform(d1, levelsup)
    m0, m1 = model.transform(d0, levelsup), model.transform(d1, levelsup)
    fv_of = pkg.ORBVocabulary.feat_vec
    rng = np.random.default_rng(8)
    mp0 = (rng.random(len(k0)) < 0.8).astype(np.uint8)

    def view(k, d, t, **kw):
        """KeyFrameView whose three FeatureVector arrays ARE the transform's outputs."""
        V = pkg.KeyFrameView(k, d, {}, sf, sigma2, **kw)
        V.node_id, V.node_start, V.node_idx = t["fv_node_id"], t["fv_start"], (t["fv_idx"] if len(t["fv_idx"]) else np.zeros(1, np.int32))
        return V
    m = pkg.ORBmatcher(0.7, True)
    try:
        n_gpu, m_gpu = m.SearchByBoW(view(k0, d0, t0, has_mappoint=mp0), view(k1, d1, t1))
        n_ref, m_ref = oracle.search_by_bow(oracle.OracleKeyFrame(k0, d0, fv_of(m0), sf, sigma2, has_mp=mp0),
                                            oracle.OracleKeyFrame(k1, d1, fv_of(m1), sf, sigma2), 0.7, True)
        assert n_gpu == n_ref and n_ref > 100 and np.array_equal(m_gpu, m_ref)
    finally:
        m.close()
    cam = np.array([458.654, 457.296, 367.215, 248.375], np.float32)
    z = np.float32(5.0)
    dx, dy = offs[0][0] - offs[1][0], offs[0][1] - offs[1][1]
    R1w, t1w, Cw1 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
    R2w = np.eye(3, dtype=np.float32)
    t2w = np.array([dx * z / cam[0], dy * z / cam[1], 0.02], np.float32)
    none0, none1 = np.zeros(len(k0), np.uint8), np.zeros(len(k1), np.uint8)
    m = pkg.ORBmatcher(0.6, False)
    try:
        n_gpu, pairs_gpu = m.SearchForTriangulation(view(k0, d0, t0, has_mappoint=none0), view(k1, d1, t1, has_mappoint=none1), R1w, t1w, R2w, t2w,
                                                    Cw1, cam, cam)
        n_ref, pairs_ref = oracle.search_for_triangulation(oracle.OracleKeyFrame(k0, d0, fv_of(m0), sf, sigma2, has_mp=none0),
                                                           oracle.OracleKeyFrame(k1, d1, fv_of(m1), sf, sigma2, has_mp=none1), R1w, t1w, R2w, t2w,
                                                           Cw1, cam, cam, only_stereo=False, coarse=False, check_ori=False)
        assert n_gpu == n_ref and n_ref > 100 and np.array_equal(pairs_gpu, pairs_ref)
    finally:
        m.close()


def test_four_host_threads_on_one_handle(pkg):
    """Tracking and LocalMapping call ComputeBoW on one vocabulary at the same time: each call takes its stream and workspace from the
    handle's pool, the tables are only read."""
    S = VS.scene("regular")
    voc = VS.vocabulary(pkg, "regular", 0, 0, device=0)
    sizes = (1000, 257, 64, 5, 999, 0, 65)
    want = {n: voc.transform_host(S["queries"][:n], 1) for n in sizes}
    errors = []

    def work(k):
        try:
            for r in range(12):
                n = sizes[(k + r) % len(sizes)]
                VM.same(voc.transform(S["queries"][:n], 1), want[n], "thread %d round %d" % (k, r))
        except BaseException as e:   # noqa: B902 - reported by the main thread
            errors.append(e)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[0]
