"""GPU: the keyframe database on the device (orbd_query_reloc, orbd_query_place, orbd_score_batch_device: k_kfdb_mark, k_kfdb_count,
k_kfdb_order, k_kfdb_score, k_kfdb_unmark) against the literal model of tests/kfdb_model.py on the scenes of tests/kfdb_scene.py,
floats by bit pattern and lists by order; the shapes at which the kernels can go wrong; compaction; host threads on one handle; the
resident batch form against single queries; the chain transform -> add_device -> score_batch_device -> SearchByBoW."""
import threading

import numpy as np
import pytest

import kfdb_scene as KS
import voc_scene as VS
from conftest import EUROC

pytestmark = pytest.mark.gpu
T = KS.T


def _batch(db, qids, bows, cap=None, ragged_pad=True):
    """orbd_score_batch_device for the BowVectors `bows` laid out as orbv_transform_batch_device writes them.  Returns one dict per query."""
    import torch
    dev = torch.device("cuda", 0)
    nq = len(bows)
    cap = cap or max(max(len(b[0]) for b in bows), 1)
    ids = np.full((nq, cap), 0xFFFFFFF0, np.uint32)       # what lies past a frame's count is never read as a word
    val = np.full((nq, cap), np.nan, np.float64)
    n = np.zeros(nq, np.int32)
    for q, (i, v) in enumerate(bows):
        ids[q, :len(i)], val[q, :len(i)], n[q] = i, v, len(i)
    d_ids, d_val, d_n = (torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev) for a in (ids, val, n))
    out_cap = max(len(db), 1)
    d_tag = torch.full((nq, out_cap), -1, dtype=torch.int64, device=dev)
    d_score = torch.full((nq, out_cap), -1.0, dtype=torch.float32, device=dev)
    d_cnt = torch.full((nq, 4), -1, dtype=torch.int32, device=dev)
    scratch = torch.full((db.batch_scratch_bytes(nq) // 8 + 1,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)    # not zeroed for it
    db.score_batch_device(qids, d_ids.data_ptr(), d_val.data_ptr(), d_n.data_ptr(), cap, d_tag.data_ptr(), d_score.data_ptr(), out_cap,
                          d_cnt.data_ptr(), scratch.data_ptr(), stream=0)
    torch.cuda.synchronize()
    tag, score, cnt = d_tag.cpu().numpy().view(np.uint64), d_score.cpu().numpy(), d_cnt.cpu().numpy()
    return [dict(tags=tag[q, :cnt[q, 2]].copy(), scores=score[q, :cnt[q, 2]].copy(), max_common=int(cnt[q, 0]), min_common=int(cnt[q, 1]),
                 n_listed=int(cnt[q, 3])) for q in range(nq)]


def _same(a, b, what):
    assert [int(t) for t in a["tags"]] == [int(t) for t in b["tags"]], what
    assert KS.bits(a["scores"], np.float32) == KS.bits(b["scores"], np.float32), what
    assert (a["max_common"], a["min_common"], a["n_listed"]) == (b["max_common"], b["min_common"], b["n_listed"]), what


def _with_batch(db):
    """The batch form asked before every relocalisation step (it changes nothing), three ragged queries a call, held against the model."""
    def before(qid, b):
        half = (b[0][:len(b[0]) // 2], b[1][:len(b[0]) // 2])
        got = _batch(db, [qid, qid, qid + 1], [b, KS.bow([], []), half])
        single_half = _batch(db, [qid + 1], [half])[0]

        def after(scored, mx, mn, nl, what):
            want = dict(tags=[k.tag for _, k in scored], scores=[s for s, _ in scored], max_common=mx, min_common=mn, n_listed=nl)
            _same(got[0], want, what + ": batch form against the model")
            _same(got[1], dict(tags=[], scores=[], max_common=0, min_common=0, n_listed=0), what + ": batch form, empty query")
            _same(got[2], single_half, what + ": batch form, a query at another position")
        return after
    return before


@pytest.mark.parametrize("name", KS.NAMES)
def test_device_forms_equal_model(pkg, name):
    """orbd_query_reloc / orbd_query_place and orbd_accumulate_* on their output against the model's lists, and the batch form."""
    db = pkg.KeyFrameDatabase(KS.N_WORDS, capacity=64, device=0)
    KS.Replay(db=db, host=False, before_reloc=_with_batch(db)).run(KS.SCENES[name](), name)


def _shapes_script():
    rng = np.random.default_rng(21)
    NW = 20000

    def vals(ids):
        v = rng.random(len(ids)) + 0.05
        return KS.bow(ids, v / v.sum())
    big = np.sort(np.concatenate([[0, NW - 1], rng.choice(np.arange(1, NW - 1), 15358, replace=False)]))
    qbig = np.sort(np.concatenate([[0, NW - 1], rng.choice(np.arange(1, NW - 1), 15358, replace=False)]))
    s = [("add", T + 1, 1, vals([0, 31, 32, 63, 64, NW - 1]), [], None),
         ("add", T + 2, 1, KS.bow([], []), [], None),
         ("add", T + 3, 1, vals([31]), [], None)]
    for k, n in enumerate((63, 64, 65, 129)):
        s.append(("add", T + 10 + k, 1, vals(np.arange(100, 100 + n)), [T + 1], None))
    s.append(("add", T + 20, 2, vals(big), [T + 13], None))
    s += [("reloc", 1, vals([0, 31, 32, 63, 64, NW - 1]), 1),                        # the bitmap's dword borders and its last bit
          ("reloc", 2, vals([100, 163, 164, 228]), 1),                              # lanes 0 and 63; the last word of a step and the next one's first
          ("place", 3, [T + 10], vals([100, 163, 164, 228]), 1, 3),
          ("reloc", 4, KS.bow([], []), 1),
          ("reloc", 5, vals(qbig), 2),                                              # 15360 words against 15360
          ("place", 6, [], vals(np.arange(90, 240)), 1, 3),
          ("reloc", 7, vals([NW - 1]), 2)]
    return NW, s


def test_shapes_where_the_kernels_can_go_wrong(pkg):
    NW, script = _shapes_script()
    db = pkg.KeyFrameDatabase(NW, capacity=16, device=0)
    tr = KS.Replay(n_words=NW, db=db, host=False, before_reloc=_with_batch(db)).run(script, "shapes")
    assert T + 1 in [t for _, t in tr[0]["scored"]] and tr[0]["max_common"] == 6
    assert T + 13 in [t for _, t in tr[1]["scored"]] and tr[1]["max_common"] == 4
    assert tr[4]["max_common"] > 10000 and [t for _, t in tr[4]["scored"]] == [T + 20]
    with pytest.raises(ValueError):
        db.query_reloc(9, KS.flat(range(15361), 1e-4))


def test_compaction_on_the_device(pkg):
    """A capacity of 8: adds after erases renumber the slots and move the words; results do not change."""
    db = pkg.KeyFrameDatabase(KS.N_WORDS, capacity=8, device=0)
    KS.Replay(db=db, host=False).run(KS.scene_random(5, n_kf=8, n_steps=120, span=50), "capacity 8")


def test_200_keyframes_a_third_erased(pkg):
    rng = np.random.default_rng(31)
    s = [("add", T + i, 1 + i % 2, KS.rand_bow(rng, int(rng.integers(10, 40)), 0, 300), [T + (i * 7 + k) % 200 for k in range(1, 11)], None)
         for i in range(200)]
    s += [("erase", T + i) for i in range(0, 200, 3)]
    for q in range(6):
        b = KS.rand_bow(rng, 60, 0, 300)
        s.append(("reloc", 10 + q, b, 1) if q % 2 == 0 else ("place", 10 + q, [T + 1, T + 2], b, 1, 3))
    db = pkg.KeyFrameDatabase(KS.N_WORDS, capacity=256, device=0)
    tr = KS.Replay(db=db, host=False, before_reloc=_with_batch(db)).run(s, "200 keyframes")
    assert len(db) == 133 and all(len(t["sharing"]) > 100 for t in tr)


def test_full_capacity(pkg):
    """ORBD_MAX_KEYFRAMES slots: k_kfdb_order sorts 16384 keys in 128 KiB of LDS and every lane walks 16 sorted positions (the other tests
    stay below 1024 slots, one position per lane).  Two words per keyframe, so hundreds pass the gate and the compaction of the list
    crosses many lanes."""
    rng = np.random.default_rng(61)
    n = pkg.MAX_KEYFRAMES
    s = [("add", T + i, 1 + i % 2, KS.rand_bow(rng, 2, 0, 400), [T + (i * 5 + 1) % n, T + (i * 11 + 3) % n], None) for i in range(n)]
    s += [("erase", T + i) for i in range(0, n, 7)]
    s += [("reloc", 1, KS.rand_bow(rng, 40, 0, 400), 1), ("place", 2, [T + 1, T + 9], KS.rand_bow(rng, 40, 0, 400), 2, 3),
          ("add", T + 0, 1, KS.rand_bow(rng, 2, 0, 400), [], None),                 # the slots are full of tombstones: a compaction
          ("reloc", 3, KS.rand_bow(rng, 300, 0, 400), 1)]
    db = pkg.KeyFrameDatabase(KS.N_WORDS, capacity=n, device=0)
    tr = KS.Replay(db=db, host=False, before_reloc=_with_batch(db)).run(s, "full capacity")
    assert len(tr[0]["sharing"]) > 1024 and len(tr[0]["scored"]) > 64 and len(tr[2]["sharing"]) > 8192
    with pytest.raises(ValueError):
        db2 = pkg.KeyFrameDatabase(KS.N_WORDS, capacity=2, device=0)
        db2.add(1, 1, KS.flat([1], 1.0))
        db2.add(2, 1, KS.flat([1], 1.0))
        db2.add(3, 1, KS.flat([1], 1.0))                                            # `capacity` live keyframes


def test_two_queries_in_a_row_leave_a_clean_bitmap(pkg):
    db = pkg.KeyFrameDatabase(KS.N_WORDS, capacity=4, device=0)
    db.add(1, 1, KS.flat(range(0, 64), 1 / 64))
    db.add(2, 1, KS.flat(range(2000, 2064), 1 / 64))
    a = db.query_reloc(1, KS.flat(range(0, 64), 1 / 64))
    b = db.query_reloc(2, KS.flat(range(2000, 2064), 1 / 64))
    c = db.query_reloc(3, KS.flat([4095], 1.0))
    assert list(a["tags"]) == [1] and list(b["tags"]) == [2] and (b["n_listed"], b["max_common"]) == (1, 64)
    assert (c["n_listed"], c["max_common"], len(c["tags"])) == (0, 0, 0)


def test_four_host_threads_on_one_handle(pkg):
    """Tracking, LocalMapping and LoopClosing share one database.  The threads use disjoint word ranges, tags and query ids, so every
    serial order of their calls gives each thread the results of its own script alone: those of the model."""
    db = pkg.KeyFrameDatabase(KS.N_WORDS, capacity=16, device=0)      # 4 threads x at most 4 live keyframes: compactions happen
    errors = []

    def work(k):
        try:
            script = KS.scene_random(50 + k, n_kf=4, n_steps=40, span=60, lo=1000 * k, tag0=T + 1000 * (k + 1), qid0=100000 * (k + 1),
                                     clear_maps=False)
            KS.Replay(db=db, host=False, shared=True).run(script, "thread %d" % k)
        except BaseException as e:   # noqa: B902 - reported by the main thread
            errors.append(e)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[0]


def test_ragged_batch_equals_single_queries(pkg):
    rng = np.random.default_rng(41)
    db = pkg.KeyFrameDatabase(KS.N_WORDS, capacity=64, device=0)
    for i in range(40):
        db.add(T + i, 1, KS.rand_bow(rng, int(rng.integers(1, 130)), 0, 400))
    db.erase(T + 5)
    first = db.query_reloc(7, KS.rand_bow(rng, 100, 0, 400))            # marks keyframes with id 7: the batch must see it
    assert first["n_listed"] > 10
    sizes = (0, 1, 63, 64, 65, 200, 0, 129, 300, 17)
    bows = [KS.rand_bow(rng, n, 0, 400) if n else KS.bow([], []) for n in sizes]
    qids = [7 if q in (3, 8) else 100 + q for q in range(len(sizes))]
    got = _batch(db, qids, bows, cap=333)
    assert sum(g["n_listed"] for g in got) > 100
    for q, (b, g) in enumerate(zip(bows, got)):
        if qids[q] == 7:
            assert g["n_listed"] < 39 - first["n_listed"] + 1
        else:
            _same(g, db.query_reloc(qids[q], b), "query %d" % q)        # single queries of fresh ids see what the batch saw


def test_chain_from_transform_to_search_by_bow(pkg, oracle, synth):
    """orbv_transform_batch_device -> add_device for three frames -> score_batch_device for the fourth, nothing downloaded in between;
    expected values from the model on transform_host's vectors; then the scored keyframes as the candidates of one SearchByBoW call."""
    import torch
    import kfdb_model as KM
    dev = torch.device("cuda", 0)
    frames, _ = synth.make_stream(3800, 4, 240, 376)
    ex = pkg.ORBextractor(**EUROC)
    kd = [ex(f, None, (0, 1000))[1:] for f in frames]
    voc = VS.vocabulary(pkg, "regular", 0, 0, device=0)
    levelsup, B = 2, 4
    cap = max(len(d) for _, d in kd) + 3
    desc, cnt = np.zeros((B, cap, 32), np.uint8), np.zeros(B, np.int32)
    for p, (_, d) in enumerate(kd):
        desc[p, :len(d)], cnt[p] = d, len(d)
    d_desc, d_n = torch.from_numpy(desc).to(dev), torch.from_numpy(cnt).to(dev)
    z = lambda shape, dt: torch.full(shape, -3, dtype=dt, device=dev)
    o = dict(bow_id=z((B, cap), torch.int32), bow_val=z((B, cap), torch.float64), n_bow=z((B,), torch.int32), fv_node_id=z((B, cap), torch.int32),
             fv_start=z((B, cap + 1), torch.int32), fv_idx=z((B, cap), torch.int32), n_fv=z((B,), torch.int32))
    scratch = torch.zeros(pkg.ORBVocabulary.batch_scratch_bytes(B, cap), dtype=torch.uint8, device=dev)
    voc.transform_batch_device(d_desc.data_ptr(), B, cap, d_n.data_ptr(), 1, levelsup, o["bow_id"].data_ptr(), o["bow_val"].data_ptr(),
                               o["n_bow"].data_ptr(), o["fv_node_id"].data_ptr(), o["fv_start"].data_ptr(), o["fv_idx"].data_ptr(),
                               o["n_fv"].data_ptr(), scratch.data_ptr(), stream=0)
    db = pkg.KeyFrameDatabase.for_vocabulary(voc, capacity=8, device=0)
    for p in range(3):
        db.add_device(T + p, 1, o["bow_id"].data_ptr(), o["bow_val"].data_ptr(), o["n_bow"].data_ptr(), cap, p, stream=0)
    out_cap = 3
    d_tag, d_score, d_cnt = z((1, out_cap), torch.int64), z((1, out_cap), torch.float32), z((1, 4), torch.int32)
    ks = torch.zeros(db.batch_scratch_bytes(1) // 8 + 1, dtype=torch.int64, device=dev)
    db.score_batch_device([55], o["bow_id"].data_ptr() + 3 * cap * 4, o["bow_val"].data_ptr() + 3 * cap * 8, o["n_bow"].data_ptr() + 3 * 4, cap,
                          d_tag.data_ptr(), d_score.data_ptr(), out_cap, d_cnt.data_ptr(), ks.data_ptr(), stream=0)
    torch.cuda.synchronize()
    c = d_cnt.cpu().numpy()[0]
    got = dict(tags=d_tag.cpu().numpy().view(np.uint64)[0, :c[2]], scores=d_score.cpu().numpy()[0, :c[2]], max_common=int(c[0]),
               min_common=int(c[1]), n_listed=int(c[3]))
    th = [voc.transform_host(d, levelsup) for _, d in kd]
    model = KM.Database(voc.n_words)
    for p in range(3):
        model.add(KM.KF(T + p, 1, (th[p]["bow_id"], th[p]["bow_val"])))
    scored, mx, mn, nl = model.reloc_scored(55, [(int(i), float(v)) for i, v in zip(th[3]["bow_id"], th[3]["bow_val"])])
    _same(got, dict(tags=[k.tag for _, k in scored], scores=[s for s, _ in scored], max_common=mx, min_common=mn, n_listed=nl), "chain")
    assert len(scored) >= 1 and mx > 20
    with pytest.raises(ValueError):      # the handle holds entries without a host copy
        db.query_reloc_host(56, th[3])
    _same(db.query_reloc(56, th[3]), dict(got, tags=got["tags"]), "the single query on device-added entries")
    # the winners as the candidates of one SearchByBoW call
    sf = oracle.OracleExtractor(**EUROC).scale_factors
    sigma2 = (sf * sf).astype(np.float32)
    tr = [voc.transform(d, levelsup) for _, d in kd]

    def view(p, **kw):
        V = pkg.KeyFrameView(kd[p][0], kd[p][1], {}, sf, sigma2, **kw)
        V.node_id, V.node_start, V.node_idx = tr[p]["fv_node_id"], tr[p]["fv_start"], (tr[p]["fv_idx"] if len(tr[p]["fv_idx"]) else np.zeros(1, np.int32))
        return V
    winners = [int(t) - T for t in got["tags"]]
    rng = np.random.default_rng(8)
    kfs = [view(p, has_mappoint=(rng.random(len(kd[p][0])) < 0.8).astype(np.uint8)) for p in winners]
    m = pkg.ORBmatcher(0.75, True)
    try:
        nm, rows = m.SearchByBoWCandidates(kfs, view(3))
        for j, kf in enumerate(kfs):
            n1, row = m.SearchByBoW(kf, view(3))
            assert nm[j] == n1 and np.array_equal(rows[j], row)
        assert nm.max() > 20
    finally:
        m.close()
