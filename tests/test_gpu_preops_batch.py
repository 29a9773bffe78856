"""orbx_clahe_batch_device and orbx_remap_linear_batch_device on resident batches: every frame against oracle.clahe /
oracle.remap_linear (np.array_equal), at tight, unaligned and padded layouts, in place, as a batch of one against the per-image call,
chained into orbx_extract_batch_device, and the refusals next to live buffers.  Destinations are pre-filled with 0xA5: every byte
outside the frames' rows x cols must still be 0xA5 afterwards."""
import ctypes as C

import numpy as np
import pytest

from conftest import EUROC

pytestmark = pytest.mark.gpu

FILL = 0xA5


def rectify_maps(H, W, seed=0):
    """A plausible rectification map pair: small rotation + radial term, reaching outside the source near the corners (the recipe of
    tests/test_preops.py)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    cx, cy, f = W / 2 + rng.uniform(-5, 5), H / 2 + rng.uniform(-5, 5), 0.6 * W
    a = np.deg2rad(rng.uniform(-2, 2))
    xn, yn = (xs - cx) / f, (ys - cy) / f
    xr, yr = np.cos(a) * xn - np.sin(a) * yn, np.sin(a) * xn + np.cos(a) * yn
    r2 = xr * xr + yr * yr
    d = 1 + 0.28 * r2 + 0.07 * r2 * r2
    return (xr * d * f + cx).astype(np.float32), (yr * d * f + cy).astype(np.float32)


def extent(n, H, W, stride, fs):
    return (n - 1) * fs + (H - 1) * stride + W


def pack(frames, stride, fs, lead=0, tail=0):
    """The frames at lead + k * fs with `stride` bytes per row; every other byte, `lead` before and `tail` behind included, is 0xA5."""
    H, W = frames[0].shape
    buf = np.full(lead + extent(len(frames), H, W, stride, fs) + tail, FILL, np.uint8)
    for k, f in enumerate(frames):
        for y in range(H):
            o = lead + k * fs + y * stride
            buf[o:o + W] = f[y]
    return buf


def unpack(buf, n, H, W, stride, fs, lead=0):
    """(frames, mask of the bytes that belong to no frame)."""
    outside = np.ones(len(buf), bool)
    frames = []
    for k in range(n):
        rows = []
        for y in range(H):
            o = lead + k * fs + y * stride
            rows.append(buf[o:o + W])
            outside[o:o + W] = False
        frames.append(np.stack(rows))
    return frames, outside


def align(x, a):
    return (x + a - 1) // a * a


# ---- CLAHE -------------------------------------------------------------------------------------------------------------------------
CLAHE_CASES = [(67, 101, (8, 8), 3.0), (64, 64, (16, 16), 40.0), (300, 333, (5, 7), 2.0), (96, 128, (8, 8), 0.0), (512, 512, (8, 8), 3.0),
               (480, 752, (8, 8), 3.0)]
_clahe_cache = {}


def clahe_frames(synth, oracle, H, W, tiles, clip):
    """The frames of one case and their oracle results, computed once: frame 1 constant 77; random, a smooth ramp plus noise (small
    shapes), a synth.make_frame image (the two real sizes)."""
    key = (H, W, tiles, clip)
    if key not in _clahe_cache:
        rng = np.random.default_rng([H, W])
        const = np.full((H, W), 77, np.uint8)
        if H >= 480:
            frames = [synth.make_frame(4300 + H, H, W), const]
        else:
            ramp = (np.linspace(20, 120, W)[None, :] + 30 * np.sin(np.arange(H) / 5.0)[:, None] + rng.normal(0, 6, (H, W))).clip(0, 255).astype(np.uint8)
            frames = [rng.integers(0, 256, (H, W), dtype=np.uint8), const, ramp]
        _clahe_cache[key] = (frames, [oracle.clahe(f, clip, tiles) for f in frames])
    return _clahe_cache[key]


def run_clahe(pkg, frames, tiles, clip, sstride, sfs, dstride=None, dfs=None, lead=0):
    """One batch call; dstride None = in place.  Returns (result frames, every byte outside them still 0xA5, source buffer unchanged)."""
    import torch
    n, (H, W) = len(frames), frames[0].shape
    src = pack(frames, sstride, sfs, lead, 7)
    d_src = torch.from_numpy(src).cuda()
    d_lut = torch.zeros(n * tiles[0] * tiles[1] * 256, dtype=torch.uint8, device="cuda")
    if dstride is None:
        d_dst, dstride, dfs, dlead = d_src, sstride, sfs, lead
    else:
        dlead = 64
        d_dst = torch.full((dlead + extent(n, H, W, dstride, dfs) + 64,), FILL, dtype=torch.uint8, device="cuda")
    rc = pkg.clahe_batch_device(n, d_src.data_ptr() + lead, H, W, sstride, sfs, clip, tiles[0], tiles[1], d_lut.data_ptr(), d_dst.data_ptr() + dlead,
                                dstride, dfs, stream=torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    out = d_dst.cpu().numpy()
    got, outside = unpack(out, n, H, W, dstride, dfs, dlead)
    return got, bool((out[outside] == FILL).all()), d_dst is d_src or np.array_equal(d_src.cpu().numpy(), src)


@pytest.mark.parametrize("H,W,tiles,clip", CLAHE_CASES, ids=["%dx%d" % c[:2] for c in CLAHE_CASES])
def test_clahe_batch_layouts(pkg, oracle, synth, H, W, tiles, clip):
    frames, ref = clahe_frames(synth, oracle, H, W, tiles, clip)
    pad_d = align(W, 64) + 64
    layouts = [("tight", W, H * W, W, H * W, 0),
               ("unaligned source, padded destination", W + 3, H * (W + 3) + 5, pad_d, H * pad_d + 128, 0),
               ("source base + 1", W, H * W, pad_d, H * pad_d, 1),
               ("in place, tight", W, H * W, None, None, 0),
               ("in place, unaligned", W + 3, H * (W + 3) + 5, None, None, 0),
               ("in place, padded", pad_d, H * pad_d + 64, None, None, 64)]
    for name, ss, sfs, ds, dfs, lead in layouts:
        got, pad_ok, src_ok = run_clahe(pkg, frames, tiles, clip, ss, sfs, ds, dfs, lead)
        for k in range(len(frames)):
            assert np.array_equal(got[k], ref[k]), "%s: frame %d differs from the oracle" % (name, k)
        assert pad_ok, "%s: a byte outside the frames was written" % name
        assert src_ok, "%s: the source buffer was written" % name


@pytest.mark.parametrize("H,W,tiles,clip", [c for c in CLAHE_CASES if c[0] < 480], ids=["%dx%d" % c[:2] for c in CLAHE_CASES if c[0] < 480])
def test_clahe_batch_of_one_equals_per_image_call(pkg, oracle, synth, H, W, tiles, clip):
    import torch
    frames, ref = clahe_frames(synth, oracle, H, W, tiles, clip)
    L = pkg.load()
    stride = W + 3
    d_src = torch.from_numpy(pack(frames[:1], stride, 0)).cuda()
    d_lut = torch.zeros(tiles[0] * tiles[1] * 256, dtype=torch.uint8, device="cuda")
    d_a = torch.full((H * stride,), FILL, dtype=torch.uint8, device="cuda")
    d_b = torch.full((H * stride,), FILL, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert pkg.clahe_batch_device(1, d_src.data_ptr(), H, W, stride, 0, clip, tiles[0], tiles[1], d_lut.data_ptr(), d_a.data_ptr(), stride, 0, stream=s) == 0
    lut_a = d_lut.cpu().numpy()
    d_lut.zero_()
    assert L.orbx_clahe_device(C.c_void_p(d_src.data_ptr()), H, W, C.c_size_t(stride), C.c_double(clip), tiles[0], tiles[1], C.c_void_p(d_lut.data_ptr()),
                               C.c_void_p(d_b.data_ptr()), C.c_size_t(stride), C.c_void_p(s)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(lut_a, d_lut.cpu().numpy())            # the tables themselves
    assert np.array_equal(d_a.cpu().numpy(), d_b.cpu().numpy())  # padding included
    assert np.array_equal(unpack(d_a.cpu().numpy(), 1, H, W, stride, 0)[0][0], ref[0])


# ---- remap -------------------------------------------------------------------------------------------------------------------------
def run_remap(pkg, frames, mx, my, sstride, sfs, dstride, dfs, mstride=None):
    import torch
    n, (SH, SW), (H, W) = len(frames), frames[0].shape, mx.shape
    mstride = mstride or W
    mxp, myp = np.full((H, mstride), np.nan, np.float32), np.full((H, mstride), np.nan, np.float32)
    mxp[:, :W], myp[:, :W] = mx, my
    src = pack(frames, sstride, sfs, 0, 3)
    d_src, d_mx, d_my = torch.from_numpy(src).cuda(), torch.from_numpy(mxp).cuda(), torch.from_numpy(myp).cuda()
    d_dst = torch.full((32 + extent(n, H, W, dstride, dfs) + 32,), FILL, dtype=torch.uint8, device="cuda")
    rc = pkg.remap_linear_batch_device(n, d_src.data_ptr(), SH, SW, sstride, sfs, d_mx.data_ptr(), d_my.data_ptr(), mstride, H, W, d_dst.data_ptr() + 32,
                                       dstride, dfs, stream=torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    out = d_dst.cpu().numpy()
    got, outside = unpack(out, n, H, W, dstride, dfs, 32)
    assert (out[outside] == FILL).all(), "a byte outside the frames was written"
    assert np.array_equal(d_src.cpu().numpy(), src), "the source buffer was written"
    return got


@pytest.fixture(scope="module")
def small(oracle):
    """Frames of 120 x 188, more than two chunks of them, and their references for the two map pairs."""
    rng = np.random.default_rng(5)
    SH, SW = 120, 188
    mx, my = rectify_maps(SH, SW, 1)
    mx2, my2 = rectify_maps(100, 130, 4)
    mx2, my2 = mx2 * 4, my2 * 4
    mx2[3, 4] = np.nan; my2[5, 6] = np.inf; mx2[7, 8] = -1e30; my2[9, 9] = 3e9
    return dict(rng=rng, SH=SH, SW=SW, maps=(mx, my), maps2=(mx2, my2), frames=[], ref={}, oracle=oracle)


def small_frames(S, n):
    while len(S["frames"]) < n:
        S["frames"].append(S["rng"].integers(1, 256, (S["SH"], S["SW"]), dtype=np.uint8))
    return S["frames"][:n]


def small_ref(S, which, k):
    if (which, k) not in S["ref"]:
        S["ref"][which, k] = S["oracle"].remap_linear(S["frames"][k], *S[which])
    return S["ref"][which, k]


def test_remap_batch_rectification_maps(pkg, small):
    frames = small_frames(small, 3)
    SH, SW = small["SH"], small["SW"]
    mx, my = small["maps"]
    ref = [small_ref(small, "maps", k) for k in range(3)]
    assert all((r == 0).any() and (r != 0).any() for r in ref)       # zero border pixels and non-zero ones
    assert not np.array_equal(ref[0], ref[1]) and not np.array_equal(ref[1], ref[2])
    pad_s, pad_d = SW + 3, align(SW, 64) + 64
    for name, ss, sfs, ds, dfs, ms in [("tight", SW, SH * SW, SW, SH * SW, None), ("map stride", SW, SH * SW, SW, SH * SW, SW + 5),
                                       ("padded", pad_s, SH * pad_s + 5, pad_d, SH * pad_d + 77, SW + 5)]:
        got = run_remap(pkg, frames, mx, my, ss, sfs, ds, dfs, ms)
        for k in range(3):
            assert np.array_equal(got[k], ref[k]), "%s: frame %d differs from the oracle" % (name, k)


def test_remap_batch_other_output_size_and_non_finite_entries(pkg, small):
    frames = small_frames(small, 3)
    mx2, my2 = small["maps2"]
    got = run_remap(pkg, frames, mx2, my2, small["SW"] + 1, small["SH"] * (small["SW"] + 1), 130 + 2, 100 * 132 + 3, 130 + 5)
    for k in range(3):
        assert np.array_equal(got[k], small_ref(small, "maps2", k))


def test_remap_batch_identity_returns_the_sources(pkg, small):
    frames = small_frames(small, 3)
    SH, SW = small["SH"], small["SW"]
    ys, xs = np.mgrid[0:SH, 0:SW].astype(np.float32)
    got = run_remap(pkg, frames, xs, ys, SW, SH * SW, SW, SH * SW)
    for k in range(3):
        assert np.array_equal(got[k], frames[k])


@pytest.mark.parametrize("SW", [1, 2, 3])
def test_remap_batch_narrow_sources(pkg, oracle, SW):
    """Sources of one, two and three columns: the kernel reads the two taps of a row as one column pair, which a one-column source does
    not have and which in a two-column source is always the same pair.  The map sweeps from two pixels left of the source to two
    pixels right of it and from above it to below it in steps of 1/8 pixel."""
    rng = np.random.default_rng(SW)
    SH, H, W = 9, 13 * 8, (SW + 4) * 8
    frames = [rng.integers(1, 256, (SH, SW), dtype=np.uint8) for _ in range(3)]
    mx = np.broadcast_to((np.arange(W, dtype=np.float32) / 8 - 2)[None, :], (H, W)).copy()
    my = np.broadcast_to((np.arange(H, dtype=np.float32) / 8 - 2)[:, None], (H, W)).copy()
    ref = [oracle.remap_linear(f, mx, my) for f in frames]
    assert all((r == 0).any() and (r != 0).any() for r in ref)
    got = run_remap(pkg, frames, mx, my, SW, SH * SW, W + 3, H * (W + 3) + 1)
    for k in range(3):
        assert np.array_equal(got[k], ref[k])


def test_remap_batch_frame_chunks(pkg, small):
    """Batches below one chunk of frames, one more than a chunk, and two chunks plus a rest."""
    ch = pkg.REMAP_FRAME_CHUNK
    SH, SW = small["SH"], small["SW"]
    mx, my = small["maps"]
    for n in sorted({1, max(ch - 1, 1), ch + 1, 2 * ch + 3}):
        frames = small_frames(small, n)
        got = run_remap(pkg, frames, mx, my, SW, SH * SW + 1, SW, SH * SW)
        for k in range(n):
            assert np.array_equal(got[k], small_ref(small, "maps", k)), "%d frames: frame %d" % (n, k)


def test_remap_batch_euroc_size(pkg, oracle, synth):
    H, W = 480, 752
    frames = [synth.make_frame(4400, H, W), synth.make_frame(4401, H, W)]
    mx, my = rectify_maps(H, W, 3)
    got = run_remap(pkg, frames, mx, my, W, H * W, W, H * W)
    for k in range(2):
        ref = oracle.remap_linear(frames[k], mx, my)
        assert (ref == 0).any() and (ref != 0).any()
        assert np.array_equal(got[k], ref)


# ---- chain -------------------------------------------------------------------------------------------------------------------------
def extract_resident(pkg, ex, d_ptr, H, W, stride, fs, n):
    import torch
    cap = ex.configure(H, W, n)
    d_kps = torch.zeros((n, cap, 7), dtype=torch.int32, device="cuda")
    d_desc = torch.zeros((n, cap, 32), dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    ex.extract_batch_device(d_ptr, H, W, stride, fs, n, d_kps.data_ptr(), d_desc.data_ptr(), d_cnt.data_ptr(), cap, (0, 1000),
                            stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    cnt, kps, desc = d_cnt.cpu().numpy(), d_kps.cpu().numpy(), d_desc.cpu().numpy()
    return [(int(cnt[k, 1]), kps[k, :cnt[k, 0]].tobytes(), desc[k, :cnt[k, 0]].tobytes()) for k in range(n)]


def test_chain_into_batched_extraction(pkg, synth):
    """clahe_batch_device in place, then extract_batch_device, against ex(ex.CLAHE(im)) per frame; remap_linear_batch_device into a
    second buffer with a padded stride, then extract_batch_device, against ex(ex.remap(im, mx, my)) per frame."""
    import torch
    H, W, n = 128, 192, 2          # the smallest image tests/test_gpu_batch_layouts.py extracts
    frames = [(synth.make_frame(4500 + k, H, W) // 2 + 30).astype(np.uint8) for k in range(n)]
    mx, my = rectify_maps(H, W, 6)
    host, batch = pkg.ORBextractor(**EUROC), pkg.ORBextractor(**EUROC)
    s = torch.cuda.current_stream().cuda_stream
    try:
        want_clahe, want_remap = [], []
        for f in frames:
            for want, im in ((want_clahe, host.CLAHE(f, 3.0, (8, 8))), (want_remap, host.remap(f, mx, my))):
                mono, kps, desc = host(im)
                assert len(kps) > 50
                want.append((mono, kps.tobytes(), desc.tobytes()))
        d_lut = torch.zeros(n * 64 * 256, dtype=torch.uint8, device="cuda")
        d_img = torch.from_numpy(np.stack(frames)).cuda()
        assert pkg.clahe_batch_device(n, d_img.data_ptr(), H, W, W, H * W, 3.0, 8, 8, d_lut.data_ptr(), d_img.data_ptr(), W, H * W, stream=s) == 0
        assert extract_resident(pkg, batch, d_img.data_ptr(), H, W, W, H * W, n) == want_clahe
        stride = align(W, 64) + 64
        d_src = torch.from_numpy(np.stack(frames)).cuda()
        d_rect = torch.full((n, H, stride), FILL, dtype=torch.uint8, device="cuda")
        d_mx, d_my = torch.from_numpy(mx).cuda(), torch.from_numpy(my).cuda()
        assert pkg.remap_linear_batch_device(n, d_src.data_ptr(), H, W, W, H * W, d_mx.data_ptr(), d_my.data_ptr(), W, H, W, d_rect.data_ptr(), stride,
                                             H * stride, stream=s) == 0
        assert extract_resident(pkg, batch, d_rect.data_ptr(), H, W, stride, H * stride, n) == want_remap
    finally:
        host.close(); batch.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_with_live_buffers(pkg, oracle, small):
    import torch
    frames = small_frames(small, 3)
    SH, SW, n = small["SH"], small["SW"], 3
    mx, my = small["maps"]
    src = np.stack(frames)
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.full((n, SH, SW), FILL, dtype=torch.uint8, device="cuda")
    d_lut = torch.zeros(n * 64 * 256, dtype=torch.uint8, device="cuda")
    d_mx, d_my = torch.from_numpy(mx).cuda(), torch.from_numpy(my).cuda()
    s = torch.cuda.current_stream().cuda_stream
    clahe = dict(nframes=n, d_src=d_src.data_ptr(), rows=SH, cols=SW, src_stride=SW, src_frame_stride=SH * SW, clip_limit=3.0, tiles_x=8, tiles_y=8,
                 d_lut=d_lut.data_ptr(), d_dst=d_dst.data_ptr(), dst_stride=SW, dst_frame_stride=SH * SW, stream=s)
    remap = dict(nframes=n, d_src=d_src.data_ptr(), src_rows=SH, src_cols=SW, src_stride=SW, src_frame_stride=SH * SW, d_mapx=d_mx.data_ptr(),
                 d_mapy=d_my.data_ptr(), map_stride_elems=SW, rows=SH, cols=SW, d_dst=d_dst.data_ptr(), dst_stride=SW, dst_frame_stride=SH * SW, stream=s)
    for c in (dict(d_dst=d_src.data_ptr() + 1), dict(d_dst=d_src.data_ptr() + SH * SW), dict(src_frame_stride=SH * SW - 1), dict(dst_frame_stride=SH * SW - 1)):
        with pytest.raises(ValueError):
            pkg.clahe_batch_device(**dict(clahe, **c))
    for c in (dict(d_dst=d_src.data_ptr()), dict(d_dst=d_src.data_ptr() + n * SH * SW - 1), dict(src_frame_stride=SH * SW - 1),
              dict(dst_frame_stride=SH * SW - 1)):
        with pytest.raises(ValueError):
            pkg.remap_linear_batch_device(**dict(remap, **c))
    torch.cuda.synchronize()
    assert np.array_equal(d_src.cpu().numpy(), src) and bool((d_dst == FILL).all())      # nothing was touched
    assert pkg.remap_linear_batch_device(**remap) == 0                                   # and the good calls still work
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    for k in range(n):
        assert np.array_equal(got[k], small_ref(small, "maps", k))
    assert pkg.clahe_batch_device(**clahe) == 0
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    for k in range(n):
        assert np.array_equal(got[k], oracle.clahe(frames[k], 3.0, (8, 8)))
