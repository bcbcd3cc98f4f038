"""Row pitch and alignment of the input frames: stride > w * channels, offset base pointers, padded
frame strides (a cv::Mat ROI is such a view).

launch_front picks k_front's interior loads from the alignment of the base pointers, the stride and
the frame stride (16-B / 48-B loads and LDS-DMA, or a byte per lane); k_gray_pad, k_gray_rows and
the trajectory / ring entries take the same arguments.  The frames are mdx_synth_pair's, embedded
in byte buffers full of seeded noise, so a read of the padding changes a result; every buffer ends
exactly with the last row's last pixel.  Results equal the oracle's on the packed frames bit for
bit.
"""
import numpy as np
import pytest

from oracle_check import (OutputSet, assert_batch_equals_oracle, assert_pair_equals_oracle, assert_traj_equals_oracle,
                          uploaded)
from traj_seq import sequence

W, H = 330, 250          # three pyramid levels, 825 points at pixel_step 10


def _embed(frames, stride, offset=0, frame_stride=None, seed=1):
    """The frames (same shape) at `offset` into one noise-filled byte buffer, `frame_stride` apart
    (default: one buffer per frame).  Returns (buffers, views): views[i] is a numpy view of frame i
    with row pitch `stride`; a buffer ends with its last frame's last pixel."""
    h, w = frames[0].shape[:2]
    ch = 1 if frames[0].ndim == 2 else 3
    assert stride >= w * ch
    one = stride * (h - 1) + w * ch
    rng = np.random.default_rng(seed)
    groups = [[f] for f in frames] if frame_stride is None else [frames]
    bufs, views = [], []
    for g in groups:
        size = offset + (frame_stride or 0) * (len(g) - 1) + one
        buf = rng.integers(0, 256, size, dtype=np.uint8)
        assert buf.nbytes == offset + (frame_stride or 0) * (len(g) - 1) + stride * (h - 1) + w * ch
        for i, f in enumerate(g):
            start = offset + (frame_stride or 0) * i
            shape, strides = ((h, w), (stride, 1)) if ch == 1 else ((h, w, 3), (stride, 3, 1))
            v = np.lib.stride_tricks.as_strided(buf[start:start + one], shape, strides)
            v[...] = f
            assert v.ctypes.data == buf.ctypes.data + start
            views.append(v)
        bufs.append(buf)
    return bufs, views


_shared = {}             # packed frames and their oracle results, computed once and left unchanged


def _pair_ref(mdx, oracle, w, h, ps, ch, fmt_name="rgb"):
    key = (w, h, ps, ch, fmt_name)
    if key not in _shared:
        a, b, _ = mdx.synth_pair(9000 + w + ch, w, h, ch)
        fmt = None if ch == 1 else (oracle.FMT_RGB8 if fmt_name == "rgb" else oracle.FMT_BGR8)
        _shared[key] = (a, b, oracle.calculate_optical_flow(a, b, fmt=fmt, nthreads=8, pixel_step=ps,
                                                             min_vector_size=1.0))
    return _shared[key]


def _traj_ref(mdx, oracle, ch):
    key = ("traj", ch)
    if key not in _shared:
        frames = sequence(mdx, oracle, W, H, 4, seed=77 + ch, channels=ch)
        _shared[key] = (frames, oracle.flow_trajectory(frames, nthreads=8, pixel_step=10))
    return _shared[key]


def test_wrapper_keeps_pitched_views():
    """CPU: a valid row-pitched view reaches the C-ABI as it is; anything else is packed."""
    from motion_detection_amd import context as mctx
    buf = np.zeros(4 + 336 * 250, np.uint8)
    v = np.lib.stride_tricks.as_strided(buf[3:], (250, 330), (336, 1))
    assert mctx._frame_view(v) is v
    rgb = np.lib.stride_tricks.as_strided(buf[1:], (80, 100, 3), (336, 3, 1))
    assert mctx._frame_view(rgb) is rgb
    crop = np.zeros((300, 400), np.uint8)[20:270, 30:360]          # a ROI of a larger image
    assert mctx._frame_view(crop).strides == (400, 1) and np.shares_memory(mctx._frame_view(crop), crop)
    for bad in (v[::-1], v[:, ::2], v.T, rgb[:, :, ::-1], rgb[:, :, :2]):
        out = mctx._frame_view(bad)
        assert out.flags.c_contiguous and np.array_equal(out, bad)
    # the two frames of a pair are packed only when their pitches differ
    p, q = mctx._frame_views([v, v.copy()])
    assert p.flags.c_contiguous and q.flags.c_contiguous
    p, q = mctx._frame_views([v, v])
    assert p is v and q is v


GRAY_HOST = [(336, 0), (333, 0), (331, 0), (336, 1), (336, 2), (336, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("stride,offset", GRAY_HOST)
def test_host_entry_gray_pitched(mdx, ctx, oracle, stride, offset):
    a, b, ref = _pair_ref(mdx, oracle, W, H, 10, 1)
    _, (va, vb) = _embed([a, b], stride, offset, seed=stride + offset)
    assert va.strides == (stride, 1)
    ctx.set_params(pixel_step=10, min_vector_size=1.0, fit_mode=mdx.FIT_FIRST4)
    assert_pair_equals_oracle(ctx.flow_warp_diff(va, vb), ref, f"gray stride {stride} offset {offset}")


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [990, 992, 1001])
@pytest.mark.parametrize("fmt_name", ["rgb", "bgr"])
def test_host_entry_color_pitched(mdx, ctx, oracle, fmt_name, stride):
    a, b, ref = _pair_ref(mdx, oracle, W, H, 10, 3, fmt_name)
    _, (va, vb) = _embed([a, b], stride, seed=stride)
    ctx.set_params(pixel_step=10, min_vector_size=1.0, fit_mode=mdx.FIT_FIRST4)
    res = ctx.flow_warp_diff(va, vb, fmt=mdx.FMT_RGB8 if fmt_name == "rgb" else mdx.FMT_BGR8)
    assert_pair_equals_oracle(res, ref, f"{fmt_name} stride {stride}")


@pytest.mark.gpu
def test_host_entry_single_level_pitched(mdx, ctx, oracle):
    """64 x 48: one pyramid level, k_gray_pad."""
    a, b, ref = _pair_ref(mdx, oracle, 64, 48, 4, 1)
    _, (va, vb) = _embed([a, b], 67, seed=67)
    ctx.set_params(pixel_step=4, min_vector_size=1.0, fit_mode=mdx.FIT_FIRST4)
    try:
        res = ctx.flow_warp_diff(va, vb)
    finally:
        ctx.set_params(pixel_step=10)
    assert_pair_equals_oracle(res, ref, "64x48 stride 67")


TRAJ_PITCH = [(1, 336, 0), (1, 333, 1), (3, 992, 0), (3, 1001, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("ch,stride,offset", TRAJ_PITCH)
def test_flow_trajectory_pitched(mdx, ctx, oracle, ch, stride, offset):
    frames, ref = _traj_ref(mdx, oracle, ch)
    _, views = _embed(frames, stride, offset, seed=stride)
    ctx.set_params(pixel_step=10, min_vector_size=1.0)
    assert_traj_equals_oracle(ctx.flow_trajectory(views), ref, f"ch {ch} stride {stride} offset {offset}")


@pytest.mark.gpu
@pytest.mark.parametrize("ch,stride,offset", TRAJ_PITCH)
def test_ring_pitched(mdx, ctx, oracle, ch, stride, offset):
    frames, ref = _traj_ref(mdx, oracle, ch)
    _, views = _embed(frames, stride, offset, seed=stride + 1)
    ctx.set_params(pixel_step=10, min_vector_size=1.0)
    ctx.ring_reset()
    try:
        for k, v in enumerate(views):
            assert ctx.ring_push(v, len(views)) == k + 1
        res = ctx.ring_trajectory(W, H, len(views))
    finally:
        ctx.ring_reset()
    assert_traj_equals_oracle(res, ref, f"ring ch {ch} stride {stride} offset {offset}")


@pytest.mark.gpu
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("stride_px,fs_pad", [(336, 0), (336, 2), (333, 1)])
def test_batch_dev_pitched(mdx, oracle, stride_px, fs_pad, base, ch):
    """flow_warp_diff_batch_dev, B = 3: (stride, frame_stride) = (s, s * h + pad) with s = stride_px *
    channels, the frames starting `base` bytes into the allocation."""
    B = 3
    stride = stride_px * ch
    frame_stride = stride * H + fs_pad
    pairs = []
    for i in range(B):
        key = ("dev", i, ch)
        if key not in _shared:
            a, b, _ = mdx.synth_pair(9100 + i, W, H, ch)
            _shared[key] = (a, b, oracle.calculate_optical_flow(a, b, nthreads=8, pixel_step=10, min_vector_size=1.0))
        pairs.append(_shared[key])
    (buf1,), _ = _embed([p[0] for p in pairs], stride, base, frame_stride, seed=1 + fs_pad)
    (buf2,), _ = _embed([p[1] for p in pairs], stride, base, frame_stride, seed=2 + fs_pad)
    n = mdx.grid_count(W, H, 10)
    with mdx.Context(0, W, H, B) as c:
        c.set_params(pixel_step=10, min_vector_size=1.0)
        with uploaded(c, buf1, buf2) as (d1, d2), OutputSet(c, B, W, H, n) as out:
            out.prefill()
            out.call(d1 + base, d2 + base, stride, frame_stride, mdx.FMT_GRAY8 if ch == 1 else mdx.FMT_RGB8)
            c.sync()
            got = out.read()
    assert_batch_equals_oracle(got, [p[2] for p in pairs], f"stride {stride} frame_stride {frame_stride} base {base}")


@pytest.mark.gpu
def test_band_flow_pitched_rgb(mdx, oracle):
    """band_flow_dev / band_fit_warp_dev, 3 bands, on a pitched rgb pair one byte into its buffer."""
    from motion_detection_amd import rowtile
    nb, stride, base = 3, 1001, 1
    a, b, ref = _pair_ref(mdx, oracle, W, H, 10, 3)
    (buf1,), _ = _embed([a], stride, base, seed=5)
    (buf2,), _ = _embed([b], stride, base, seed=6)
    n = mdx.grid_count(W, H, 10)
    with mdx.Context(0, W, H, 1, pixel_step=10, min_vector_size=1.0) as c:
        d = {k: c.dev_alloc(sz) for k, sz in dict(i1=buf1.nbytes, i2=buf2.nbytes, np=n * 8, st=n, vec=n * 32,
                                                   cand=nb * 96, mask=W * H, H=72, num=4).items()}
        try:
            c.h2d(d["i1"], buf1)
            c.h2d(d["i2"], buf2)
            c.h2d(d["vec"], np.zeros(n * 32, np.uint8))
            for r in range(nb):
                y0, y1 = rowtile.band_rows(H, nb, r)
                c.band_flow_dev(d["i1"] + base, d["i2"] + base, W, H, stride, mdx.FMT_RGB8, y0, y1, d["np"], d["st"],
                                d["cand"] + 96 * r, d["vec"])
            c.sync()
            for r in range(nb):
                y0, y1 = rowtile.band_rows(H, nb, r)
                c.band_fit_warp_dev(nb, d["cand"], y0, y1, d["mask"] + y0 * W, d["H"], d["num"])
            c.sync()
            out = dict(np=np.empty((n, 2), np.float32), st=np.empty(n, np.uint8), vec=np.empty((n, 4)),
                       mask=np.empty((H, W), np.uint8), H=np.empty((3, 3)), num=np.empty(1, np.int32))
            for k, arr in out.items():
                c.d2h(arr, d[k])
        finally:
            for p in d.values():
                c.dev_free(p)
    got = dict(num_vectors=out["num"][0], status=out["st"], next_pts=out["np"], vectors=out["vec"], H=out["H"],
               mask=out["mask"])
    assert_pair_equals_oracle(got, ref, "3 bands, pitched rgb")
