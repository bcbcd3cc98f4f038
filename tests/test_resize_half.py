"""Half-size ingest (include/mdx.h mdx_half_size, mdx_resize_half_dev, mdx_resize_half, mdx_ring_push_half;
DESIGN.md §7i): the reference node's cv::resize(img, out, cv::Size(), 0.5, 0.5) of every frame wider than
320 px (ros/src/motion_detection_node.cpp:470-474), as a device stage.

The checker below is a direct numpy transcription of the arithmetic in include/mdx.h (OpenCV 2.4.8's
INTER_LINEAR -> INTER_AREA redirection at scale 2 and resizeAreaFast_'s 2x2 fast mode): integer sums,
(s + 2) >> 2 for full cells, np.rint of the exact s / count for partial ones.  It shares nothing with the
kernel.  CPU: the size table, known answers by hand, the inputs' teeth, argument checks.  GPU: every byte
of the destination, pitch padding included, over shapes, channels, pitches and base offsets that reach
both of k_half's paths; batches; the host entry; the ring entry against the oracle on the checker's
halved frames.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

# motion_detection_amd/csrc/mdx_internal.h
HALF_PX = 4                    # kHalfPx: destination pixels per lane
HALF_WAVE_PX = 64 * HALF_PX    # kHalfWavePx: destination pixels of a row per wave
HALF_WG_PX = 256 * HALF_PX     # kHalfWgPx: destination pixels of a row per workgroup
HALF_ROWS = 4                  # kHalfRows: destination rows per workgroup (its row strip)

FILL = 0xAA


# ---------------------------------------------------------------- the checker

def half_size_ref(w, h):
    """cvRound(side * 0.5), half to even."""
    def side(v):
        k = v // 2
        return k if v % 2 == 0 or k % 2 == 0 else k + 1
    return side(w), side(h)


def block_sums(img):
    """(sums, counts) over the in-frame pixels of every destination cell's 2 x 2 block."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    dw, dh = half_size_ref(w, h)
    assert dw > 0 and dh > 0
    a = img.reshape(h, w, -1).astype(np.int64)
    H, W = max(2 * dh, h), max(2 * dw, w)
    s = np.zeros((H, W, a.shape[2]), np.int64)
    n = np.zeros((H, W, 1), np.int64)
    s[:h, :w] = a
    n[:h, :w] = 1
    s, n = s[:2 * dh, :2 * dw], n[:2 * dh, :2 * dw]           # a side that rounded down drops its last pixel
    blk = lambda v: v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2]
    return blk(s), np.broadcast_to(blk(n), blk(s).shape)


def half_ref(img):
    sums, cnt = block_sums(img)
    out = np.where(cnt == 4, (sums + 2) >> 2, np.rint(sums / cnt).astype(np.int64))
    return out.astype(np.uint8).reshape(out.shape[:2] if np.ndim(img) == 2 else out.shape)


# ---------------------------------------------------------------- shapes and inputs

SHAPES = [(2, 2), (3, 2), (2, 3), (3, 3), (5, 5), (7, 7), (9, 6), (321, 7), (322, 5), (323, 9), (647, 483), (1027, 6),
          (640, 480)]
SHAPES += [
    (2 * HALF_WAVE_PX - 2, 2 * HALF_ROWS - 2),   # dw one below kHalfWavePx, dh one below kHalfRows
    (2 * HALF_WAVE_PX, 2 * HALF_ROWS),           # dw = kHalfWavePx, dh = kHalfRows: exactly one wave, one strip
    (2 * HALF_WAVE_PX + 2, 2 * HALF_ROWS + 2),   # one above either: a second wave with one lane, a second strip
    (2 * HALF_WG_PX - 2, 2 * HALF_ROWS + 1),     # dw one below kHalfWgPx; h = 9 drops its last row (dh = kHalfRows)
    (2 * HALF_WG_PX, 2 * HALF_ROWS + 3),         # dw = kHalfWgPx; h = 11: a partial last row opens a second strip
    (2 * HALF_WG_PX + 2, 2 * HALF_ROWS - 1),     # a second workgroup with one lane; h = 7: a partial row ends the strip
    (2 * HALF_WG_PX + 3, 2 * HALF_ROWS + 2),     # w = 2051: the second workgroup's lane holds a partial column
    (2 * HALF_PX * 3 + 1, 2 * HALF_ROWS),        # w = 25: a lane whose cells are all full next to a dropped column
    (2 * HALF_PX * 3 + 3, 2 * HALF_ROWS),        # w = 27: the last lane mixes full cells and the partial column
]
SRC_PADS = (0, 1, 13)
SRC_OFFSETS = (0, 1, 3)
DST_PADS = (0, 5)


def frame_for(w, h, cn):
    """Uniform noise, with the cells the arithmetic's tie rules decide planted in every channel: a full cell
    summing to 2, and on a partial last column / row two-pixel cells summing to 1 and (where there is
    room) to 3."""
    rng = np.random.default_rng(w * 10007 + h * 31 + cn)
    f = rng.integers(0, 256, (h, w, cn), dtype=np.uint8)
    dw, dh = half_size_ref(w, h)
    f[0, 0], f[0, 1], f[1, 0], f[1, 1] = 0, 1, 1, 0
    if 2 * dw > w:
        f[0, w - 1], f[1, w - 1] = 0, 1
        if h >= 4:
            f[2, w - 1], f[3, w - 1] = 1, 2
    if 2 * dh > h:
        f[h - 1, 0], f[h - 1, 1] = 0, 1
        if w >= 5:
            f[h - 1, 2], f[h - 1, 3] = 1, 2
    return f[:, :, 0].copy() if cn == 1 else f


def vector_path(src_ptr, stride, dst_ptr, dst_stride, batch=1, frame_stride=0, dst_frame_stride=0):
    """k_half's alignment rule (mdx_resize.hip half_vector_path): every base and pitch, and a batch's frame
    pitches, a multiple of 4."""
    m = src_ptr | stride | dst_ptr | dst_stride
    if batch > 1:
        m |= frame_stride | dst_frame_stride
    return m % 4 == 0


def pitch_cases(w, cn):
    """(src pad, src offset, dst pad): the issue's grid, plus the pads that make each pitch a multiple of 4,
    so that every shape reaches the vector path as well."""
    dw, _ = half_size_ref(w, 2)
    src_pads = sorted(set(SRC_PADS) | {(-w * cn) % 4})
    dst_pads = sorted(set(DST_PADS) | {(-dw * cn) % 4})
    return list(itertools.product(src_pads, SRC_OFFSETS, dst_pads))


# ---------------------------------------------------------------- CPU

SIZE_TABLE = {3: 2, 5: 2, 7: 4, 9: 4, 321: 160, 323: 162, 2: 1, 4: 2, 320: 160, 640: 320, 1920: 960, 1081: 540,
              1083: 542}


def test_half_size_values(mdx):
    for v, d in SIZE_TABLE.items():
        assert half_size_ref(v, v) == (d, d), v
        assert mdx.half_size(v, v) == (d, d), v
        assert mdx.half_size(v, 480) == (d, 240) and mdx.half_size(640, v) == (320, d), v
    assert half_size_ref(1, 1) == (0, 0)
    L = mdx.lib()
    dw, dh = C.c_int(-7), C.c_int(-9)
    for w, h in [(1, 480), (640, 1), (0, 5), (5, 0), (-4, 8), (1, 1)]:
        assert L.mdx_half_size(w, h, C.byref(dw), C.byref(dh)) == mdx._lib.MDX_EINVAL, (w, h)
        assert (dw.value, dh.value) == (-7, -9)            # untouched
        with pytest.raises(ValueError):
            mdx.half_size(w, h)
    assert L.mdx_half_size(8, 8, None, C.byref(dh)) == mdx._lib.MDX_EINVAL


HAND_CASES = [
    # >> 2 against half-even rounding: the sum 2 gives (2 + 2) >> 2 = 1, cvRound(2 / 4.) = 0
    (np.array([[0, 1], [1, 0]], np.uint8), np.array([[1]], np.uint8)),
    # 3 x 3 -> 2 x 2: a full cell, both edge ties (1 -> 0, 3 -> 2) and the count-1 corner
    (np.array([[10, 20, 1], [30, 41, 0], [1, 2, 77]], np.uint8), np.array([[25, 0], [2, 77]], np.uint8)),
    # 5 x 5 -> 2 x 2: the last row and column (255) are read by nothing
    (np.array([[4, 4, 8, 8, 255], [4, 4, 8, 9, 255], [0, 0, 1, 1, 255], [0, 1, 1, 1, 255], [255] * 5], np.uint8),
     np.array([[4, 8], [0, 1]], np.uint8)),
]


def test_known_answers_by_hand():
    for src, want in HAND_CASES:
        assert np.array_equal(half_ref(src), want), src
        rgb = np.stack([src, src, src], 2)
        assert np.array_equal(half_ref(rgb), np.stack([want] * 3, 2))
    # the ties once more, spelled out: two pixels summing to 1 give 0, to 3 give 2, to 5 give 2, to 7 give 4
    col = np.array([[0, 0, 0], [0, 0, 1], [0, 0, 2], [0, 0, 1], [0, 0, 3], [0, 0, 2], [0, 0, 4], [0, 0, 3]], np.uint8)
    assert half_ref(col)[:, 1].tolist() == [0, 2, 2, 4]


@pytest.mark.parametrize("w,h", SHAPES)
def test_inputs_have_teeth(w, h):
    """Every GPU input holds full cells whose sum is 2 mod 4 (where (s + 2) >> 2 and cvRound(s / 4.)
    differ), and every shape with two-pixel partial cells holds odd sums among them (the half-even ties),
    rounding down (1 -> 0) and, where the edge has two such cells, up (3 -> 2) as well."""
    dw, dh = half_size_ref(w, h)
    for cn in (1, 3):
        s, n = block_sums(frame_for(w, h, cn))
        assert np.any(s[n == 4] % 4 == 2), (w, h, cn)
        assert s[0, 0].tolist() == [2] * cn
        two = s[n == 2]
        assert (two.size > 0) == (2 * dw > w or 2 * dh > h)
        if two.size:
            assert np.any(two == 1), (w, h, cn)
        if (2 * dw > w and h >= 4) or (2 * dh > h and w >= 5):
            assert np.any(two == 3), (w, h, cn)
        assert np.any(n == 1) == (2 * dw > w and 2 * dh > h)


def test_argument_checks_without_a_device(mdx):
    L = mdx.lib()
    E = mdx._lib.MDX_EINVAL
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.mdx_resize_half_dev(None, 1, p, 4, 4, 4, 16, 1, p, 2, 4) == E
    assert L.mdx_resize_half_dev(None, 1, p, 4, 4, 4, 16, 2, p, 2, 4) == E      # and bad channels
    assert L.mdx_resize_half_dev(None, 1, p, 4, 4, 3, 16, 1, p, 2, 4) == E      # and a short pitch
    assert L.mdx_resize_half(None, p, 4, 4, 4, 1, p, 2) == E
    assert L.mdx_resize_half(None, p, 4, 4, 4, 1, p, 1) == E                    # and a short destination pitch
    assert L.mdx_ring_push_half(None, p, 4, 4, 4, 0, 1) == E
    assert L.mdx_ring_push_half(None, None, 4, 4, 4, 0, 1) == E


# ---------------------------------------------------------------- GPU

class DevArena:
    """One device allocation for sources and one for destinations, reused by every case."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.n = ctx, nbytes
        self.src, self.dst = ctx.dev_alloc(nbytes), ctx.dev_alloc(nbytes)

    def close(self):
        self.ctx.dev_free(self.src)
        self.ctx.dev_free(self.dst)


@pytest.fixture(scope="module")
def arena(ctx):
    a = DevArena(ctx, 64 << 20)
    yield a
    a.close()


def pitched(frames, stride, frame_stride, offset):
    """The frames' bytes at a row pitch and a frame pitch, `offset` bytes into a buffer; every byte between
    rows and frames is 0x55."""
    h = frames[0].shape[0]
    row = frames[0].reshape(h, -1).shape[1]
    buf = np.full(offset + frame_stride * len(frames), 0x55, np.uint8)
    for b, f in enumerate(frames):
        o = offset + b * frame_stride
        v = np.lib.stride_tricks.as_strided(buf[o:], (h, row), (stride, 1))
        v[...] = f.reshape(h, row)
    return buf


def run_dev(arena, frames, cn, stride, frame_stride, offset, dst_stride, dst_frame_stride):
    """mdx_resize_half_dev on pitched frames; returns the destination buffer, prefilled with FILL."""
    ctx = arena.ctx
    h, w = frames[0].shape[:2]
    src = pitched(frames, stride, frame_stride, offset)
    out = np.full(dst_frame_stride * len(frames), FILL, np.uint8)
    assert src.nbytes <= arena.n and out.nbytes <= arena.n
    ctx.h2d(arena.src, src)
    ctx.h2d(arena.dst, out)
    ctx.resize_half_dev(len(frames), arena.src + offset, w, h, stride, frame_stride, cn, arena.dst, dst_stride,
                        dst_frame_stride)
    ctx.sync()
    ctx.d2h(out, arena.dst)
    return out


def check_dst(out, wants, dst_stride, dst_frame_stride, label):
    """Every byte: the halved rows, and FILL everywhere else (pitch padding, frame padding)."""
    dh = wants[0].shape[0]
    row = wants[0].reshape(dh, -1).shape[1]
    expect = np.full(out.shape, FILL, np.uint8)
    for b, wnt in enumerate(wants):
        v = np.lib.stride_tricks.as_strided(expect[b * dst_frame_stride:], (dh, row), (dst_stride, 1))
        v[...] = wnt.reshape(dh, row)
    if not np.array_equal(out, expect):
        bad = np.nonzero(out != expect)[0]
        raise AssertionError(f"{label}: {bad.size} bytes differ, first at {bad[0]} (frame {bad[0] // dst_frame_stride}, "
                             f"row {bad[0] % dst_frame_stride // dst_stride}, byte {bad[0] % dst_frame_stride % dst_stride}): "
                             f"got {out[bad[0]]}, want {expect[bad[0]]}")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SHAPES)
def test_dev_entry_every_byte(arena, w, h):
    dw, dh = half_size_ref(w, h)
    for cn in (1, 3):
        f = frame_for(w, h, cn)
        want = half_ref(f)
        paths = set()
        for spad, off, dpad in pitch_cases(w, cn):
            stride, dst_stride = w * cn + spad, dw * cn + dpad
            paths.add(vector_path(arena.src + off, stride, arena.dst, dst_stride))
            out = run_dev(arena, [f], cn, stride, stride * h, off, dst_stride, dst_stride * dh)
            check_dst(out, [want], dst_stride, dst_stride * dh, f"{w}x{h} cn {cn} pad {spad} off {off} dpad {dpad}")
        assert paths == {True, False}, (w, h, cn)          # the vector and the byte path


@pytest.mark.gpu
def test_hand_cases_on_the_device(ctx):
    for src, want in HAND_CASES:
        assert np.array_equal(ctx.resize_half(src), want)
        assert np.array_equal(ctx.resize_half(np.stack([src] * 3, 2)), np.stack([want] * 3, 2))


def _hip():
    """The HIP runtime libmdx.so is linked against (already loaded: dlopen returns it)."""
    L = C.CDLL("libamdhip64.so")
    L.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return L


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 3, 32])
@pytest.mark.parametrize("w,h,cn,spad,dpad,vec", [(323, 9, 3, 3, 2, True), (323, 9, 3, 1, 5, False),
                                                  (646, 51, 1, 2, 1, True), (1027, 6, 3, 0, 0, False)])
def test_batches_behind_an_upload(mdx, arena, batch, w, h, cn, spad, dpad, vec):
    """One launch for the batch, frame pitches padded, queued right behind the frames' upload on the
    context's stream with no host synchronisation in between; each frame equals its single-frame result."""
    ctx = arena.ctx
    dw, dh = half_size_ref(w, h)
    frames = [frame_for(w, h, cn) ^ np.uint8(37 * b % 256) for b in range(batch)]
    stride, dst_stride = w * cn + spad, dw * cn + dpad
    # frame pitches: padded, and a multiple of 4 exactly when the row pitches are (so both paths get batches)
    frame_stride = stride * h + 4 * stride + (0 if stride % 4 == 0 else 1)
    dst_frame_stride = dst_stride * dh + 8 * dst_stride
    singles = []
    for f in frames:
        out = run_dev(arena, [f], cn, stride, stride * h, 0, dst_stride, dst_stride * dh)
        singles.append(np.lib.stride_tricks.as_strided(out, (dh, dw * cn), (dst_stride, 1)).copy())
        assert np.array_equal(singles[-1].reshape(half_ref(f).shape), half_ref(f))
    src = pitched(frames, stride, frame_stride, 0)
    host = mdx.host_empty((src.nbytes,))
    host[...] = src
    out = np.full(dst_frame_stride * batch, FILL, np.uint8)
    ctx.h2d(arena.src, np.zeros(src.nbytes, np.uint8))        # a launch that ran early would halve zeros
    ctx.h2d(arena.dst, out)
    assert _hip().hipMemcpyAsync(arena.src, host.ctypes.data, src.nbytes, 1, ctx.stream) == 0
    ctx.resize_half_dev(batch, arena.src, w, h, stride, frame_stride, cn, arena.dst, dst_stride, dst_frame_stride)
    ctx.sync()
    ctx.d2h(out, arena.dst)
    check_dst(out, singles, dst_stride, dst_frame_stride, f"batch {batch}")
    assert vector_path(arena.src, stride, arena.dst, dst_stride, batch, frame_stride, dst_frame_stride) == vec


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(2, 2), (3, 3), (9, 6), (323, 9), (647, 483), (640, 480), (2 * HALF_WG_PX + 3, 10)])
def test_host_entry_same_bytes(mdx, ctx, w, h):
    for cn in (1, 3):
        f = frame_for(w, h, cn)
        assert np.array_equal(ctx.resize_half(f), half_ref(f))
        # a pitched view (a crop of a larger image) goes down with its pitch
        big = np.full((h + 2, w + 5) + f.shape[2:], 0x55, np.uint8)
        big[1:h + 1, 2:w + 2] = f
        assert np.array_equal(ctx.resize_half(big[1:h + 1, 2:w + 2]), half_ref(f))
    # the destination's pitch padding is not written
    L = mdx.lib()
    f = frame_for(w, h, 3)
    dw, dh = half_size_ref(w, h)
    out = np.full((dh, dw * 3 + 7), FILL, np.uint8)
    assert L.mdx_resize_half(ctx._h, f.ctypes.data_as(C.c_void_p), w, h, w * 3, 3, out.ctypes.data_as(C.c_void_p),
                             dw * 3 + 7) == 0
    assert np.array_equal(out[:, :dw * 3].reshape(dh, dw, 3), half_ref(f)) and np.all(out[:, dw * 3:] == FILL)


@pytest.mark.gpu
def test_argument_checks(mdx, arena):
    ctx = arena.ctx
    ok = dict(batch=1, d_src=arena.src, w=8, h=8, stride=24, frame_stride=192, channels=3, d_dst=arena.dst,
              dst_stride=12, dst_frame_stride=48)
    ctx.resize_half_dev(**ok)
    for bad, msg in [(dict(batch=0), "batch"), (dict(channels=2), "channels"), (dict(channels=4), "channels"),
                     (dict(stride=23), "stride"), (dict(frame_stride=191), "frame_stride"),
                     (dict(dst_stride=11), "dst_stride"), (dict(dst_frame_stride=47), "dst_frame_stride"),
                     (dict(w=1), "halves to 0"), (dict(h=1, frame_stride=24), "halves to 0"),
                     (dict(d_src=0), "null"), (dict(d_dst=0), "null"),
                     (dict(d_dst=arena.src + 100), "overlap"), (dict(d_dst=arena.src), "overlap"),
                     (dict(batch=2, d_dst=arena.src + 192 + 7 * 24 + 23), "overlap")]:
        with pytest.raises(mdx.MdxError, match=msg):
            ctx.resize_half_dev(**{**ok, **bad})
    ctx.resize_half_dev(**{**ok, "d_dst": arena.src + 192})          # right behind the source: no overlap
    ctx.sync()
    with pytest.raises(ValueError):
        ctx.resize_half(np.zeros((4, 4, 2), np.uint8))
    with pytest.raises(ValueError):
        ctx.resize_half(np.zeros((1, 8), np.uint8))


# ---------------------------------------------------------------- the ring entry

@pytest.mark.gpu
@pytest.mark.parametrize("channels", [3, 1])
def test_ring_push_half_matches_oracle(mdx, ctx, oracle, channels):
    """Five 647 x 483 frames pushed halved (324 x 242: both sides round up, partial column and row): the
    ring trajectory equals the oracle's on the checker's halved frames, bit for bit."""
    from oracle_check import assert_traj_equals_oracle
    from traj_seq import sequence
    w, h = 647, 483
    frames = sequence(mdx, oracle, w, h, 5, seed=90 + channels, channels=channels)
    halves = [half_ref(f) for f in frames]
    dw, dh = half_size_ref(w, h)
    assert (dw, dh) == (324, 242) and halves[0].shape[:2] == (dh, dw)
    ctx.ring_reset()
    for k, f in enumerate(frames):
        assert ctx.ring_push(f, 5, half=True) == k + 1
    assert_traj_equals_oracle(ctx.ring_trajectory(dw, dh, 5),
                              oracle.flow_trajectory(halves, pixel_step=10, nthreads=8), "halved ring")


@pytest.mark.gpu
def test_ring_mixes_halved_and_full_frames_of_one_size(mdx, ctx, oracle):
    """Frames pushed either way share a ring when their resulting sizes agree; a frame of another halved
    size empties it."""
    from oracle_check import assert_traj_equals_oracle
    from traj_seq import sequence
    big = sequence(mdx, oracle, 640, 480, 3, seed=61, channels=3)
    small = sequence(mdx, oracle, 320, 240, 1, seed=62, channels=3)
    ctx.ring_reset()
    for k, f in enumerate(big):
        assert ctx.ring_push(f, 5, half=True) == k + 1
    assert ctx.ring_push(small[0], 5) == 4                          # 320 x 240 as it is: the ring is kept
    ring = [half_ref(f) for f in big] + small
    assert_traj_equals_oracle(ctx.ring_trajectory(320, 240, 4),
                              oracle.flow_trajectory(ring, pixel_step=10, nthreads=8), "mixed ring")
    assert ctx.ring_push(frame_for(646, 480, 3), 5, half=True) == 1  # 323 x 240: another size, the ring starts over
    assert ctx.ring_push(big[0], 5, half=True) == 1
    ctx.ring_reset()
    ctx.sync()
