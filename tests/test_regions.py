"""The pair path's mask labelled into regions on the device (mdx_mask_regions_dev / mdx_mask_regions).

Recipe: BackgroundSubtractor::getMotionContours (reference
common/src/background_subtractor.cpp:31-35: erode, dilate with the default 3x3 element, findContours'
8-connected blobs), each blob reduced to its boundingRect (common/src/optical_flow_visualizer.cpp:230-236).
Restated from the source; unpinned against a real build (no OpenCV 2.4 to run).

The checker below is written from that text, not from the kernels: the opening by padded shifts, then
a raster scan with a flood fill per unlabelled foreground pixel.  It knows nothing of tiles, bit
words or union-find, so the two check each other; every device output must equal it exactly.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AA = np.int32(-1431655766)       # 0xAAAAAAAA: what every output buffer holds before a call
OPEN3 = 1


# ---------------------------------------------------------------- the checker

def opening(fg):
    """fg (h, w) bool -> D (h, w) bool: 3x3 erosion then 3x3 dilation; out-of-image neighbours
    neither erode nor dilate."""
    h, w = fg.shape
    p = np.ones((h + 2, w + 2), bool)
    p[1:-1, 1:-1] = fg
    e = np.ones((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            e &= p[dy:dy + h, dx:dx + w]
    q = np.zeros((h + 2, w + 2), bool)
    q[1:-1, 1:-1] = e
    d = np.zeros((h, w), bool)
    for dy in range(3):
        for dx in range(3):
            d |= q[dy:dy + h, dx:dx + w]
    return d


def regions_reference(mask, open3=True, min_area=1, connectivity=8):
    """labels (h, w) int32 (-1 background), num_all, the kept records (k, 8) and D as 0 / 255.
    connectivity=4 is the wrong variant the diagonal inputs must tell apart."""
    fg = np.asarray(mask) != 0
    h, w = fg.shape
    d = opening(fg) if open3 else fg
    w2 = w + 2
    g = np.zeros((h + 2, w2), np.uint8)
    g[1:-1, 1:-1] = d
    todo = bytearray(g.tobytes())                  # 1: foreground not yet labelled
    offs = (-w2, -1, 1, w2) if connectivity == 4 else (-w2 - 1, -w2, -w2 + 1, -1, 1, w2 - 1, w2, w2 + 1)
    lab = np.full((h + 2) * w2, -1, np.int32)
    recs = []
    for start in np.flatnonzero(g.ravel()).tolist():   # raster order: a component's first pixel opens it
        if not todo[start]:
            continue
        todo[start] = 0
        stack, members = [start], []
        while stack:
            p = stack.pop()
            members.append(p)
            for o in offs:
                if todo[p + o]:
                    todo[p + o] = 0
                    stack.append(p + o)
        m = np.array(members)
        ys, xs = m // w2 - 1, m % w2 - 1
        cid = len(recs)
        lab[m] = cid
        recs.append((xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1, len(m),
                     start % w2 - 1, start // w2 - 1, cid))
    recs = np.array(recs, np.int32).reshape(-1, 8)
    kept = recs[recs[:, 4] >= min_area]
    return dict(labels=lab.reshape(h + 2, w2)[1:-1, 1:-1].copy(), num_all=len(recs), kept=kept,
                mask_out=np.where(d, 255, 0).astype(np.uint8))


# ---------------------------------------------------------------- CPU: the checker itself, and the entries' null check

def test_null_context_is_einval(mdx):
    L = mdx.lib()
    m = np.zeros((4, 4), np.uint8)
    n = C.c_int(0)
    assert L.mdx_mask_regions(None, m.ctypes.data_as(C.c_void_p), 4, 4, 4, OPEN3, 1, None, 0, C.byref(n), C.byref(n),
                              None, None) == -1
    assert L.mdx_mask_regions_dev(None, 1, None, 4, 4, 4, 16, OPEN3, 1, None, 0, None, None, None, None) == -1


def test_region_record_is_32_bytes(mdx):
    from motion_detection_amd import _lib
    assert C.sizeof(_lib.MdxRegion) == 32 and _lib.ABI_VERSION >= 7
    assert mdx.RegionResult is not None


def test_checker_diagonal_pair_is_one_component():
    m = np.zeros((3, 3), np.uint8)
    m[0, 0] = m[1, 1] = 255
    r = regions_reference(m, open3=False)
    assert r["num_all"] == 1
    assert r["labels"].tolist() == [[0, -1, -1], [-1, 0, -1], [-1, -1, -1]]
    assert r["kept"].tolist() == [[0, 0, 2, 2, 2, 0, 0, 0]]
    assert regions_reference(m, open3=False, connectivity=4)["num_all"] == 2     # the 4-connected reading fails it


def test_checker_anti_diagonal_and_order():
    m = np.array([[0, 1, 0, 0, 1],
                  [1, 0, 0, 0, 1],
                  [0, 0, 1, 0, 0]], np.uint8)
    r = regions_reference(m, open3=False)
    assert r["labels"].tolist() == [[-1, 0, -1, -1, 1], [0, -1, -1, -1, 1], [-1, -1, 2, -1, -1]]
    assert r["kept"].tolist() == [[0, 0, 2, 2, 2, 1, 0, 0], [4, 0, 1, 2, 2, 4, 0, 1], [2, 2, 1, 1, 1, 2, 2, 2]]
    assert regions_reference(m, open3=False, min_area=2)["kept"][:, 7].tolist() == [0, 1]


def test_checker_opening_edge_blocks():
    """A 2-wide, 3-high block touching the left edge keeps its edge column through the erosion and
    comes back whole; the same block one column in vanishes."""
    m = np.zeros((7, 8), np.uint8)
    m[2:5, 0:2] = 255
    r = regions_reference(m, open3=True)
    assert np.array_equal(r["mask_out"], m) and r["kept"].tolist() == [[0, 2, 2, 3, 6, 0, 2, 0]]
    m = np.zeros((7, 8), np.uint8)
    m[2:5, 1:3] = 255
    r = regions_reference(m, open3=True)
    assert r["num_all"] == 0 and not r["mask_out"].any() and (r["labels"] == -1).all()
    assert regions_reference(m, open3=False)["num_all"] == 1


def test_checker_nested_components_are_all_reported():
    m = np.zeros((7, 7), np.uint8)
    m[0, :] = m[6, :] = m[:, 0] = m[:, 6] = 1
    m[3, 3] = 1
    r = regions_reference(m, open3=False)
    assert r["kept"].tolist() == [[0, 0, 7, 7, 24, 0, 0, 0], [3, 3, 1, 1, 1, 3, 3, 1]]


# ---------------------------------------------------------------- GPU: through the C-ABI

def run_dev(mdx, c, masks, open3=True, min_area=1, max_regions=None, stride=None, frame_stride=None,
            want_labels=True, want_mask=True):
    """mdx_mask_regions_dev on a batch of equal-sized masks; padding bytes are 0xFF, every output
    buffer 0xAA.  Returns the whole buffers, batch-major."""
    B = len(masks)
    h, w = masks[0].shape
    stride = stride or w
    frame_stride = frame_stride or h * stride
    src = np.full(B * frame_stride, 0xFF, np.uint8)
    for i, m in enumerate(masks):
        rows = src[i * frame_stride:i * frame_stride + h * stride].reshape(h, stride)
        rows[:, :w] = m
    cap = ((w + 1) // 2) * ((h + 1) // 2) if max_regions is None else max_regions
    host = dict(regs=np.full((B, max(cap, 1), 8), AA, np.int32), nall=np.full(B, AA, np.int32),
                nkept=np.full(B, AA, np.int32), labels=np.full((B, h, w), AA, np.int32),
                mout=np.full((B, h, w), 0xAA, np.uint8))
    d = {k: c.dev_alloc(v.nbytes) for k, v in host.items()}
    d["src"] = c.dev_alloc(src.nbytes)
    try:
        for k, v in host.items():
            c.h2d(d[k], v)
        c.h2d(d["src"], src)
        c.mask_regions_dev(B, d["src"], w, h, stride, frame_stride, open3, min_area, d["regs"], cap, d["nall"],
                           d["nkept"], d["labels"] if want_labels else 0, d["mout"] if want_mask else 0)
        c.sync()
        for k, v in host.items():
            c.d2h(v, d[k])
        back = np.empty_like(src)
        c.d2h(back, d["src"])
        assert np.array_equal(back, src), "the input mask was modified"
    finally:
        for p in d.values():
            c.dev_free(p)
    host["cap"] = cap
    return host


def same(out, i, ref):
    """Image i of a run_dev result equals the checker's, and nothing past its records was written."""
    assert out["nall"][i] == ref["num_all"]
    assert out["nkept"][i] == len(ref["kept"])
    n = min(len(ref["kept"]), out["cap"])
    assert np.array_equal(out["regs"][i, :n], ref["kept"][:n])
    assert (out["regs"][i, n:] == AA).all()
    assert np.array_equal(out["labels"][i], ref["labels"])
    assert np.array_equal(out["mout"][i], ref["mask_out"])


def patterns(w, h):
    y, x = np.mgrid[0:h, 0:w]
    inset = np.minimum(np.minimum(x, w - 1 - x), np.minimum(y, h - 1 - y))
    corners = np.zeros((h, w), bool)
    corners[[0, 0, h - 1, h - 1], [0, w - 1, 0, w - 1]] = True
    serp = (y % 2 == 0) | ((y % 4 == 1) & (x == w - 1)) | ((y % 4 == 3) & (x == 0))
    lines = np.zeros((h, w), bool)
    lines[h // 2, :] = True
    lines[:, w // 3] = True
    rng = np.random.default_rng(w * 1000 + h)
    p = dict(empty=np.zeros((h, w), bool), full=np.ones((h, w), bool), corners=corners,
             checkerboard=(x + y) % 2 == 1, isolated=(x % 2 == 0) & (y % 2 == 0),
             diagonal=(x * max(h - 1, 1) == y * max(w - 1, 1)) | (x == y),
             anti_diagonal=(x == w - 1 - y) | (x + y == h - 1),
             row=y == h // 2, column=x == w // 2, lines=lines, serpentine=serp,
             thick_serpentine=((y % 8 < 3) | ((y % 16 >= 3) & (y % 16 < 8) & (x >= w - 3)) | ((y % 16 >= 11) & (x < 3))),
             comb=(y == 0) | (x % 2 == 0), thick_comb=(y < 3) | (x % 7 < 3),
             rings=inset % 2 == 0, thick_rings=inset % 8 < 3)
    for dens in (0.05, 0.40, 0.45, 0.60):
        p["random_%.2f" % dens] = rng.random((h, w)) < dens
    return {k: np.where(v, 255, 0).astype(np.uint8) for k, v in p.items()}


SIZES = [(1, 1), (97, 1), (1, 97), (7, 5), (64, 64), (65, 63), (130, 67), (257, 129), (300, 200)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_patterns_equal_the_checker(mdx, ctx, w, h):
    pats = patterns(w, h)
    names = list(pats)
    for open3 in (False, True):
        # the patterns of one size go as one batch: no leakage between them either
        out = run_dev(mdx, ctx, [pats[n] for n in names], open3=open3)
        for i, n in enumerate(names):
            ref = regions_reference(pats[n], open3=open3)
            try:
                same(out, i, ref)
            except AssertionError as e:
                raise AssertionError(f"{n} at {w}x{h}, open3={open3}: {e}") from None
    iso = regions_reference(pats["isolated"], open3=False)
    assert iso["num_all"] == ((w + 1) // 2) * ((h + 1) // 2)                       # the maximum a frame holds
    if w > 1 and h > 1:
        assert regions_reference(pats["checkerboard"], open3=False)["num_all"] == 1  # 8-connected through the diagonals
    if w > 1 and h > 2:
        assert regions_reference(pats["serpentine"], open3=False)["num_all"] == 1  # one deep component


@functools.lru_cache(maxsize=None)
def big_random(dens):
    return np.where(np.random.default_rng(int(dens * 100)).random((480, 640)) < dens, 255, 0).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("dens", [0.05, 0.40, 0.45, 0.60])
def test_random_640x480(mdx, ctx, dens):
    m = big_random(dens)
    for open3 in (False, True):
        ref = regions_reference(m, open3=open3)
        same(run_dev(mdx, ctx, [m], open3=open3), 0, ref)
        if not open3 and dens >= 0.45:
            assert ref["kept"][:, 4].max() > 100000          # the giant component of the statistics pass
        if not open3 and dens == 0.45:
            assert ref["num_all"] > 1000                     # and the many-components case


@pytest.mark.gpu
def test_nested_rings_inner_inside_outer(mdx, ctx):
    m = patterns(65, 63)["rings"]
    out = run_dev(mdx, ctx, [m], open3=False)
    ref = regions_reference(m, open3=False)
    same(out, 0, ref)
    r = out["regs"][0, :out["nkept"][0]]
    assert len(r) >= 10
    for a, b in zip(r[:-1], r[1:]):
        assert a[0] < b[0] and a[1] < b[1] and a[0] + a[2] > b[0] + b[2] and a[1] + a[3] > b[1] + b[3]


@pytest.mark.gpu
@pytest.mark.parametrize("value", [1, 128, 255])
def test_any_nonzero_byte_is_foreground(mdx, ctx, value):
    m = (patterns(130, 67)["random_0.60"] // 255 * value).astype(np.uint8)
    for open3 in (False, True):
        same(run_dev(mdx, ctx, [m], open3=open3), 0, regions_reference(m, open3=open3))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,stride,extra", [(130, 67, 160, 0), (65, 63, 65, 100), (97, 1, 128, 64), (7, 5, 9, 3)])
def test_padding_is_never_foreground(mdx, ctx, w, h, stride, extra):
    """stride > w and frame_stride > h*stride with 0xFF in the padding."""
    masks = [patterns(w, h)[n] for n in ("random_0.40", "empty", "corners")]
    for open3 in (False, True):
        out = run_dev(mdx, ctx, masks, open3=open3, stride=stride, frame_stride=h * stride + extra)
        for i, m in enumerate(masks):
            same(out, i, regions_reference(m, open3=open3))


@pytest.mark.gpu
def test_batch_of_three_does_not_leak(mdx, ctx):
    p = patterns(257, 129)
    masks = [p["empty"], p["full"], p["random_0.45"]]
    for open3 in (False, True):
        out = run_dev(mdx, ctx, masks, open3=open3)
        for i, m in enumerate(masks):
            same(out, i, regions_reference(m, open3=open3))
    assert out["nall"].tolist()[:2] == [0, 1]


@pytest.mark.gpu
def test_small_call_after_large_sees_no_stale_scratch(mdx):
    with mdx.Context(0, 320, 240, 1) as c:
        big, small = patterns(300, 200)["random_0.60"], patterns(7, 5)["checkerboard"]
        same(run_dev(mdx, c, [big], open3=False), 0, regions_reference(big, open3=False))
        same(run_dev(mdx, c, [small], open3=False), 0, regions_reference(small, open3=False))
        same(run_dev(mdx, c, [big], open3=True), 0, regions_reference(big, open3=True))


@pytest.mark.gpu
def test_min_area_keeps_equal_drops_below(mdx, ctx):
    m = patterns(130, 67)["random_0.40"]
    areas = np.unique(regions_reference(m, open3=False)["kept"][:, 4])
    a = int(areas[len(areas) // 2])                          # an area some component has
    assert a > 1
    for min_area in (-5, 0, 1, a, a + 1):
        ref = regions_reference(m, open3=False, min_area=min_area)
        out = run_dev(mdx, ctx, [m], open3=False, min_area=min_area)
        same(out, 0, ref)
        ids = out["regs"][0, :len(ref["kept"]), 7]
        assert np.all(np.diff(ids) > 0)                      # ascending id among ALL components
    at = regions_reference(m, open3=False, min_area=a)["kept"][:, 4]
    above = regions_reference(m, open3=False, min_area=a + 1)["kept"][:, 4]
    assert (at == a).any() and not (above == a).any()


@pytest.mark.gpu
@pytest.mark.parametrize("max_regions", [0, 1, 5])
def test_max_regions_below_num_kept(mdx, ctx, max_regions):
    m = patterns(130, 67)["random_0.40"]
    ref = regions_reference(m, open3=False)
    assert len(ref["kept"]) > 5
    out = run_dev(mdx, ctx, [m, m], open3=False, max_regions=max_regions)
    for i in range(2):
        same(out, i, ref)                                    # num_kept is the full count; the rest stays 0xAA


@pytest.mark.gpu
def test_host_entry_and_python_wrapper(mdx, ctx):
    m = patterns(257, 129)["random_0.60"]
    for open3 in (False, True):
        ref = regions_reference(m, open3=open3, min_area=4)
        r = ctx.mask_regions(m, open3=open3, min_area=4, want_labels=True, want_mask=True)
        assert isinstance(r, mdx.RegionResult)
        assert (r.num_all, r.num_kept) == (ref["num_all"], len(ref["kept"]))
        assert np.array_equal(r.regions, ref["kept"]) and np.array_equal(r.labels, ref["labels"])
        assert np.array_equal(r.mask_out, ref["mask_out"])
        assert r.rectangles == [tuple(k[:4]) for k in ref["kept"].tolist()]
        q = ctx.mask_regions(m[:, 3:200], open3=open3, min_area=4, max_regions=2)     # a strided view: stride > w
        ref = regions_reference(m[:, 3:200], open3=open3, min_area=4)
        assert q.num_kept == len(ref["kept"]) > 2 and np.array_equal(q.regions, ref["kept"][:2])
        assert q.labels is None and q.mask_out is None


@pytest.mark.gpu
def test_einval_cases(mdx, ctx):
    L = mdx.lib()
    w, h = 16, 8
    d = ctx.dev_alloc(4096)
    host = np.zeros((h, w), np.uint8)
    hp = host.ctypes.data_as(C.c_void_p)
    try:
        vp = C.c_void_p
        ok = dict(batch=1, mask=vp(d), w=w, h=h, stride=w, frame_stride=w * h, flags=OPEN3, min_area=1,
                  regions=vp(d + 1024), max_regions=4, nall=None, nkept=None, labels=None, mask_out=vp(d + 2048))

        def dev(**kw):
            a = dict(ok, **kw)
            return L.mdx_mask_regions_dev(ctx._h, a["batch"], a["mask"], a["w"], a["h"], a["stride"], a["frame_stride"],
                                          a["flags"], a["min_area"], a["regions"], a["max_regions"], a["nall"],
                                          a["nkept"], a["labels"], a["mask_out"])

        def hst(**kw):
            a = dict(ok, mask=hp, regions=None, max_regions=0, mask_out=None)
            a.update(kw)
            return L.mdx_mask_regions(ctx._h, a["mask"], a["w"], a["h"], a["stride"], a["flags"], a["min_area"],
                                      a["regions"], a["max_regions"], None, None, a["labels"], a["mask_out"])
        assert dev() == 0 and hst() == 0
        ctx.sync()
        bad = [dict(batch=0), dict(batch=-1), dict(w=0), dict(h=0), dict(w=-3), dict(stride=w - 1),
               dict(frame_stride=w * h - 1), dict(w=1 << 16, h=(1 << 14) + 1, stride=1 << 16, frame_stride=1 << 31),
               dict(max_regions=-1), dict(regions=None, max_regions=1), dict(flags=2), dict(flags=OPEN3 | 4),
               dict(mask_out=vp(d))]
        for kw in bad:
            assert dev(**kw) == -1, kw
            assert b"mdx_mask_regions_dev" in L.mdx_last_error(ctx._h)
        for kw in [dict(w=0), dict(h=-1), dict(stride=w - 1), dict(w=1 << 16, h=(1 << 14) + 1, stride=1 << 16),
                   dict(max_regions=-1), dict(regions=None, max_regions=1), dict(flags=8), dict(mask_out=hp)]:
            assert hst(**kw) == -1, kw
        assert dev(regions=None, max_regions=0) == 0         # no records wanted: NULL is fine
        ctx.sync()
    finally:
        ctx.dev_free(d)


# ---------------------------------------------------------------- end to end: chained behind the pair entry

def _chain(mdx, seeds, pipelining):
    """mdx_flow_warp_diff_batch_dev then mdx_mask_regions_dev on the same stream with no sync in
    between; one sync; the regions against the checker run on the device mask."""
    w, h, B = 160, 120, len(seeds)
    pairs = [mdx.synth_pair(s, w, h, 1) for s in seeds]
    if seeds[0] == 20141105:
        g = np.load(os.path.join(ROOT, "tests", "golden", "synth_160x120_gray.npz"))
        assert np.array_equal(pairs[0][0], g["img1"]) and np.array_equal(pairs[0][1], g["img2"])
    g1 = np.stack([p[0] for p in pairs])
    g2 = np.stack([p[1] for p in pairs])
    Hs = np.stack([p[2] for p in pairs]).astype(np.float64)
    cap = 64
    with mdx.Context(0, w, h, B, fit_mode=mdx.FIT_EXTERNAL, thresh=30, call_pipelining=pipelining) as c:
        n = mdx.grid_count(w, h, c.params.pixel_step)
        host = dict(regs=np.full((B, cap, 8), AA, np.int32), nall=np.full(B, AA, np.int32),
                    nkept=np.full(B, AA, np.int32), mask=np.full((B, h, w), 0xAA, np.uint8))
        d = {k: c.dev_alloc(v.nbytes) for k, v in host.items()}
        d.update(i1=c.dev_alloc(g1.nbytes), i2=c.dev_alloc(g2.nbytes), H=c.dev_alloc(Hs.nbytes), np=c.dev_alloc(B * n * 8),
                 st=c.dev_alloc(B * n))
        try:
            for k, v in host.items():
                c.h2d(d[k], v)
            c.h2d(d["i1"], g1), c.h2d(d["i2"], g2), c.h2d(d["H"], Hs)
            c.flow_warp_diff_batch_dev(B, d["i1"], d["i2"], w, h, w, w * h, mdx.FMT_GRAY8, d["np"], d["st"], 0,
                                       d["mask"], 0, d["H"], 0)
            c.mask_regions_dev(B, d["mask"], w, h, w, w * h, True, 50, d["regs"], cap, d["nall"], d["nkept"])
            c.sync()
            for k, v in host.items():
                c.d2h(v, d[k])
        finally:
            for p in d.values():
                c.dev_free(p)
    for i in range(B):
        assert set(np.unique(host["mask"][i])) <= {0, 255}
        ref = regions_reference(host["mask"][i], open3=True, min_area=50)
        assert host["nall"][i] == ref["num_all"] and host["nkept"][i] == len(ref["kept"])
        assert host["nkept"][i] >= 1                         # else the comparison is vacuous
        assert np.array_equal(host["regs"][i, :len(ref["kept"])], ref["kept"])
        assert (host["regs"][i, len(ref["kept"]):] == AA).all()


@pytest.mark.gpu
def test_chained_behind_the_pair_entry(mdx):
    _chain(mdx, [20141105], 0)


@pytest.mark.gpu
def test_chained_batch_of_three_pipelined(mdx):
    _chain(mdx, [20141105, 20141106, 20141107], 1)
