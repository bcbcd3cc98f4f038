"""Convex hulls of the mask regions on the device (mdx_region_hulls_dev / mdx_mask_region_hulls).

What the node takes from a blob next to its boundingRect is cv::convexHull (reference
common/src/optical_flow_visualizer.cpp:204-240); the hull of a blob's contour is the hull of its pixels,
so the vertex set is determined mathematically.  The start and the orientation are mdx_cluster_hulls'
(cv::convexHull(.., clockwise=false) as restated there) and, like them, unpinned against a real build.

The checker is two pieces already in the tree, neither of which shares anything with the kernels:
test_regions.regions_reference (a flood fill) gives the label image and the kept records, and
test_hulls.hull_oracle (Andrew's monotone chain on Python ints) is applied to the pixels of each label.
Everything is integer and exact: every output buffer is prefilled with 0xAA words and every word of it
is compared, `offsets` past the records that take part and `xy` past the last vertex included.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_hulls import hull_oracle, upper_rounds
from test_regions import AA, OPEN3, ROOT, big_random, patterns, regions_reference


# ---------------------------------------------------------------- the checker

def clamp_box(rec, w, h):
    x, y, wd, ht = (int(v) for v in rec[:4])
    x0, y0 = min(max(x, 0), w), min(max(y, 0), h)
    return x0, y0, min(max(x + wd, x0), w), min(max(y + ht, y0), h)


def expected_hulls(labels, recs):
    """hull_oracle of each record's members: the pixels inside its rectangle (clamped to the frame)
    whose label is its id."""
    h, w = labels.shape
    ys, xs = np.nonzero(labels >= 0)
    lab = labels[ys, xs]
    order = np.argsort(lab, kind="stable")
    ys, xs, lab = ys[order], xs[order], lab[order]
    out = []
    for rec in np.asarray(recs).reshape(-1, 8):
        x0, y0, x1, y1 = clamp_box(rec, w, h)
        a, b = np.searchsorted(lab, [rec[7], rec[7] + 1]) if rec[7] >= 0 else (0, 0)
        mx, my = xs[a:b], ys[a:b]
        inside = (mx >= x0) & (mx < x1) & (my >= y0) & (my < y1)
        pts = list(zip(mx[inside].tolist(), my[inside].tolist()))
        out.append(hull_oracle(pts) if pts else [])
    return out


def tail_mask():
    """49 columns x 1133 rows, one solid region: column x < 48 holds rows 0 .. B - x(x-1)/2 with
    B = 48*47/2 + 2 = 1130, column 48 rows 0 .. B + 2.  Its max-y profile loses one candidate per
    simultaneous round, beyond kHullRounds = 32: the sequential tail finishes it."""
    B = 48 * 47 // 2 + 2
    m = np.zeros((B + 3, 49), np.uint8)
    for x in range(48):
        m[:B - x * (x - 1) // 2 + 1, x] = 255
    m[:, 48] = 255
    return m


TAIL_HULL = [(48, 1132), (0, 1130), (0, 0), (48, 0)]


# ---------------------------------------------------------------- CPU

def test_header_and_binding_declare_both_entries(mdx):
    from test_abi import HEADER, header_functions
    names = header_functions()
    for n in ("mdx_region_hulls_dev", "mdx_mask_region_hulls"):
        assert n in names and n in mdx._lib.EXPORTED
    assert sorted(mdx._lib.EXPORTED) == names
    hdr = open(HEADER).read()
    assert int(re.search(r"#define MDX_ABI_VERSION (\d+)", hdr).group(1)) == mdx._lib.ABI_VERSION == 11
    assert C.sizeof(mdx._lib.MdxParams) == 80


def test_null_context_is_einval(mdx):
    L = mdx.lib()
    m = np.zeros((4, 4), np.uint8)
    off = np.zeros(2, np.int32)
    n = C.c_int(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert L.mdx_region_hulls_dev(None, 1, p(off), 4, 4, None, 0, None, p(off), None, 0, None) == mdx._lib.MDX_EINVAL
    assert L.mdx_mask_region_hulls(None, p(m), 4, 4, 4, OPEN3, 1, None, 0, C.byref(n), C.byref(n), p(off), None, 0,
                                   C.byref(n)) == mdx._lib.MDX_EINVAL


def test_hulls_field_is_last_and_defaults(mdx):
    import dataclasses
    from motion_detection_amd.node import MotionDetectionNode
    z = np.zeros((0, 8), np.int32)
    assert dataclasses.fields(mdx.RegionResult)[-1].name == "hulls"
    assert mdx.RegionResult(z, 0, 0).hulls is None
    assert mdx.RegionResult(z, 0, 0, None, None).hulls is None          # positional construction is unchanged
    assert '"region_contours": False' in inspect.getsource(MotionDetectionNode.__init__)
    assert list(mdx.FlowResult.__dataclass_fields__)[-1] == "contours"  # nothing was added behind it


def test_tail_mask_is_what_it_claims():
    m = tail_mask()
    assert m.shape == (1133, 49)
    ref = regions_reference(m, open3=False)
    assert ref["num_all"] == 1 and ref["kept"][0, :4].tolist() == [0, 0, 49, 1133]
    assert (m[0] != 0).all() and all(m[:, x].sum() // 255 == np.flatnonzero(m[:, x]).max() + 1 for x in range(49))  # solid
    profile = [(x, int(np.flatnonzero(m[:, x]).max())) for x in range(49)]
    rounds = upper_rounds(profile, 60)
    assert rounds == [1] * 47                                # one candidate per round, 47 rounds
    assert len(rounds) >= 40                                 # above kHullRounds = 32
    assert expected_hulls(ref["labels"], ref["kept"]) == [TAIL_HULL]


def test_checker_filters_by_label_and_clamps():
    m = np.zeros((7, 7), np.uint8)
    m[0, :] = m[6, :] = m[:, 0] = m[:, 6] = 1
    m[3, 3] = 1
    ref = regions_reference(m, open3=False)
    assert expected_hulls(ref["labels"], ref["kept"]) == [[(6, 6), (0, 6), (0, 0), (6, 0)], [(3, 3)]]
    rec = ref["kept"][0].copy()
    rec[:4] = [-3, 2, 5, 100]                                # columns 0..1, rows 2..6 of the ring
    assert expected_hulls(ref["labels"], [rec]) == [[(1, 6), (0, 6), (0, 2)]]
    rec[7] = 5
    assert expected_hulls(ref["labels"], [rec]) == [[]]


def test_write_contour_lines_of_a_region_hull(tmp_path, mdx):
    """frame, id, x, y, ... of a region's hull in the Python logger and in host/'s MotionLogger."""
    import shutil
    import subprocess
    from motion_detection_amd.formats import MotionLogger
    from node_io import HOST
    m = np.zeros((5, 6), np.uint8)
    m[1:4, 1:5] = 255
    m[2, 0] = 255
    ref = regions_reference(m, open3=False)
    hull = np.array(expected_hulls(ref["labels"], ref["kept"])[0], np.int32)
    assert hull.tolist() == [[4, 3], [1, 3], [0, 2], [1, 1], [4, 1]]
    lg = MotionLogger(str(tmp_path / "py_log"))
    lg.writeBoundingBox(tuple(ref["kept"][0, :4].tolist()), 7, 0)
    lg.writeContour(hull, 7, 0)
    lg.close()
    assert (tmp_path / "py_log").read_text() == "7, 0, 0, 1, 5, 4\n7, 0, 4, 3, 1, 3, 0, 2, 1, 1, 4, 1\n"
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    src = tmp_path / "c.cpp"
    src.write_text('#include "mdx_host.h"\nint main(int, char** argv) { mdx_host::MotionLogger lg(argv[1]); '
                   "lg.write_bounding_box(0, 1, 5, 3, 7, 0); "
                   "lg.write_contour({4, 3, 1, 3, 0, 2, 1, 1, 4, 1}, 7, 0); return 0; }\n")
    libdir = os.path.join(ROOT, "motion_detection_amd", "lib")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", HOST, "-I", os.path.join(ROOT, "include"), str(src),
                    os.path.join(HOST, "mdx_host.cpp"), "-L", libdir, "-lmdx", f"-Wl,-rpath,{libdir}", "-o",
                    str(tmp_path / "c")], check=True)
    subprocess.run([str(tmp_path / "c"), str(tmp_path / "cpp_log")], check=True)
    assert (tmp_path / "cpp_log").read_bytes() == (tmp_path / "py_log").read_bytes()


# ---------------------------------------------------------------- GPU: through the C-ABI

def run_chain(c, masks, open3=False, min_area=1, max_regions=None, max_vertices=None, xy_null=False, edit=None,
              stride=None):
    """mdx_mask_regions_dev then mdx_region_hulls_dev on a batch of equal-sized masks, on one stream with one
    sync at the end; every output buffer 0xAA.  edit(regs, nkept), when given, changes the records on the
    device between the two calls (the one case with a sync in between).  Returns the whole buffers."""
    B = len(masks)
    h, w = masks[0].shape
    stride = stride or w
    src = np.full((B, h, stride), 0xFF, np.uint8)
    for i, m in enumerate(masks):
        src[i, :, :w] = m
    cap = ((w + 1) // 2) * ((h + 1) // 2) if max_regions is None else max_regions
    maxv = min(w * h, 2 * min(w, h) * cap) + 8 if max_vertices is None else max_vertices
    host = dict(regs=np.full((B, max(cap, 1), 8), AA, np.int32), nall=np.full(B, AA, np.int32),
                nkept=np.full(B, AA, np.int32), labels=np.full((B, h, w), AA, np.int32),
                offsets=np.full((B, cap + 1), AA, np.int32), xy=np.full((B, max(maxv, 1), 2), AA, np.int32),
                nv=np.full(B, AA, np.int32))
    d = {k: c.dev_alloc(v.nbytes) for k, v in host.items()}
    d["src"] = c.dev_alloc(src.nbytes)
    try:
        for k, v in host.items():
            c.h2d(d[k], v)
        c.h2d(d["src"], src)
        c.mask_regions_dev(B, d["src"], w, h, stride, h * stride, open3, min_area, d["regs"], cap, d["nall"], d["nkept"],
                           d["labels"], 0)
        if edit is not None:
            c.sync()
            c.d2h(host["regs"], d["regs"]), c.d2h(host["nkept"], d["nkept"])
            edit(host["regs"], host["nkept"])
            c.h2d(d["regs"], host["regs"]), c.h2d(d["nkept"], host["nkept"])
        c.region_hulls_dev(B, d["labels"], w, h, d["regs"], cap, d["nkept"], d["offsets"], 0 if xy_null else d["xy"], maxv,
                           d["nv"])
        c.sync()
        for k, v in host.items():
            c.d2h(v, d[k])
    finally:
        for p in d.values():
            c.dev_free(p)
    host.update(cap=cap, maxv=maxv)
    return host


def same(out, i, ref, hulls=None):
    """Image i of a run_chain result: the records equal the checker's, and every word of offsets, xy and
    num_vertices equals the oracle's hulls of the records that take part.  Returns the hulls."""
    cap, maxv = out["cap"], out["maxv"]
    r = min(len(ref["kept"]), cap)
    if hulls is None:
        assert out["nkept"][i] == len(ref["kept"])
        assert np.array_equal(out["regs"][i, :r], ref["kept"][:r])
        assert np.array_equal(out["labels"][i], ref["labels"])
        hulls = expected_hulls(ref["labels"], ref["kept"][:r])
    assert len(hulls) == r
    ends = np.cumsum([0] + [len(v) for v in hulls])
    want_off = np.concatenate([ends, np.full(cap - r, ends[-1])]).astype(np.int32)
    assert np.array_equal(out["offsets"][i], want_off), (out["offsets"][i][:r + 2], want_off[:r + 2])
    assert out["nv"][i] == ends[-1]
    flat = np.array([p for v in hulls for p in v], np.int32).reshape(-1, 2)
    m = min(len(flat), maxv)
    assert np.array_equal(out["xy"][i, :m], flat[:m])
    assert (out["xy"][i, m:] == AA).all()
    return hulls


def one(ctx, mask, open3=False, **kw):
    ref = regions_reference(mask, open3=open3, min_area=kw.get("min_area", 1))
    return same(run_chain(ctx, [mask], open3=open3, **kw), 0, ref)


def full(w, h):
    return np.full((h, w), 255, np.uint8)


@pytest.mark.gpu
def test_degenerate_shapes(ctx):
    assert one(ctx, full(1, 1)) == [[(0, 0)]]
    assert one(ctx, full(97, 1)) == [[(96, 0), (0, 0)]]
    assert one(ctx, full(1, 97)) == [[(0, 96), (0, 0)]]      # one column, two distinct y: the nl == 1 branch
    assert one(ctx, full(7, 5)) == [[(6, 4), (0, 4), (0, 0), (6, 0)]]
    eye = np.eye(64, dtype=np.uint8) * 255
    assert one(ctx, eye) == [[(63, 63), (0, 0)]]             # every member collinear
    assert one(ctx, eye[::-1].copy()) == [[(63, 0), (0, 63)]]
    corners = one(ctx, patterns(65, 63)["corners"])
    assert corners == [[(0, 0)], [(64, 0)], [(0, 62)], [(64, 62)]]


def combs(w=41, h=21):
    """Two interleaved combs.  Two 8-connected components cannot share a rectangle exactly (one that
    touches its left and right side separates top from bottom), so these overlap in all but two rows:
    A hangs from the top row with teeth at x % 4 == 0, B stands on the bottom row with teeth at
    x % 4 == 2; every tooth crosses the other comb's rectangle."""
    y, x = np.mgrid[0:h, 0:w]
    a = (y == 0) | ((x % 4 == 0) & (y <= h - 3))
    b = (y == h - 1) | ((x % 4 == 2) & (y >= 2))
    return np.where(a | b, 255, 0).astype(np.uint8)


@pytest.mark.gpu
def test_label_filter_nested_and_interleaved(ctx):
    rings = patterns(65, 63)["rings"]
    hulls = one(ctx, rings)
    assert len(hulls) >= 10
    assert hulls[0] == [(64, 62), (0, 62), (0, 0), (64, 0)]  # the outer ring ignores everything inside it
    assert hulls[1] == [(62, 60), (2, 60), (2, 2), (62, 2)]
    m = combs()
    ref = regions_reference(m, open3=False)
    assert ref["kept"][:, :4].tolist() == [[0, 0, 41, 19], [0, 2, 41, 19]]
    hulls = one(ctx, m)
    assert hulls == [[(40, 18), (0, 18), (0, 0), (40, 0)], [(40, 20), (0, 20), (2, 2), (38, 2)]]
    cb = patterns(65, 63)["checkerboard"]
    assert regions_reference(cb, open3=False)["num_all"] == 1
    one(ctx, cb)                                             # one 8-connected component: against the oracle


def jagged(w):
    y, x = np.mgrid[0:3, 0:w]
    return np.where(y >= x % 3, 255, 0).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("w", [63, 64, 65, 1023, 1024, 1025, 8192])
def test_full_width_region_at_word_edges(ctx, w):
    m = jagged(w)
    hulls = one(ctx, m, max_regions=4)
    assert len(hulls) == 1 and hulls[0][0] == (w - 1, 2) and (0, 0) in hulls[0]


@pytest.mark.gpu
def test_width_beyond_the_span_is_einval(ctx, mdx):
    L = mdx.lib()
    d = ctx.dev_alloc(8193 * 4 + 64)
    try:
        ctx.h2d(d, np.full(8193 + 16, AA, np.int32))
        v = C.c_void_p
        assert L.mdx_region_hulls_dev(ctx._h, 1, v(d), 8193, 1, None, 0, None, v(d + 8193 * 4), None, 0, None) == -1
        assert b"mdx_region_hulls_dev" in L.mdx_last_error(ctx._h)
        assert L.mdx_region_hulls_dev(ctx._h, 1, v(d), 8192, 1, None, 0, None, v(d + 8193 * 4), None, 0, None) == 0
        ctx.sync()
        back = np.empty(8193 + 16, np.int32)
        ctx.d2h(back, d)
        assert back[8193] == 0 and (np.delete(back, 8193) == AA).all()
    finally:
        ctx.dev_free(d)


@pytest.mark.gpu
def test_row_strips_and_frame_edges(ctx):
    m = np.zeros((600, 9), np.uint8)                         # 3 columns, 600 rows: the lanes fold into row strips
    m[5:598, 3] = m[0:600, 4] = m[17:411, 5] = 255
    assert one(ctx, m) == [[(5, 410), (4, 599), (3, 597), (3, 5), (4, 0), (5, 17)]]
    m = np.zeros((200, 300), np.uint8)                       # touches all four frame edges
    m[100, :] = m[:, 150] = 255
    m[90:111, 140:161] = 255
    hulls = one(ctx, m)
    assert len(hulls) == 1 and {(299, 100), (150, 199), (0, 100), (150, 0)} <= set(hulls[0])


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(7, 5), (65, 63), (130, 67), (257, 129), (300, 200)])
def test_patterns_end_to_end(ctx, w, h):
    pats = patterns(w, h)
    names = list(pats)
    for open3 in (False, True):
        out = run_chain(ctx, [pats[n] for n in names], open3=open3)    # one batch: no leakage between them either
        for i, n in enumerate(names):
            try:
                same(out, i, regions_reference(pats[n], open3=open3))
            except AssertionError as e:
                raise AssertionError(f"{n} at {w}x{h}, open3={open3}: {e}") from None


@pytest.mark.gpu
@pytest.mark.parametrize("dens", [0.05, 0.45])
def test_random_640x480(ctx, dens):
    m = big_random(dens)
    for open3 in (False, True):
        ref = regions_reference(m, open3=open3, min_area=20)
        same(run_chain(ctx, [m], open3=open3, min_area=20), 0, ref)
        if not open3 and dens == 0.45:
            assert ref["kept"][:, 4].max() > 100000          # a frame-wide blob among many small ones


@pytest.mark.gpu
def test_many_vertices_disc(ctx):
    y, x = np.mgrid[0:257, 0:257]
    m = np.where((x - 128) ** 2 + (y - 128) ** 2 <= 120 * 120, 255, 0).astype(np.uint8)
    hulls = one(ctx, m, max_regions=3)
    assert len(hulls) == 1 and len(hulls[0]) > 60            # the count itself is the oracle's


@pytest.mark.gpu
@pytest.mark.parametrize("flip", ["none", "v", "h", "vh"])
def test_through_the_sequential_tail(ctx, flip):
    m = tail_mask()
    if "v" in flip:
        m = m[::-1]                                          # the min-y chain
    if "h" in flip:
        m = m[:, ::-1]
    hulls = one(ctx, np.ascontiguousarray(m), max_regions=2)
    if flip == "none":
        assert hulls == [TAIL_HULL]
    assert len(hulls[0]) == 4


@pytest.mark.gpu
def test_batch_of_three_does_not_leak(ctx):
    p = patterns(257, 129)
    masks = [p["empty"], p["full"], p["random_0.45"]]
    out = run_chain(ctx, masks)
    for i, m in enumerate(masks):
        same(out, i, regions_reference(m, open3=False))
    assert out["nv"].tolist()[:2] == [0, 4]


@pytest.mark.gpu
def test_small_call_after_large_and_twice_the_same(mdx):
    with mdx.Context(0, 320, 240, 1) as c:
        big, small = patterns(300, 200)["random_0.60"], patterns(7, 5)["checkerboard"]
        a = run_chain(c, [big])
        same(a, 0, regions_reference(big, open3=False))
        same(run_chain(c, [small]), 0, regions_reference(small, open3=False))
        b = run_chain(c, [big])
        for k in ("regs", "nkept", "labels", "offsets", "xy", "nv"):
            assert a[k].tobytes() == b[k].tobytes(), k       # the same call twice: identical bytes


@pytest.mark.gpu
@pytest.mark.parametrize("max_regions", [0, 1, 5])
def test_max_regions_below_num_kept(ctx, max_regions):
    m = patterns(130, 67)["random_0.40"]
    ref = regions_reference(m, open3=False)
    assert len(ref["kept"]) > 5
    out = run_chain(ctx, [m, m], max_regions=max_regions)
    for i in range(2):
        assert len(same(out, i, ref)) == max_regions         # the written records' hulls only; offsets complete
        assert (out["regs"][i, max_regions:] == AA).all()


@pytest.mark.gpu
def test_max_vertices_cuts_inside_a_hull(ctx):
    m = patterns(130, 67)["random_0.40"]
    ref = regions_reference(m, open3=False)
    hulls = expected_hulls(ref["labels"], ref["kept"])
    j = next(i for i, v in enumerate(hulls) if len(v) >= 4)
    cut = sum(len(v) for v in hulls[:j]) + 2                 # two vertices into hull j
    out = run_chain(ctx, [m], max_vertices=cut)
    same(out, 0, ref)
    assert out["nv"][0] == sum(len(v) for v in hulls) > cut  # the full total
    out = run_chain(ctx, [m], max_vertices=0, xy_null=True)
    same(out, 0, ref)
    assert (out["xy"] == AA).all()


@pytest.mark.gpu
def test_records_edited_on_the_device(ctx):
    m = patterns(130, 67)["thick_rings"]
    ref = regions_reference(m, open3=False)
    assert len(ref["kept"]) >= 3
    edited = {}

    def edit(regs, nkept):
        regs[0, 0, :4] = [-40, 5, 100, 1 << 30]              # leaves the frame on the left and below
        regs[0, 1, :4] = [60, -(1 << 30), (1 << 31) - 61, (1 << 30) + 40]   # width past w, y far above
        regs[0, 2, 7] = ref["num_all"] + 1000                # an id no pixel has
        edited["recs"] = regs[0, :len(ref["kept"])].copy()
    out = run_chain(ctx, [m], edit=edit)
    hulls = expected_hulls(ref["labels"], edited["recs"])
    assert hulls[2] == [] and len(hulls[0]) >= 3 and len(hulls[1]) >= 3
    assert all(x < 60 for x, _ in hulls[0]) and all(x >= 60 and y < 40 for x, y in hulls[1])
    same(out, 0, ref, hulls=hulls)
    assert np.array_equal(out["labels"][0], ref["labels"])   # nothing else was written


@pytest.mark.gpu
def test_equals_cluster_hulls_on_the_same_pixels(ctx):
    m = patterns(130, 67)["random_0.45"]
    ref = regions_reference(m, open3=False, min_area=3)
    hulls = same(run_chain(ctx, [m], min_area=3), 0, ref)
    ys, xs = np.nonzero(ref["labels"] >= 0)
    pts = np.stack([xs, ys], 1).astype(np.float32)
    got = ctx.cluster_hulls(pts, ref["labels"][ys, xs], ref["kept"][:, 7])
    assert len(got) == len(hulls) > 10
    for a, b in zip(got, hulls):
        assert a.tolist() == [list(p) for p in b]


@pytest.mark.gpu
def test_host_entry_and_python_wrapper(mdx, ctx):
    L = mdx.lib()
    m = patterns(257, 129)["random_0.60"]
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    for open3 in (False, True):
        ref = regions_reference(m, open3=open3, min_area=4)
        dev = run_chain(ctx, [m], open3=open3, min_area=4)
        hulls = same(dev, 0, ref)
        k = len(ref["kept"])
        r = ctx.mask_regions(m, open3=open3, min_area=4, want_hulls=True)
        assert (r.num_all, r.num_kept) == (ref["num_all"], k) and np.array_equal(r.regions, ref["kept"])
        assert len(r.hulls) == k and all(a.dtype == np.int32 and a.tolist() == [list(q) for q in b]
                                         for a, b in zip(r.hulls, hulls))
        assert ctx.mask_regions(m, open3=open3, min_area=4).hulls is None
        # the raw entry on a pitched view with 0xFF padding, every word of its outputs
        pitched = np.full((129, 300), 0xFF, np.uint8)
        pitched[:, :257] = m
        cap, maxv = k + 3, int(dev["nv"][0]) + 5
        regs, off = np.full((cap, 8), AA, np.int32), np.full(cap + 1, AA, np.int32)
        xy = np.full((maxv, 2), AA, np.int32)
        nall, nkept, nv = C.c_int(-5), C.c_int(-5), C.c_int(-5)
        assert L.mdx_mask_region_hulls(ctx._h, p(pitched), 257, 129, 300, OPEN3 if open3 else 0, 4, p(regs), cap,
                                       C.byref(nall), C.byref(nkept), p(off), p(xy), maxv, C.byref(nv)) == 0
        assert (nall.value, nkept.value, nv.value) == (ref["num_all"], k, dev["nv"][0])
        assert np.array_equal(regs[:k], ref["kept"]) and (regs[k:] == AA).all()
        assert np.array_equal(off, np.concatenate([dev["offsets"][0, :k + 1], [nv.value] * 3]))
        assert np.array_equal(xy[:nv.value], dev["xy"][0, :nv.value]) and (xy[nv.value:] == AA).all()
        # cut short: only the vertices that exist and fit come back
        xy[:] = AA
        assert L.mdx_mask_region_hulls(ctx._h, p(pitched), 257, 129, 300, OPEN3 if open3 else 0, 4, p(regs), cap, None,
                                       None, p(off), p(xy), 7, C.byref(nv)) == 0
        assert nv.value == dev["nv"][0] and np.array_equal(xy[:7], dev["xy"][0, :7]) and (xy[7:] == AA).all()


@pytest.mark.gpu
def test_einval_cases_leave_the_outputs_untouched(mdx, ctx):
    L = mdx.lib()
    w, h, M, V = 16, 8, 4, 32
    m = patterns(w, h)["thick_comb"]
    vp = C.c_void_p
    out = run_chain(ctx, [m], max_regions=M, max_vertices=V)          # a good call's outputs, to start from
    words = 4096
    d = ctx.dev_alloc(words * 4)
    try:
        img = np.full(words, AA, np.int32)
        img[:w * h] = out["labels"][0].ravel()
        img[1024:1024 + 8 * M] = out["regs"][0].ravel()
        img[1100] = out["nkept"][0]
        ctx.h2d(d, img)
        lab, rec, nk, off, xy, nv = (vp(d + 4 * o) for o in (0, 1024, 1100, 2048, 2100, 2090))
        ok = dict(batch=1, labels=lab, w=w, h=h, regions=rec, max_regions=M, num_kept=nk, offsets=off, xy=xy,
                  max_vertices=V, nv=nv)

        def dev(**kw):
            a = dict(ok, **kw)
            return L.mdx_region_hulls_dev(ctx._h, a["batch"], a["labels"], a["w"], a["h"], a["regions"], a["max_regions"],
                                          a["num_kept"], a["offsets"], a["xy"], a["max_vertices"], a["nv"])
        bad = [dict(batch=0), dict(batch=-1), dict(w=0), dict(h=0), dict(w=-3), dict(w=1 << 13, h=(1 << 17) + 1),
               dict(w=8193, h=1), dict(max_regions=-1), dict(max_vertices=-1), dict(labels=None), dict(offsets=None),
               dict(regions=None), dict(num_kept=None), dict(xy=None)]
        for kw in bad:
            assert dev(**kw) == -1, kw
            assert b"mdx_region_hulls_dev" in L.mdx_last_error(ctx._h)
        ctx.sync()
        back = np.empty_like(img)
        ctx.d2h(back, d)
        assert np.array_equal(back, img)                              # no rejected call wrote anything
        assert dev(regions=None, num_kept=None, max_regions=0, xy=None, max_vertices=0) == 0   # nothing wanted: NULLs are fine
        assert dev() == 0
        ctx.sync()
        ctx.d2h(back, d)
        assert np.array_equal(back[2048:2048 + M + 1], out["offsets"][0]) and back[2090] == out["nv"][0]
        assert np.array_equal(back[2100:2100 + 2 * V], out["xy"][0].ravel())
        back[2048:2048 + M + 1] = back[2090] = back[2100:2100 + 2 * V] = AA
        assert np.array_equal(back, img)                              # and nothing else
    finally:
        ctx.dev_free(d)
    # the host entry: mdx_mask_regions' errors plus its own
    p = lambda a: a.ctypes.data_as(vp)   # noqa: E731
    regs, offs, pts = np.full((M, 8), AA, np.int32), np.full(M + 1, AA, np.int32), np.full((V, 2), AA, np.int32)
    cnt = [C.c_int(-5) for _ in range(3)]
    okh = dict(mask=p(m), w=w, h=h, stride=w, flags=OPEN3, regions=p(regs), max_regions=M, offsets=p(offs), xy=p(pts),
               max_vertices=V)

    def hst(**kw):
        a = dict(okh, **kw)
        return L.mdx_mask_region_hulls(ctx._h, a["mask"], a["w"], a["h"], a["stride"], a["flags"], 1, a["regions"],
                                       a["max_regions"], C.byref(cnt[0]), C.byref(cnt[1]), a["offsets"], a["xy"],
                                       a["max_vertices"], C.byref(cnt[2]))
    wide = np.zeros((1, 8193), np.uint8)
    for kw in [dict(mask=None), dict(w=0), dict(h=-1), dict(stride=w - 1), dict(w=1 << 13, h=(1 << 17) + 1, stride=1 << 13),
               dict(max_regions=-1), dict(regions=None), dict(flags=8), dict(mask=p(wide), w=8193, h=1, stride=8193),
               dict(max_vertices=-1), dict(offsets=None), dict(xy=None)]:
        assert hst(**kw) == -1, kw
        assert b"mdx_mask_region_hulls" in L.mdx_last_error(ctx._h)
    assert (regs == AA).all() and (offs == AA).all() and (pts == AA).all() and [v.value for v in cnt] == [-5] * 3
    assert hst() == 0 and hst(xy=None, max_vertices=0) == 0 and hst(regions=None, max_regions=0) == 0
    assert offs[0] == 0 and cnt[2].value == 0                         # max_regions 0: no record takes part


# ---------------------------------------------------------------- end to end: chained behind the pair entry

def _chain(mdx, seeds, pipelining):
    """test_regions._chain's inputs: mdx_flow_warp_diff_batch_dev, mdx_mask_regions_dev and
    mdx_region_hulls_dev on one stream with no sync in between; one sync, then one copy each of the
    records, the offsets and xy; the checker runs on the device mask."""
    w, h, B = 160, 120, len(seeds)
    pairs = [mdx.synth_pair(s, w, h, 1) for s in seeds]
    g1 = np.stack([p[0] for p in pairs])
    g2 = np.stack([p[1] for p in pairs])
    Hs = np.stack([p[2] for p in pairs]).astype(np.float64)
    cap, maxv = 64, 2048
    with mdx.Context(0, w, h, B, fit_mode=mdx.FIT_EXTERNAL, thresh=30, call_pipelining=pipelining) as c:
        n = mdx.grid_count(w, h, c.params.pixel_step)
        host = dict(regs=np.full((B, cap, 8), AA, np.int32), nall=np.full(B, AA, np.int32),
                    nkept=np.full(B, AA, np.int32), mask=np.full((B, h, w), 0xAA, np.uint8),
                    labels=np.full((B, h, w), AA, np.int32), offsets=np.full((B, cap + 1), AA, np.int32),
                    xy=np.full((B, maxv, 2), AA, np.int32), nv=np.full(B, AA, np.int32))
        d = {k: c.dev_alloc(v.nbytes) for k, v in host.items()}
        d.update(i1=c.dev_alloc(g1.nbytes), i2=c.dev_alloc(g2.nbytes), H=c.dev_alloc(Hs.nbytes), np=c.dev_alloc(B * n * 8),
                 st=c.dev_alloc(B * n))
        try:
            for k, v in host.items():
                c.h2d(d[k], v)
            c.h2d(d["i1"], g1), c.h2d(d["i2"], g2), c.h2d(d["H"], Hs)
            c.flow_warp_diff_batch_dev(B, d["i1"], d["i2"], w, h, w, w * h, mdx.FMT_GRAY8, d["np"], d["st"], 0,
                                       d["mask"], 0, d["H"], 0)
            c.mask_regions_dev(B, d["mask"], w, h, w, w * h, True, 50, d["regs"], cap, d["nall"], d["nkept"], d["labels"])
            c.region_hulls_dev(B, d["labels"], w, h, d["regs"], cap, d["nkept"], d["offsets"], d["xy"], maxv, d["nv"])
            c.sync()
            for k, v in host.items():
                c.d2h(v, d[k])
        finally:
            for p in d.values():
                c.dev_free(p)
    host.update(cap=cap, maxv=maxv)
    for i in range(B):
        ref = regions_reference(host["mask"][i], open3=True, min_area=50)
        assert host["nall"][i] == ref["num_all"] and host["nkept"][i] >= 1   # else the comparison is vacuous
        hulls = same(host, i, ref)
        assert all(len(v) >= 3 for v in hulls)


@pytest.mark.gpu
@pytest.mark.parametrize("pipelining", [0, 1])
def test_chained_behind_the_pair_entry(mdx, pipelining):
    _chain(mdx, [20141105, 20141106, 20141107], pipelining)
