"""Convex hulls of the kept clusters on the device (mdx_cluster_hulls).

Reference: showClusterContours (common/src/optical_flow_visualizer.cpp:204-221): cv::convexHull of each
cluster after cv::Mat(cluster).copyTo(vector<cv::Point>).  The vertex set is determined mathematically;
the start and the orientation (cv::convexHull(.., clockwise=false)) are restated from OpenCV 2.4's
documentation and unpinned against a real build.

The oracle is Andrew's monotone chain on Python ints over sorted(set(points)).  It shares nothing with
the kernel (no column bins, no rounds); a brute-force vertex definition checks it in turn.  Everything
is integer and exact: every device word must equal the oracle's, the unwritten tail included.
"""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

SENT = -77777777          # prefill of xy and offsets


def cv_round(points):
    """copyTo(vector<cv::Point>): cvRound, half to even, of float32 members; Python-int tuples."""
    p = np.rint(np.asarray(points, np.float32).reshape(-1, 2).astype(np.float64)).astype(np.int64)
    return [(int(x), int(y)) for x, y in p]


def cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull_oracle(int_points):
    """The hull of integer points in cv::convexHull(.., clockwise=false)'s order: from the greatest
    vertex along the max-y side to the smallest, then along the min-y side back; not closed."""
    pts = sorted(set((int(x), int(y)) for x, y in int_points))
    if len(pts) == 1:
        return pts

    def chain(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and cross(h[-2], h[-1], p) <= 0:
                h.pop()
            h.append(p)
        return h
    return chain(reversed(pts))[:-1] + chain(pts)[:-1]


def brute_vertices(int_points):
    """A point is a vertex iff it lies on no segment between two others and in no non-degenerate
    triangle of three others."""
    pts = sorted(set(int_points))
    out = set()
    for p in pts:
        others = [q for q in pts if q != p]
        hit = False
        for a, b in itertools.combinations(others, 2):
            if cross(a, b, p) == 0 and min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1]):
                hit = True
                break
        if not hit:
            for a, b, c in itertools.combinations(others, 3):
                d = cross(a, b, c)
                if d == 0:
                    continue
                s = 1 if d > 0 else -1
                if s * cross(a, b, p) >= 0 and s * cross(b, c, p) >= 0 and s * cross(c, a, p) >= 0:
                    hit = True
                    break
        if not hit:
            out.add(p)
    return out


# ---------------------------------------------------------------- CPU: the oracle itself

@pytest.mark.parametrize("rng_range", [2, 3, 5, 40])
def test_oracle_against_brute_force(rng_range):
    rng = np.random.default_rng(100 + rng_range)
    for _ in range(600):
        n = int(rng.integers(1, 10))
        pts = [tuple(int(v) for v in p) for p in rng.integers(-rng_range, rng_range + 1, (n, 2))]
        h = hull_oracle(pts)
        assert len(set(h)) == len(h)
        assert set(h) == brute_vertices(pts), pts
        assert h[0] == max(set(pts))                                   # greatest x, then greatest y
        if len(h) >= 3:                                                # counter-clockwise with y up, strictly convex
            assert all(cross(h[i - 2], h[i - 1], h[i]) > 0 for i in range(len(h))), (pts, h)
            i0 = h.index(min(set(pts)))
            assert all(h[i][0] >= h[i + 1][0] for i in range(i0))      # the max-y side runs towards smaller x
        elif len(h) == 2:
            assert h[1] == min(set(pts))


def test_oracle_known_answers():
    # the unit square with its centre: (0.5, 0.5) converts to (0, 0), half to even
    unit = cv_round([(0, 0), (1, 0), (1, 1), (0, 1), (0.5, 0.5)])
    assert hull_oracle(unit) == [(1, 1), (0, 1), (0, 0), (1, 0)]
    assert hull_oracle([(0, 0), (2, 0), (2, 2), (0, 2), (1, 1)]) == [(2, 2), (0, 2), (0, 0), (2, 0)]
    assert hull_oracle([(0, 0), (1, 0), (2, 0)]) == [(2, 0), (0, 0)]           # horizontal
    assert hull_oracle([(0, 0), (0, 1), (0, 2)]) == [(0, 2), (0, 0)]           # vertical
    assert hull_oracle([(0, 0), (1, 1), (2, 2)]) == [(2, 2), (0, 0)]           # rising diagonal
    assert hull_oracle([(0, 2), (1, 1), (2, 0)]) == [(2, 0), (0, 2)]           # falling diagonal
    assert hull_oracle([(3, -4)]) == [(3, -4)]
    assert hull_oracle([(3, -4), (3, -4)]) == [(3, -4)]


def test_cv_round_is_half_to_even():
    assert cv_round([(0.5, 1.5), (2.5, -0.5), (-1.5, 3.5)]) == [(0, 2), (2, 0), (-2, 4)]


def test_write_contour_lines_from_a_hull(tmp_path, mdx):
    """frame, id, x, y, x, y, ... in the Python logger and in host/'s MotionLogger."""
    import os
    import shutil
    import subprocess
    from motion_detection_amd.formats import MotionLogger
    from node_io import HOST, ROOT
    hull = np.array(hull_oracle([(0, 0), (4, 0), (4, 3), (0, 3), (2, 1), (-2, 1)]), np.int32)
    assert hull.tolist() == [[4, 3], [0, 3], [-2, 1], [0, 0], [4, 0]]
    lg = MotionLogger(str(tmp_path / "py_log"))
    lg.writeContour(hull, 41, 2)
    lg.close()
    assert (tmp_path / "py_log").read_text() == "41, 2, 4, 3, 0, 3, -2, 1, 0, 0, 4, 0\n"
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    src = tmp_path / "c.cpp"
    src.write_text('#include "mdx_host.h"\nint main(int, char** argv) { mdx_host::MotionLogger lg(argv[1]); '
                   "lg.write_contour({4, 3, 0, 3, -2, 1, 0, 0, 4, 0}, 41, 2); return 0; }\n")
    libdir = os.path.join(ROOT, "motion_detection_amd", "lib")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", HOST, "-I", os.path.join(ROOT, "include"), str(src),
                    os.path.join(HOST, "mdx_host.cpp"), "-L", libdir, "-lmdx", f"-Wl,-rpath,{libdir}", "-o",
                    str(tmp_path / "c")], check=True)
    subprocess.run([str(tmp_path / "c"), str(tmp_path / "cpp_log")], check=True)
    assert (tmp_path / "cpp_log").read_bytes() == (tmp_path / "py_log").read_bytes()


def test_null_context_is_einval(mdx):
    pts = np.zeros((4, 2), np.float32)
    lab = np.zeros(4, np.int32)
    ids = np.zeros(1, np.int32)
    off = np.zeros(2, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert mdx.lib().mdx_cluster_hulls(None, p(pts), p(lab), 4, p(ids), 1, p(off), None, 0, None) == mdx._lib.MDX_EINVAL


def test_binding_lists_the_entry(mdx):
    import re
    from test_abi import HEADER, header_functions
    assert "mdx_cluster_hulls" in header_functions() and "mdx_cluster_hulls" in mdx._lib.EXPORTED
    assert sorted(mdx._lib.EXPORTED) == header_functions()
    hdr = open(HEADER).read()
    assert int(re.search(r"#define MDX_ABI_VERSION (\d+)", hdr).group(1)) == mdx._lib.ABI_VERSION == 11
    assert int(re.search(r"#define MDX_HULL_MAX_SPAN (\d+)", hdr).group(1)) == mdx._lib.HULL_MAX_SPAN == 8192


def test_contours_field_is_last_and_defaults(mdx):
    from motion_detection_amd.node import LiveResult, MotionDetectionNode
    import dataclasses
    assert dataclasses.fields(LiveResult)[-1].name == "contours"
    assert LiveResult(3, None, [], [], []).contours == []
    assert mdx.FlowResult.__dataclass_fields__["contours"].default_factory is list
    assert list(mdx.FlowResult.__dataclass_fields__)[-1] == "contours"
    # off by default (the reference's writeContour loop is commented out)
    import inspect
    assert '"cluster_contours": False' in inspect.getsource(MotionDetectionNode.__init__)


# ---------------------------------------------------------------- GPU: the device against the oracle

def call(ctx, pts, labels, ids, max_vertices=None, cap=None):
    """The raw entry on sentinel-filled outputs: (rc, offsets [k+1], xy [cap][2], num_vertices)."""
    from motion_detection_amd._lib import lib
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    labels = np.ascontiguousarray(labels, np.int32)
    ids = np.ascontiguousarray(ids, np.int32)
    n, k = len(pts), len(ids)
    cap = n + 8 if cap is None else cap
    maxv = cap if max_vertices is None else max_vertices
    offsets = np.full(k + 1, SENT, np.int32)
    xy = np.full((cap, 2), SENT, np.int32)
    total = C.c_int(SENT)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = lib().mdx_cluster_hulls(ctx._h, p(pts), p(labels), n, p(ids), k, p(offsets), p(xy), maxv, C.byref(total))
    return rc, offsets, xy, total.value


def expected(pts, labels, ids):
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    labels = np.asarray(labels)
    return [hull_oracle(cv_round(pts[labels == int(i)])) for i in ids]


def check(ctx, pts, labels, ids, hulls=None, max_vertices=None):
    """Every word of offsets and xy against the oracle, the unwritten tail included."""
    hulls = expected(pts, labels, ids) if hulls is None else hulls
    rc, offsets, xy, total = call(ctx, pts, labels, ids, max_vertices)
    assert rc == 0
    want_off = np.concatenate([[0], np.cumsum([len(h) for h in hulls])]).astype(np.int32)
    assert np.array_equal(offsets, want_off)
    assert total == want_off[-1]
    flat = np.array([v for h in hulls for v in h], np.int32).reshape(-1, 2)
    m = len(flat) if max_vertices is None else min(len(flat), max_vertices)
    assert np.array_equal(xy[:m], flat[:m])
    assert np.all(xy[m:] == SENT)
    return hulls


def one(ctx, pts, hull=None):
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    return check(ctx, pts, np.zeros(len(pts), np.int32), [0], None if hull is None else [hull])[0]


@pytest.mark.gpu
def test_degenerate_and_ties(ctx):
    assert one(ctx, [(3, -4)]) == [(3, -4)]
    assert one(ctx, [(3, -4), (3, -4)]) == [(3, -4)]
    assert one(ctx, [(3, -4), (5, -4)]) == [(5, -4), (3, -4)]
    assert one(ctx, [(3, -4), (3, 9)]) == [(3, 9), (3, -4)]
    assert one(ctx, [(0, 0), (1, 0), (2, 0), (1, 0), (2, 0), (0, 0)]) == [(2, 0), (0, 0)]
    assert one(ctx, [(0, 0), (0, 1), (0, 2), (0, 1), (0, 2)]) == [(0, 2), (0, 0)]
    assert one(ctx, [(1, 1), (0, 0), (2, 2), (3, 3), (1, 1), (3, 3)]) == [(3, 3), (0, 0)]
    assert one(ctx, [(1, 2), (0, 3), (3, 0), (2, 1), (2, 1), (0, 3)]) == [(3, 0), (0, 3)]
    # cvRound ties: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> 0, -1.5 -> -2
    assert one(ctx, [(0.5, 0.5)]) == [(0, 0)]
    assert one(ctx, [(1.5, -0.5)]) == [(2, 0)]
    assert one(ctx, [(2.5, -1.5)]) == [(2, -2)]
    assert one(ctx, [(0.5, 1.5), (2.5, -0.5), (-1.5, 2.5), (-0.5, -1.5)]) == hull_oracle([(0, 2), (2, 0), (-2, 2), (0, -2)])
    assert one(ctx, [(0.5, 0), (-0.5, 0), (0.49, 0)]) == [(0, 0)]
    assert one(ctx, [(0, 0), (2, 0), (2, 2), (0, 2), (1, 1)]) == [(2, 2), (0, 2), (0, 0), (2, 0)]
    neg = [(-7, -3), (-2, -9), (-5.5, -4.5), (-1, -1), (-9, -8), (-4, -4)]
    assert one(ctx, neg) == hull_oracle(cv_round(neg))


@pytest.mark.gpu
def test_coordinate_limit(ctx, mdx):
    L = float(2 ** 29)
    # float32 steps by 32 below 2^29: every coordinate here is exact
    I = 2 ** 29
    assert one(ctx, [(L, L), (L - 64, -L), (L - 8160, 0)]) == [(I, I), (I - 8160, 0), (I - 64, -I)]
    assert one(ctx, [(-L, -L), (-L + 8128, L), (-L + 4064, 0)]) == [(-I + 8128, I), (-I, -I)]      # collinear
    assert one(ctx, [(-L, L), (-L + 8160, -L), (-L + 4096, 32)]) == [(-I + 8160, -I), (-I + 4096, 32), (-I, I)]
    beyond = float(np.nextafter(np.float32(L), np.float32(np.inf)))
    for bad in [(beyond, 0), (0, beyond), (-beyond, 0), (0, -beyond)]:
        rc, *_ = call(ctx, [(0, 0), bad], [0, 0], [0])
        assert rc == mdx._lib.MDX_EINVAL
    # a member beyond the limit that takes no part does not matter
    check(ctx, [(0, 0), (beyond, 0), (1, 5)], [0, 1, 0], [0])


SPANS = [1, 2, 63, 64, 65, 255, 256, 257, 8191, 8192]


def span_points(span, sparse, seed):
    """Members in exactly `span` columns (every other one empty when sparse), two or three per column."""
    rng = np.random.default_rng(seed)
    cols = np.arange(0, span, 2 if sparse else 1)
    if cols[-1] != span - 1:
        cols = np.append(cols, span - 1)
    x = np.repeat(cols, 3)[: len(cols) * 3 - int(rng.integers(0, 2))]
    y = rng.integers(-500, 500, len(x))
    p = np.stack([x + 100, y], 1).astype(np.float32)
    return p[rng.permutation(len(p))]


@pytest.mark.gpu
@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("span", SPANS)
def test_column_counts(ctx, span, sparse):
    pts = span_points(span, sparse, span)
    c = cv_round(pts)
    assert max(x for x, _ in c) - min(x for x, _ in c) + 1 == span
    one(ctx, pts)


@pytest.mark.gpu
@pytest.mark.parametrize("sparse", [False, True])
def test_span_beyond_the_limit_is_einval(ctx, mdx, sparse):
    pts = span_points(8193, sparse, 5)
    rc, *_ = call(ctx, pts, np.zeros(len(pts), np.int32), [0])
    assert rc == mdx._lib.MDX_EINVAL
    # the same members as two clusters of legal span
    lab = (pts[:, 0] >= 100 + 4096).astype(np.int32)
    check(ctx, pts, lab, [0, 1])


def parabola(sign):
    """(x, +-(x - 4096)^2) over 8192 columns.  Centred, so that every y is at most 2^24 and exact in
    float32: (x, x^2) itself is not beyond x = 4096, and its rounded members are not all vertices."""
    x = np.arange(8192, dtype=np.int64)
    return np.stack([x, sign * (x - 4096) ** 2], 1)


def tail_input(exact=False):
    """(x, -x^2), x = 0..8190, under (8191, 10^8): only the last interior candidate of the max-y chain is
    removable in each simultaneous round.  exact: the centred parabola, whose float32 members keep that
    property to the last column (the members of -x^2 are rounded to multiples of 4 beyond x = 4096)."""
    x = np.arange(8191, dtype=np.int64)
    y = -(x - 4096) ** 2 if exact else -x * x
    return np.concatenate([np.stack([x, y], 1), [(8191, 10 ** 8)]]).astype(np.float64)


def tail_stairs():
    """Four concave arcs of 2047 columns, each under a far point four times as high as the one before: the
    sequential chain behind the rounds pushes an arc, pops it at its far point, and pops the earlier far
    points too."""
    out = []
    for a in range(4):
        x = np.arange(2047, dtype=np.int64)
        out += [np.stack([x + 2048 * a, -(x - 1024) ** 2], 1), [(2048 * a + 2047, 10 ** 6 * 4 ** a)]]
    return np.concatenate(out).astype(np.float64)


def upper_rounds(points, limit):
    """Simultaneous rounds on the max-y chain of points in distinct columns (a model, not the kernel's
    code): how many remove something, counted up to `limit`, and the candidates each removed."""
    up, removed = sorted(points), []
    while len(removed) < limit:
        keep = [True] + [cross(up[i - 1], up[i], up[i + 1]) < 0 for i in range(1, len(up) - 1)] + [True]
        if all(keep):
            break
        removed.append(keep.count(False))
        up = [p for p, k in zip(up, keep) if k]
    return removed


def circle(r=4000):
    x = np.arange(-r, r + 1, dtype=np.int64)
    y = np.rint(np.sqrt(r * r - x * x)).astype(np.int64)
    return np.concatenate([np.stack([x, y], 1), np.stack([x, -y], 1)])


def sawtooth():
    x = np.arange(4096, dtype=np.int64)
    amp = 1 << (x // 256)                       # the amplitude doubles every 256 columns
    return np.stack([x, np.where(x % 2 == 0, amp, -amp)], 1)


STRESS = {
    "parabola_up": lambda: parabola(1),
    "parabola_down": lambda: parabola(-1),
    "parabola_up_x2": lambda: np.stack([np.arange(8192), np.arange(8192, dtype=np.int64) ** 2], 1),
    "parabola_down_x2": lambda: np.stack([np.arange(8192), -np.arange(8192, dtype=np.int64) ** 2], 1),
    "sawtooth": sawtooth,
    "circle": circle,
    "tail": tail_input,
    "tail_mirror_x": lambda: tail_input() * [-1, 1],
    "tail_mirror_y": lambda: tail_input() * [1, -1],
    "tail_mirror_xy": lambda: tail_input() * [-1, -1],
    "tail_exact": lambda: tail_input(True),
    "tail_exact_mirror_xy": lambda: tail_input(True) * [-1, -1],
    "tail_stairs": tail_stairs,
    "tail_stairs_mirror_xy": lambda: tail_stairs() * [-1, -1],
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STRESS))
def test_chain_stress(ctx, name):
    pts = np.asarray(STRESS[name](), np.float64).astype(np.float32)
    h = one(ctx, pts)
    if name in ("parabola_up", "parabola_down"):
        assert len(h) == 8192
    if name.startswith("tail_exact"):
        assert len(h) == 3


def test_stress_inputs_are_what_they_claim():
    """CPU: the float32 members of the centred parabolas are all vertices (8192), and the exact tail
    input takes one simultaneous round per column (a model of the rounds, not the kernel's code)."""
    for sign in (1, -1):
        assert len(hull_oracle(cv_round(parabola(sign).astype(np.float32)))) == 8192
    pts = cv_round(tail_input(True).astype(np.float32))
    assert pts == [(int(x), int(y)) for x, y in tail_input(True)]
    assert upper_rounds(pts, 40) == [1] * 40                  # only the last interior candidate goes: 8,190 rounds in all
    stairs = cv_round(tail_stairs().astype(np.float32))
    assert stairs == [(int(x), int(y)) for x, y in tail_stairs()]
    assert len(upper_rounds(stairs, 40)) == 40                # far beyond any bound on the rounds here too


@functools.lru_cache(maxsize=None)
def many(k, per=64, seed=3):
    """k requested clusters of `per` members among k + 7 labels, interleaved; some members labelled -1."""
    rng = np.random.default_rng(seed + k)
    n = (k + 7) * per
    labels = (np.arange(n) % (k + 7)).astype(np.int32)
    centre = rng.uniform(100, 1800, (k + 7, 2))
    pts = (centre[labels] + rng.normal(0, 30, (n, 2))).astype(np.float32)
    labels[rng.random(n) < 0.05] = -1
    ids = np.sort(rng.choice(k + 7, k, replace=False)).astype(np.int32)
    return pts, labels, ids


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, 300])
def test_many_clusters(ctx, k):
    pts, labels, ids = many(k)
    assert len(set(labels.tolist()) - set(ids.tolist()) - {-1}) >= 1      # labels nobody asked for
    check(ctx, pts, labels, ids)
    check(ctx, pts, labels, ids[::2])                                     # a strict subset


@pytest.mark.gpu
def test_max_vertices_cuts_the_output_short(ctx):
    pts, labels, ids = many(3)
    hulls = expected(pts, labels, ids)
    total = sum(len(h) for h in hulls)
    assert total > len(hulls[0]) + 1
    check(ctx, pts, labels, ids, hulls, max_vertices=len(hulls[0]) + 1)   # ends inside the second hull
    check(ctx, pts, labels, ids, hulls, max_vertices=0)
    from motion_detection_amd._lib import lib
    off = np.full(4, SENT, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = lib().mdx_cluster_hulls(ctx._h, p(pts), p(labels), len(pts), p(ids), 3, p(off), None, 0, None)
    assert rc == 0 and off[-1] == total


@pytest.mark.gpu
def test_largest_cluster(ctx, mdx):
    n = mdx._lib.CLUSTER_MAX_POINTS
    pts = np.random.default_rng(8).uniform(0, [1919, 1079], (n, 2)).astype(np.float32)
    one(ctx, pts)


@pytest.mark.gpu
def test_no_stale_scratch(ctx):
    big, small = span_points(8192, False, 1), span_points(65, True, 2)
    a = one(ctx, big)
    b = one(ctx, small)
    assert one(ctx, big) == a and one(ctx, small) == b
    pts, labels, ids = many(300)
    check(ctx, pts, labels, ids)
    assert one(ctx, small) == b


@pytest.mark.gpu
def test_empty_calls(ctx):
    rc, off, xy, total = call(ctx, np.zeros((0, 2)), np.zeros(0), [0, 4])
    assert rc == 0 and off.tolist() == [0, 0, 0] and total == 0 and np.all(xy == SENT)
    rc, off, xy, total = call(ctx, [(1, 2)], [0], [])
    assert rc == 0 and off.tolist() == [0] and total == 0 and np.all(xy == SENT)
    assert ctx.cluster_hulls(np.zeros((0, 2)), np.zeros(0), []) == []


@pytest.mark.gpu
def test_bad_arguments(ctx, mdx):
    from motion_detection_amd._lib import lib
    E = mdx._lib.MDX_EINVAL
    pts, labels, ids = many(3)
    n = len(pts)
    off, xy = np.zeros(4, np.int32), np.zeros((n, 2), np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731

    def raw(pts=pts, labels=labels, n=n, ids=ids, k=3, off=off, xy=xy, maxv=n):
        return lib().mdx_cluster_hulls(ctx._h, p(pts), p(labels), n, p(ids), k, p(off), p(xy), maxv, None)
    assert raw() == 0
    assert raw(n=-1) == E and raw(k=-1) == E and raw(maxv=-1) == E
    assert raw(n=mdx._lib.CLUSTER_MAX_POINTS + 1) == E
    assert raw(pts=None) == E and raw(labels=None) == E and raw(ids=None) == E and raw(off=None) == E and raw(xy=None) == E
    assert raw(xy=None, maxv=0) == 0
    assert raw(ids=ids[::-1].copy()) == E                                  # descending
    assert raw(ids=np.array([ids[0], ids[0], ids[2]], np.int32)) == E      # not strictly ascending
    assert raw(ids=np.array([-1, ids[1], ids[2]], np.int32)) == E          # negative
    assert raw(ids=np.array([ids[0], ids[1], 100000], np.int32)) == E      # an id with no member
    assert raw(n=2, ids=np.arange(3, dtype=np.int32)) == E                 # more ids than members: one has none
    for bad in (np.nan, np.inf, -np.inf):
        q = pts.copy()
        q[int(np.flatnonzero(labels == -1)[0]), 1] = bad                   # non-finite, even in a member that takes no part
        assert raw(pts=q) == E
    q = pts.copy()
    q[int(np.flatnonzero(labels == ids[1])[0]), 0] = 2.0 ** 29 + 64
    assert raw(pts=q) == E                                                 # beyond 2^29
    q = pts.copy()
    q[int(np.flatnonzero(labels == ids[1])[0]), 0] += 8192
    assert raw(pts=q) == E                                                 # more than 8192 columns
    assert raw() == 0
    with pytest.raises(mdx.MdxError):
        ctx.cluster_hulls(pts, labels, ids[::-1].copy())


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(3))
def test_through_cluster_euclidean(ctx, mdx, seed):
    from motion_detection_amd.flow_clusterer import clusters_from_labels
    from test_cluster import tie_grid
    pts = tie_grid(160, 120, seed)
    res = ctx.cluster_euclidean(pts, 10.5)
    assert len(res.kept) >= 1
    want = [hull_oracle(cv_round(m)) for m in clusters_from_labels(pts, res.labels, res.kept)]
    check(ctx, pts, res.labels, res.kept, want)
    got = ctx.cluster_hulls(pts, res.labels, res.kept)
    assert [g.dtype for g in got] == [np.int32] * len(want)
    assert [list(map(tuple, g.tolist())) for g in got] == want
    fc = mdx.FlowClusterer(context=ctx)
    members = fc.clusterEuclidean(pts, 10.5)
    assert [list(map(tuple, g.tolist())) for g in fc.hulls()] == want
    assert [list(map(tuple, g.tolist())) for g in mdx.hulls_of(members, ctx)] == want
    fc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["grid", "holes"])
def test_through_cluster_vectors(ctx, mdx, kind):
    import test_vcluster as tv
    if kind == "grid":
        vec, thr, athr = tv.grid_input(1025), tv.GRID_THR, tv.GRID_ATHR
    else:                                       # inactive vectors in between: label -1
        vec, thr, athr = tv.holes_input(513)[0], tv.UNI_THR, tv.UNI_ATHR
    res = ctx.cluster_vectors(vec, thr, athr)
    assert len(res.kept) >= 1 and (kind == "grid" or (res.labels == -1).any())
    xy = vec[:, :2].astype(np.float32)          # cv::Point2f(vec[0], vec[1]) (node.cpp:382)
    want = [hull_oracle(cv_round(xy[res.labels == int(k)])) for k in res.kept]
    check(ctx, xy, res.labels, res.kept, want)
    assert mdx.hulls_of([], ctx) == []
    # FlowClusterer.hulls() after getClusters: the Vec4d image's grid, rows outer
    img = np.zeros((480, 640, 4))
    g = tv.grid_input(1025)
    img[g[:, 1].astype(int), g[:, 0].astype(int)] = g
    fc = mdx.FlowClusterer(context=ctx)
    members = fc.getClusters(img, 10, tv.GRID_THR, tv.GRID_ATHR)
    assert len(members) >= 1
    got = [list(map(tuple, h.tolist())) for h in fc.hulls()]
    assert got == [hull_oracle(cv_round(m[:, :2].astype(np.float32))) for m in members]
    fc.close()
