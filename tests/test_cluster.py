"""FlowClusterer::clusterEuclidean + boundingRect on the device (mdx_cluster_euclidean).

Reference: clusterEuclidean (common/src/flow_clusterer.cpp:231-269), the distance
(common/src/point_cluster.cpp:63-66), the rectangles (common/src/optical_flow_visualizer.cpp:230-236).
Restated from the source; unpinned against a real build (no OpenCV 2.4 to run).

The checker below is the reference's literal loop: clusters are lists in creation order, each
cluster's distance is the minimum over its members, a strict < scan over the clusters picks one, a
double compare against the threshold decides.  It does not use the device code's (s, root) key
form, so the two check each other; every device result must equal it exactly.
"""
import ctypes as C
import functools
import sys

import numpy as np
import pytest


def _dist_row(pts, i):
    """d(i, j) for j < i: s in float32, every operation rounded (numpy does not fuse), sqrt in double."""
    dx = pts[i, 0] - pts[:i, 0]
    dy = pts[i, 1] - pts[:i, 1]
    s = dx * dx + dy * dy
    assert s.dtype == np.float32
    return np.sqrt(s.astype(np.float64))


def cluster_reference(points, thr, min_size=5, first_nearest=False):
    """The literal greedy loop.  first_nearest=True is the wrong variant the tie inputs must tell
    apart: it joins the cluster of the first nearest earlier point, not the earliest-created cluster
    among the tied ones."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
    n = len(pts)
    thr = float(thr)
    clusters = []                       # member index lists, creation order
    labels = np.zeros(n, np.int32)
    with np.errstate(over="ignore"):
        for i in range(n):
            index = -1
            closest = sys.float_info.max
            if i:
                d = _dist_row(pts, i)
                if first_nearest:
                    j = int(np.argmin(d))
                    if d[j] < closest:
                        closest, index = float(d[j]), int(labels[j])
                else:
                    dk = np.full(len(clusters), np.inf)
                    np.minimum.at(dk, labels[:i], d)        # getClosestDistance of every cluster
                    for k, v in enumerate(dk.tolist()):
                        if v < closest:
                            closest, index = v, k
            if index != -1 and closest < thr:
                clusters[index].append(i)
            else:
                index = len(clusters)
                clusters.append([i])
            labels[i] = index
    kept = [k for k, m in enumerate(clusters) if len(m) > min_size]
    members = [pts[clusters[k]] for k in kept]
    return dict(labels=labels, num_all=len(clusters), kept=np.array(kept, np.int32).reshape(-1),
                rects=reference_rects(members), members=members)


def reference_rects(members):
    """copyTo(vector<cv::Point>) = cvRound (half to even), then boundingRect of integer points."""
    out = np.zeros((len(members), 4), np.int32)
    for k, m in enumerate(members):
        p = np.rint(np.asarray(m, np.float32).astype(np.float64)).astype(np.int64)
        x0, y0 = p.min(axis=0)
        x1, y1 = p.max(axis=0)
        out[k] = (x0, y0, x1 - x0 + 1, y1 - y0 + 1)
    return out


def grid(w, h, step):
    """(x, y) of a w x h grid at `step`, x-major."""
    xs, ys = np.arange(0, w, step, dtype=np.float32), np.arange(0, h, step, dtype=np.float32)
    gx, gy = np.meshgrid(xs, ys, indexing="ij")
    return np.stack([gx.ravel(), gy.ravel()], 1)


def tie_grid(w, h, seed, keep=0.5):
    g = grid(w, h, 10)
    return g[np.random.default_rng(seed).random(len(g)) < keep]


@functools.lru_cache(maxsize=None)
def uniform_points(n):
    return np.random.default_rng(1000 + n).uniform(0, [640, 480], (n, 2)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def uniform_reference(n):
    return cluster_reference(uniform_points(n), 20.0)


def same(res, ref):
    assert np.array_equal(res.labels, ref["labels"])
    assert res.num_all == ref["num_all"]
    assert np.array_equal(res.kept, ref["kept"])
    assert np.array_equal(res.rects, ref["rects"])
    assert res.num_kept == len(ref["kept"])


# ---------------------------------------------------------------- CPU: the checker itself

def row(n, x0=0.0):
    return np.array([(x0 + i, 0.0) for i in range(n)], np.float32)


def test_checker_six_in_a_row_is_one_kept_cluster():
    r = cluster_reference(row(6), 1.5)
    assert r["num_all"] == 1 and list(r["kept"]) == [0] and list(r["labels"]) == [0] * 6
    assert np.array_equal(r["members"][0], row(6))
    assert r["rects"].tolist() == [[0, 0, 6, 1]]


def test_checker_five_in_a_row_is_not_kept():
    r = cluster_reference(row(5), 1.5)
    assert r["num_all"] == 1 and len(r["kept"]) == 0 and r["rects"].shape == (0, 4)


def test_checker_two_groups_in_creation_order():
    a, b = row(6, 100.0), row(7, 0.0)
    pts = np.empty((13, 2), np.float32)
    pts[0::2] = b                       # interleaved: b's first point comes first
    pts[1::2] = a
    r = cluster_reference(pts, 1.5)
    assert r["num_all"] == 2 and list(r["kept"]) == [0, 1]
    assert np.array_equal(r["members"][0], b) and np.array_equal(r["members"][1], a)
    assert r["rects"].tolist() == [[0, 0, 7, 1], [100, 0, 6, 1]]


def test_checker_tie_joins_the_earlier_cluster():
    # clusters {(0,0)} and {(4,0)}; (2,0) is 2 from both: strict < keeps the first
    r = cluster_reference(np.array([(0, 0), (4, 0), (2, 0)], np.float32), 2.5)
    assert list(r["labels"]) == [0, 1, 0]
    # (5.5, 0) is 4.5 from (10, 0) of cluster 1 and from (1, 0) of cluster 0: cluster 0, although the
    # first nearest earlier point in input order is cluster 1's
    pts = np.array([(0, 0), (10, 0), (1, 0), (5.5, 0)], np.float32)
    assert list(cluster_reference(pts, 5.0)["labels"]) == [0, 1, 0, 0]
    assert list(cluster_reference(pts, 5.0, first_nearest=True)["labels"]) == [0, 1, 0, 1]


def test_checker_rectangles_round_half_to_even():
    m = np.array([(2.5, -0.5), (3.5, -1.5)], np.float32)
    assert reference_rects([m]).tolist() == [[2, -2, 4 - 2 + 1, 0 - (-2) + 1]]
    assert reference_rects([np.array([(2.5, 0)], np.float32)]).tolist() == [[2, 0, 1, 1]]
    assert reference_rects([np.array([(3.5, 0)], np.float32)]).tolist() == [[4, 0, 1, 1]]
    assert reference_rects([np.array([(-0.5, 0)], np.float32)]).tolist() == [[0, 0, 1, 1]]
    assert reference_rects([np.array([(-1.5, 0)], np.float32)]).tolist() == [[-2, 0, 1, 1]]
    assert reference_rects([np.array([(1, 7), (9, 7)], np.float32)])[0, 2] == 9 - 1 + 1


def test_tie_grids_have_teeth():
    """The GPU tie inputs must separate the reference's tie-break (earliest-created cluster) from
    'first nearest earlier point': the two labellings differ on at least one of the six grids."""
    differ = 0
    for seed in range(6):
        pts = tie_grid(160, 120, seed)
        a = cluster_reference(pts, 10.5)["labels"]
        b = cluster_reference(pts, 10.5, first_nearest=True)["labels"]
        differ += int(not np.array_equal(a, b))
    assert differ >= 1, differ


def test_null_context_is_einval(mdx):
    L = mdx.lib()
    pts = np.zeros((4, 2), np.float32)
    rc = L.mdx_cluster_euclidean(None, pts.ctypes.data_as(C.c_void_p), 4, 1.0, 5, None, None, None, None, 0, None)
    assert rc == mdx._lib.MDX_EINVAL


def test_clusters_from_labels():
    from motion_detection_amd.flow_clusterer import bounding_rects, clusters_from_labels
    pts = np.arange(16, dtype=np.float32).reshape(8, 2)
    labels = np.array([0, 1, 0, 2, 1, 0, 2, 0], np.int32)
    cl = clusters_from_labels(pts, labels, [0, 2])
    assert len(cl) == 2 and cl[0].dtype == np.float32
    assert np.array_equal(cl[0], pts[[0, 2, 5, 7]]) and np.array_equal(cl[1], pts[[3, 6]])
    assert clusters_from_labels(pts, labels, []) == []
    assert bounding_rects(cl) == [(0, 1, 15, 15), (6, 7, 7, 7)]
    half = [np.array([(2.5, -0.5), (3.5, -1.5)], np.float32)]
    assert bounding_rects(half) == [tuple(reference_rects(half)[0])]


def test_motion_log_lines_from_rects(tmp_path):
    """frame, id, tl.x, tl.y, br.x, br.y with br = tl + size, id = index among the kept clusters."""
    from motion_detection_amd.flow_clusterer import bounding_rects
    from motion_detection_amd.formats import MotionLogger
    members = [row(6, 3.0), np.array([(2.5, -0.5), (3.5, -1.5)], np.float32)]
    path = tmp_path / "motion.log"
    lg = MotionLogger(str(path))
    for k, rect in enumerate(bounding_rects(members)):
        lg.writeBoundingBox(rect, 41, k)
    lg.close()
    assert path.read_text() == "41, 0, 3, 0, 9, 1\n41, 1, 2, -2, 5, 1\n"


def test_live_result_keeps_positional_construction():
    from motion_detection_amd.node import LiveResult
    r = LiveResult(3, None, [], [], [])
    assert r.clusters == [] and r.rectangles == []


# ---------------------------------------------------------------- GPU: the device against the checker

@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 5, 6])
def test_tiny(ctx, n):
    pts = row(n)
    same(ctx.cluster_euclidean(pts, 1.5), cluster_reference(pts, 1.5))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(6))
def test_tie_grid(ctx, seed):
    pts = tie_grid(160, 120, seed)
    ref = cluster_reference(pts, 10.5)
    assert len(ref["kept"]) >= 1
    same(ctx.cluster_euclidean(pts, 10.5), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(6))
def test_threshold_equal_to_the_grid_step_joins_nothing(ctx, seed):
    pts = tie_grid(200, 100, seed)
    ref = cluster_reference(pts, 10.0)
    assert ref["num_all"] == len(pts)              # 10 < 10 is false
    same(ctx.cluster_euclidean(pts, 10.0), ref)


# 64 / 128 / 192: the four point slots of a lane in the in-block walk; 256: the block size and the
# single-launch cutoff; the larger ones are several blocks with a partial last one
BLOCK_EDGES = [63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2049, 4097]


@pytest.mark.gpu
@pytest.mark.parametrize("n", BLOCK_EDGES)
def test_block_edges_uniform(ctx, n):
    same(ctx.cluster_euclidean(uniform_points(n), 20.0), uniform_reference(n))


@functools.lru_cache(maxsize=None)
def big_grid():
    return tie_grid(640, 480, 7, keep=0.6)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [n for n in BLOCK_EDGES if n <= 1500])
def test_block_edges_grid(ctx, n):
    g = big_grid()
    assert n <= len(g)
    pts = g[:n]
    same(ctx.cluster_euclidean(pts, 14.2), cluster_reference(pts, 14.2))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["forward", "zigzag"])
def test_deep_chain(ctx, order):
    n = 2049
    idx = np.arange(n)
    if order == "zigzag":                           # 0, 2048, 1, 2047, ...
        z = np.empty(n, np.int64)
        z[0::2] = idx[: (n + 1) // 2]
        z[1::2] = idx[::-1][: n // 2]
        idx = z
        assert list(idx[:4]) == [0, 2048, 1, 2047]
    pts = np.stack([idx.astype(np.float32), np.zeros(n, np.float32)], 1)
    ref = cluster_reference(pts, 1.5)
    if order == "forward":
        assert ref["num_all"] == 1
    same(ctx.cluster_euclidean(pts, 1.5), ref)


@pytest.mark.gpu
def test_threshold_edge(ctx):
    p34 = np.array([(0, 0), (3, 4)], np.float32)
    for thr, joined in [(5.0, False), (float(np.nextafter(5.0, np.inf)), True)]:
        ref = cluster_reference(p34, thr)
        assert ref["num_all"] == (1 if joined else 2)
        same(ctx.cluster_euclidean(p34, thr), ref)
    p11 = np.array([(0, 0), (1, 1)], np.float32)
    thr = 1.41421355
    assert float(np.sqrt(np.float32(2))) < thr < float(np.sqrt(2.0))    # a float root would join
    ref = cluster_reference(p11, thr)
    assert ref["num_all"] == 2
    same(ctx.cluster_euclidean(p11, thr), ref)
    for thr in (0.0, -1.0, float("inf")):
        same(ctx.cluster_euclidean(uniform_points(65), thr), cluster_reference(uniform_points(65), thr))
    dup = np.zeros((7, 2), np.float32)                                   # d = 0 < a tiny threshold
    same(ctx.cluster_euclidean(dup, 1e-200), cluster_reference(dup, 1e-200))


@pytest.mark.gpu
def test_rounding_and_negatives(ctx):
    pts = np.array([(2.5, -0.5), (3.5, -1.5), (3.0, -1.0), (2.75, -0.75), (3.25, -1.25), (2.6, -0.6), (900, 900)],
                   np.float32)
    ref = cluster_reference(pts, 2.0)
    assert ref["rects"].tolist() == [[2, -2, 3, 3]]
    same(ctx.cluster_euclidean(pts, 2.0), ref)


@pytest.mark.gpu
def test_max_kept_smaller_than_num_kept(ctx):
    pts = tie_grid(160, 120, 0)
    ref = cluster_reference(pts, 10.5, min_size=1)
    assert len(ref["kept"]) >= 3
    r = ctx.cluster_euclidean(pts, 10.5, min_size=1, max_kept=2)
    assert r.num_kept == len(ref["kept"]) and len(r.kept) == 2 and r.rects.shape == (2, 4)
    assert np.array_equal(r.kept, ref["kept"][:2]) and np.array_equal(r.rects, ref["rects"][:2])
    assert np.array_equal(r.labels, ref["labels"])
    # the arrays past max_kept are not written
    L = ctx._h
    from motion_detection_amd._lib import lib
    kept = np.full(8, -7, np.int32)
    rects = np.full((8, 4), -7, np.int32)
    nk = C.c_int(0)
    p = np.ascontiguousarray(pts)
    rc = lib().mdx_cluster_euclidean(L, p.ctypes.data_as(C.c_void_p), len(p), 10.5, 1, None, None,
                                     kept.ctypes.data_as(C.c_void_p), rects.ctypes.data_as(C.c_void_p), 2, C.byref(nk))
    assert rc == 0 and nk.value == len(ref["kept"])
    assert np.all(kept[2:] == -7) and np.all(rects[2:] == -7) and np.array_equal(kept[:2], ref["kept"][:2])


@pytest.mark.gpu
def test_bad_arguments(ctx, mdx):
    from motion_detection_amd._lib import lib
    pts = uniform_points(65).copy()

    def call(p, n, thr, max_kept=0):
        return lib().mdx_cluster_euclidean(ctx._h, None if p is None else p.ctypes.data_as(C.c_void_p), n, thr, 5,
                                           None, None, None, None, max_kept, None)
    assert call(pts, -1, 1.0) == mdx._lib.MDX_EINVAL
    assert call(pts, 65, 1.0, -1) == mdx._lib.MDX_EINVAL
    assert call(None, 3, 1.0) == mdx._lib.MDX_EINVAL
    assert call(None, 0, 1.0) == 0
    assert call(pts, 65, float("nan")) == mdx._lib.MDX_EINVAL
    assert call(pts, mdx._lib.CLUSTER_MAX_POINTS + 1, 1.0) == mdx._lib.MDX_EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        q = pts.copy()
        q[40, 1] = bad
        assert call(q, 65, 1.0) == mdx._lib.MDX_EINVAL
    assert call(pts, 65, 1.0) == 0


@pytest.mark.gpu
def test_max_points_known_answer(ctx, mdx):
    """The largest call (1024 launches), too large for the O(N^2) checker: two rows 1000 apart, their
    points 1 apart and interleaved in input order, threshold 1.5 -- two clusters, labels alternating."""
    n = mdx._lib.CLUSTER_MAX_POINTS
    k = np.arange(n // 2, dtype=np.float32)
    pts = np.empty((n, 2), np.float32)
    pts[0::2] = np.stack([k, np.zeros_like(k)], 1)
    pts[1::2] = np.stack([k, np.full_like(k, 1000.0)], 1)
    r = ctx.cluster_euclidean(pts, 1.5)
    assert r.num_all == 2 and r.num_kept == 2 and list(r.kept) == [0, 1]
    assert np.array_equal(r.labels, np.arange(n, dtype=np.int32) % 2)
    assert r.rects.tolist() == [[0, 0, n // 2, 1], [0, 1000, n // 2, 1]]


@pytest.mark.gpu
def test_no_stale_scratch(ctx):
    a = ctx.cluster_euclidean(uniform_points(4097), 20.0)
    b = ctx.cluster_euclidean(uniform_points(65), 20.0)
    c = ctx.cluster_euclidean(uniform_points(4097), 20.0)
    same(a, uniform_reference(4097))
    same(b, uniform_reference(65))
    same(c, uniform_reference(4097))
    assert np.array_equal(a.labels, c.labels) and np.array_equal(a.rects, c.rects)


@pytest.mark.gpu
def test_flow_clusterer_members(ctx, mdx):
    pts = tie_grid(160, 120, 3)
    ref = cluster_reference(pts, 10.5)
    fc = mdx.FlowClusterer(context=ctx)
    got = fc.clusterEuclidean([tuple(p) for p in pts], 10.5)
    assert len(got) == len(ref["members"]) >= 1
    for g, m in zip(got, ref["members"]):
        assert g.dtype == np.float32 and np.array_equal(g.view(np.uint32), m.view(np.uint32))
    assert np.array_equal(np.array(mdx.bounding_rects(got), np.int32).reshape(-1, 4), ref["rects"])
    fc.close()
