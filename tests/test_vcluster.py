"""FlowClusterer::getClusters + boundingRect on the device (mdx_cluster_vectors).

Reference: getClusters (common/src/flow_clusterer.cpp:178-227), the distance and the angular distance
(common/src/vector_cluster.cpp:25-50, :118-139), the rectangles (ros/src/motion_detection_node.cpp:376-395).
Restated from the source; unpinned against a real build (no OpenCV 2.4 to run).

The checker below is the reference's literal loop: clusters are member lists in creation order, a
vector joins the first cluster whose smallest distance and whose smallest angular distance (two
separate minima) both pass, the distance as np.sqrt of the unfused double expression, the angular
distance as the reference's own composite |atan2(sin d, cos d)| (np.trunc of it under ABS_INT).  It
uses neither the device's root sets nor its wrap formula, so the two check each other.  The two
angle formulas agree to a few ulp only, so the checker also returns the smallest distance of any
angular value from its decision boundary, and every GPU case asserts that margin >= MARGIN: the
inputs (seeds, hand-made angles) are chosen so that it holds.  Every device output must then equal
the checker exactly.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_cluster import reference_rects

MARGIN = 1e-9
TWO_PI = 2 * np.pi


def angles_of(vec):
    th = np.arctan2(vec[:, 3], vec[:, 2])               # getAngle (vector_cluster.cpp:131-139)
    return np.where(th < 0.0, th + TWO_PI, th)


def vcluster_reference(vectors, thr, athr, min_size=5, abs_int=False, variant=None):
    """The literal first-fit loop.  variant: a wrong reading the CPU tests must tell apart --
    "same_member" (one member must pass both tests) or "nearest" (the qualifying cluster whose
    nearest member is nearest, not the earliest)."""
    vec = np.ascontiguousarray(vectors, np.float64).reshape(-1, 4)
    n = len(vec)
    thr, athr = float(thr), float(athr)
    active = np.nonzero((np.abs(vec[:, 2]) > 0) | (np.abs(vec[:, 3]) > 0))[0]
    x, y, th = vec[active, 0], vec[active, 1], angles_of(vec[active])
    na = len(active)
    lab = np.zeros(na, np.int64)
    clusters = []                                       # member lists (active indices), creation order
    margin = np.inf
    for i in range(na):
        index = -1
        if i:
            dx, dy = x[i] - x[:i], y[i] - y[:i]
            with np.errstate(over="ignore"):
                d = np.sqrt(dx * dx + dy * dy)              # numpy does not fuse
            dl = th[i] - th[:i]
            a = np.abs(np.arctan2(np.sin(dl), np.cos(dl)))
            if abs_int:
                margin = min(margin, float(np.min(np.abs(a[:, None] - np.array([1.0, 2.0, 3.0])))))
                a = np.trunc(a)
            else:
                margin = min(margin, float(np.min(np.abs(a - athr))))
            nc = len(clusters)
            if variant == "same_member":
                ok = np.zeros(nc, bool)
                ok[lab[:i][(d < thr) & (a < athr)]] = True
                q = np.nonzero(ok)[0]
            else:
                dk, ak = np.full(nc, np.inf), np.full(nc, np.inf)
                np.minimum.at(dk, lab[:i], d)               # getClosestDistance of every cluster
                np.minimum.at(ak, lab[:i], a)               # getClosestOrientation of every cluster
                q = np.nonzero((dk < thr) & (ak < athr))[0]
                if variant == "nearest" and len(q):
                    q = q[[int(np.argmin(dk[q]))]]
            if len(q):
                index = int(q[0])                           # the first that qualifies (:189-198)
        if index < 0:
            index = len(clusters)
            clusters.append([])
        clusters[index].append(i)
        lab[i] = index
    labels = np.full(n, -1, np.int32)
    labels[active] = lab
    kept = [k for k, m in enumerate(clusters) if len(m) > min_size]
    members = [vec[active[clusters[k]]] for k in kept]
    rects = reference_rects([m[:, :2].astype(np.float32) for m in members])
    return dict(labels=labels, num_active=na, num_all=len(clusters), kept=np.array(kept, np.int32).reshape(-1),
                rects=rects, members=members, margin=margin)


def vecs(rows):
    return np.array(rows, np.float64).reshape(-1, 4)


def polar(x, y, ang, mag=2.0):
    return (x, y, mag * np.cos(ang), mag * np.sin(ang))


# ---------------------------------------------------------------- inputs of the GPU cases

SIZES = [0, 1, 5, 6, 7, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 769, 1025, 2100]
GRID_THR, GRID_ATHR = 15.0, 0.15
UNI_THR, UNI_ATHR = 60.0, 0.5


@functools.lru_cache(maxsize=None)
def grid_input(n):
    """The first n points of a 640 x 480 grid at step 10 in visiting order (rows outer); the flow of
    three coherent directions by image column band, plus noise."""
    rng = np.random.default_rng(7000 + n)
    ys, xs = np.meshgrid(np.arange(0, 480, 10.0), np.arange(0, 640, 10.0), indexing="ij")
    x, y = xs.ravel()[:n], ys.ravel()[:n]
    base = np.choose((x // 220).astype(int), [0.3, 2.4, 5.5])
    ang = base + rng.normal(0, 0.08, n)
    mag = rng.uniform(2, 5, n)
    return np.stack([x, y, mag * np.cos(ang), mag * np.sin(ang)], 1)


@functools.lru_cache(maxsize=None)
def uniform_input(n):
    rng = np.random.default_rng(9000 + n)
    p = rng.uniform(0, [640, 480], (n, 2))
    ang = rng.uniform(0, TWO_PI, n)
    mag = rng.uniform(1, 4, n)
    return np.concatenate([p, (mag * np.cos(ang))[:, None], (mag * np.sin(ang))[:, None]], 1)


@functools.lru_cache(maxsize=None)
def holes_input(n):
    """uniform_input(n) with inactive (x, y, 0, 0) and (-1, -1, 0, 0) entries interleaved; returns
    the vectors and the input index of each active one."""
    rng = np.random.default_rng(11000 + n)
    act = uniform_input(n)
    total = n + n // 2 + 3
    where = np.sort(rng.choice(total, n, replace=False))
    out = np.zeros((total, 4))
    out[:, :2] = rng.uniform(0, 640, (total, 2))
    out[::3, :2] = -1.0
    out[:, 2:] = 0.0
    out[where] = act
    return out, where


@functools.lru_cache(maxsize=None)
def grid_reference(n):
    return vcluster_reference(grid_input(n), GRID_THR, GRID_ATHR)


@functools.lru_cache(maxsize=None)
def uniform_reference(n, abs_int=False):
    return vcluster_reference(uniform_input(n), UNI_THR, UNI_ATHR, abs_int=abs_int)


def cross_block_input(s_off, q_off):
    """Three groups 500 px apart (threshold 10, 0.15 rad), the fillers far singletons with the
    opposite angle.  Per group a member P (angle 0), a supplier S and a query Q:
      group 0: P in block 0, S (5 px from P, angle 0.1) and Q in block 2; Q is 12 px from P and 7
               from S, 0.1 from P and 0.2 from S: near through S (its own block), angle through P.
      group 1: the mirror: Q is 8 px from P and 16 from S, 0.24 from P and 0.12 from S.
      group 2: P, S and Q all in block 2: both contributions in-block."""
    n = 3 * 256
    v = np.zeros((n, 4))
    for k in range(n):
        v[k] = polar(10000.0 + 100.0 * k, -5000.0, np.pi)
    b2 = 512
    v[0] = polar(0, 0, 0.0)
    v[b2 + s_off] = polar(5, 0, 0.1)
    v[b2 + q_off] = polar(12, 0, -0.1)
    v[1] = polar(0, 500, 0.0)
    v[b2 + s_off + 1] = polar(8, 500, 0.12)
    v[b2 + q_off + 1] = polar(-8, 500, 0.24)
    v[b2 + s_off + 2] = polar(0, 1000, 0.0)
    v[b2 + s_off + 3] = polar(5, 1000, 0.1)
    v[b2 + q_off + 2] = polar(12, 1000, -0.1)
    return v, (0, b2 + s_off, b2 + q_off), (1, b2 + s_off + 1, b2 + q_off + 1), (b2 + s_off + 2, b2 + s_off + 3, b2 + q_off + 2)


CROSS_OFFSETS = [(0, 4), (3, 70), (60, 200), (130, 252)]


def chain_input(order, n=600):
    idx = np.arange(n)
    if order == "zigzag":                               # 0, n-1, 1, n-2, ...
        z = np.empty(n, np.int64)
        z[0::2] = idx[: (n + 1) // 2]
        z[1::2] = idx[::-1][: n // 2]
        idx = z
    return np.stack([idx.astype(np.float64), np.zeros(n), np.full(n, 2.0), np.full(n, 1.0)], 1)


def row(n, x0=0.0, ang=0.3):
    return vecs([polar(x0 + i, 0.0, ang) for i in range(n)])


# ---------------------------------------------------------------- CPU: the checker itself

def test_checker_split_minima():
    """Cluster A holds a member 5 px from the query whose angle is 3.0 away, and a member 995 px away
    whose angle is 0.01 away: the two minima are taken separately, so the query joins A."""
    k = 31                                               # A: a row of members 33 px apart, from (0, 0) at angle
    ang = np.linspace(3.2, 0.21, k)                      # 3.2 to (1000, 0) at angle 0.21, turning 0.1 per member
    assert np.all(np.abs(np.diff(ang)) < 0.12)
    v = vecs([polar(1000.0 * j / (k - 1), 0, ang[j]) for j in range(k)] + [polar(5, 0, 0.2)])
    r = vcluster_reference(v, 40, 0.15)
    assert list(r["labels"][:k]) == [0] * k
    assert r["labels"][k] == 0 and r["num_all"] == 1
    w = vcluster_reference(v, 40, 0.15, variant="same_member")
    assert list(w["labels"][:k]) == [0] * k and w["labels"][k] == 1 and w["num_all"] == 2
    assert r["margin"] >= MARGIN


def test_checker_first_fit_not_nearest():
    """The query qualifies for cluster 0 (9 px away) and for the later cluster 1 (2 px away): it
    joins the earlier one."""
    v = vecs([polar(0, 0, 0.3), polar(11, 0, 0.3), polar(9, 0, 0.3)])
    assert list(vcluster_reference(v, 10, 0.15)["labels"]) == [0, 1, 0]
    assert list(vcluster_reference(v, 10, 0.15, variant="nearest")["labels"]) == [0, 1, 1]
    v = vecs([polar(0, 0, 0.3), polar(20, 0, 0.3), polar(11, 0, 0.3)])
    assert list(vcluster_reference(v, 10, 0.15)["labels"]) == [0, 1, 1]     # 11 from cluster 0: only 1 qualifies


def test_checker_one_test_alone_starts_a_cluster():
    near_only = vecs([polar(0, 0, 0.3), polar(5, 0, 1.3)])
    angle_only = vecs([polar(0, 0, 0.3), polar(50, 0, 0.3)])
    both = vecs([polar(0, 0, 0.3), polar(5, 0, 0.35)])
    assert vcluster_reference(near_only, 10, 0.15)["num_all"] == 2
    assert vcluster_reference(angle_only, 10, 0.15)["num_all"] == 2
    assert vcluster_reference(both, 10, 0.15)["num_all"] == 1


def test_checker_wrap():
    v = vecs([polar(0, 0, 0.05), polar(1, 0, TWO_PI - 0.05)])
    assert angles_of(v)[1] > 6.2
    r = vcluster_reference(v, 10, 0.15)
    assert r["num_all"] == 1 and abs(r["margin"] - 0.05) < 1e-12      # 0.1 apart
    assert vcluster_reference(v, 10, 0.09)["num_all"] == 2


def test_checker_abs_int():
    a = vecs([polar(0, 0, 0.2), polar(1, 0, 1.1)])          # 0.9 apart
    assert vcluster_reference(a, 10, 0.15)["num_all"] == 2
    assert vcluster_reference(a, 10, 0.15, abs_int=True)["num_all"] == 1
    b = vecs([polar(0, 0, 0.2), polar(1, 0, 1.3)])          # 1.1 apart
    assert vcluster_reference(b, 10, 0.15)["num_all"] == 2
    assert vcluster_reference(b, 10, 0.15, abs_int=True)["num_all"] == 2
    assert abs(vcluster_reference(a, 10, 0.15, abs_int=True)["margin"] - 0.1) < 1e-12


def test_checker_inactive_and_kept():
    v = np.concatenate([row(3), vecs([(1, 0, 0, 0), (-1, -1, 0, 0)]), row(3, 3.0)])
    r = vcluster_reference(v, 1.5, 0.15)
    assert list(r["labels"]) == [0, 0, 0, -1, -1, 0, 0, 0] and r["num_active"] == 6
    assert list(r["kept"]) == [0] and r["rects"].tolist() == [[0, 0, 6, 1]]
    assert len(vcluster_reference(v[:7], 1.5, 0.15)["kept"]) == 0     # 5 members: not kept


def test_cross_block_inputs_have_teeth():
    for s_off, q_off in CROSS_OFFSETS:
        v, g0, g1, g2 = cross_block_input(s_off, q_off)
        r = vcluster_reference(v, 10, 0.15)
        w = vcluster_reference(v, 10, 0.15, variant="same_member")
        assert r["margin"] >= MARGIN
        for p, s, q in (g0, g1, g2):
            assert r["labels"][p] == r["labels"][s] == r["labels"][q]
            assert w["labels"][p] == w["labels"][s] != w["labels"][q]


def test_get_clusters_gathers_rows_outer():
    """getClusters visits image rows outer (flow_clusterer.cpp:180-184); on this image the x-major
    order of the flow entries gives another partition: (0, 10) at angle 0.4 is 0.3 from (0, 0) and,
    x-major, meets it alone; rows outer, it meets (10, 0) and (20, 0) first, whose angles bridge."""
    from motion_detection_amd.flow_clusterer import grid_vectors
    ang = [[0.7, 0.6, 0.5], [0.4, 0.4, 0.3], [0.3, 0.3, 0.3]]           # [row][column]
    img = np.zeros((30, 30, 4))
    for r in range(3):
        for c in range(3):
            img[10 * r, 10 * c] = polar(10 * c, 10 * r, ang[r][c])
    img[5, 5] = polar(5, 5, 1.0)                             # off the grid: not visited
    g = grid_vectors(img, 10)
    assert g.shape == (9, 4) and g.flags.c_contiguous and g[:4, :2].tolist() == [[0, 0], [10, 0], [20, 0], [0, 10]]
    a = vcluster_reference(g, 10.5, 0.15)
    xm = img[::10, ::10].transpose(1, 0, 2).reshape(-1, 4)
    b = vcluster_reference(xm, 10.5, 0.15)
    assert a["labels"].reshape(3, 3).tolist() == [[0, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert b["labels"].reshape(3, 3).T.tolist() == [[0, 0, 0], [1, 1, 1], [1, 1, 1]]
    assert min(a["margin"], b["margin"]) > 1e-3
    with pytest.raises(ValueError):
        grid_vectors(np.zeros((30, 30, 3)), 10)


def test_null_context_is_einval(mdx):
    L = mdx.lib()
    v = row(4)
    rc = L.mdx_cluster_vectors(None, v.ctypes.data_as(C.c_void_p), 4, 1.0, 0.15, 5, 0, None, None, None, None, None, 0,
                               None)
    assert rc == mdx._lib.MDX_EINVAL


class StubClusterer:
    """Records the node's calls; getClusters returns one cluster of six vectors."""

    def __init__(self):
        self.calls = []

    def getClusters(self, vec, pixel_step, thr, athr, abs_int=False):
        self.calls.append(("getClusters", vec.shape, pixel_step, thr, athr, abs_int))
        return [np.array([polar(10 * k, 20, 0.3) for k in range(6)])]

    def clusterEuclidean(self, points, thr):
        self.calls.append(("clusterEuclidean", thr))
        return []


class StubCalculator:
    def calculateOpticalFlowTrajectory(self, images, vec, trajectories, pixel_step, _unused, mvs):
        trajectories.append(np.zeros((len(images), 2), np.float32))
        return 1


class StubDetector:
    def fitSubspace(self, trajectories, outliers, num_motions, sigma):
        return []


def stub_node(params):
    """A MotionDetectionNode whose calculator, detector and clusterer are the stubs above (its
    constructor would create a device context)."""
    from motion_detection_amd.node import MotionDetectionNode
    node = MotionDetectionNode.__new__(MotionDetectionNode)
    node.params = {"pixel_step": 10, "min_vector_size": 1.0, "skip_frames": 1, "num_motions": 2, "egomotion": False,
                   "use_all_frames": True, "sigma": 0.5, "live_chain": True, "distance_threshold": None,
                   "log_contours": False, "log_path": "", "angular_threshold": None, "abs_int": False}
    node.params.update(params)
    node.on_result = None
    node.global_frame_count = 7
    node.frames_processed = 0
    node.ofc, node.od, node.fc = StubCalculator(), StubDetector(), StubClusterer()
    node.logger = None
    node._device = 0
    return node


def test_node_stage_is_off_by_default_and_on_with_both_thresholds(tmp_path):
    import inspect

    from motion_detection_amd.node import MotionDetectionNode
    src = inspect.getsource(MotionDetectionNode.__init__)
    assert '"angular_threshold": None' in src and '"abs_int": False' in src     # the defaults: stage off
    frames = [np.zeros((40, 40, 3), np.uint8)] * 2
    for params in ({}, {"distance_threshold": 50.0}, {"angular_threshold": 0.15}):
        node = stub_node(params)
        r = node.run_live_chain(frames)
        assert node.fc.calls == []
        assert r.vector_clusters == [] and r.clusters == [] and r.rectangles == []
    # with egomotion the thresholds select clusterEuclidean, as before
    node = stub_node({"distance_threshold": 50.0, "angular_threshold": 0.15, "egomotion": True})
    r = node.run_live_chain(frames)
    assert node.fc.calls == [("clusterEuclidean", 50.0)] and r.vector_clusters == []
    log = tmp_path / "motion.log"
    node = stub_node({"distance_threshold": 50.0, "angular_threshold": 0.15, "abs_int": True, "log_contours": True,
                      "log_path": str(log)})
    r = node.run_live_chain(frames)
    assert node.fc.calls == [("getClusters", (40, 40, 4), 10, 50.0, 0.15, True)]
    assert len(r.vector_clusters) == 1 and r.vector_clusters[0].shape == (6, 4)
    assert len(r.clusters) == 1 and r.clusters[0].dtype == np.float32 and r.clusters[0].shape == (6, 2)
    assert r.rectangles == [(0, 20, 51, 1)] and r.frame_number == 7
    node.logger.close()
    assert log.read_text() == "7, 0, 0, 20, 51, 21\n"


# ---------------------------------------------------------------- GPU: the device against the checker

AA32 = np.frombuffer(b"\xaa" * 4, np.int32)[0]


def run(ctx, vectors, thr, athr, min_size=5, abs_int=False, max_kept=None):
    """mdx_cluster_vectors with every output prefilled with 0xAA; what it wrote."""
    from motion_detection_amd._lib import VCLUSTER_ABS_INT, lib
    vec = np.ascontiguousarray(vectors, np.float64).reshape(-1, 4)
    n = len(vec)
    cap = n // (min_size + 1) + 2 if max_kept is None else max_kept
    labels = np.full(n + 2, AA32, np.int32)
    kept = np.full(cap + 2, AA32, np.int32)
    rects = np.full((cap + 2, 4), AA32, np.int32)
    cnt = [C.c_int(int(AA32)) for _ in range(3)]
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = lib().mdx_cluster_vectors(ctx._h, vp(vec) if n else None, n, float(thr), float(athr), min_size,
                                   VCLUSTER_ABS_INT if abs_int else 0, vp(labels), C.byref(cnt[0]), C.byref(cnt[1]),
                                   vp(kept), vp(rects), cap, C.byref(cnt[2]))
    assert rc == 0, lib().mdx_last_error(ctx._h)
    return dict(labels=labels, num_active=cnt[0].value, num_all=cnt[1].value, kept=kept, rects=rects,
                num_kept=cnt[2].value, n=n, cap=cap)


def same(out, ref):
    assert ref["margin"] >= MARGIN, ref["margin"]          # else the two angle formulas may disagree
    n, nk = out["n"], len(ref["kept"])
    assert out["num_active"] == ref["num_active"] and out["num_all"] == ref["num_all"] and out["num_kept"] == nk
    assert np.array_equal(out["labels"][:n], ref["labels"])
    m = min(nk, out["cap"])
    assert np.array_equal(out["kept"][:m], ref["kept"][:m])
    assert np.array_equal(out["rects"][:m], ref["rects"][:m])
    # nothing is written past the arrays' ends, nor past what was kept
    assert np.all(out["labels"][n:] == AA32) and np.all(out["kept"][m:] == AA32) and np.all(out["rects"][m:] == AA32)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_sizes_grid(ctx, n):
    same(run(ctx, grid_input(n), GRID_THR, GRID_ATHR), grid_reference(n))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_sizes_uniform(ctx, n):
    ref = uniform_reference(n)
    if n >= 511:
        assert ref["num_all"] < ref["num_active"] // 2       # clusters do form
    same(run(ctx, uniform_input(n), UNI_THR, UNI_ATHR), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_sizes_with_inactive_entries(ctx, n):
    v, where = holes_input(n)
    base = uniform_reference(n)
    labels = np.full(len(v), -1, np.int32)
    labels[where] = base["labels"]
    ref = dict(base, labels=labels)
    assert ref["num_active"] == n and len(v) > n
    same(run(ctx, v, UNI_THR, UNI_ATHR), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [n for n in SIZES if n >= 5])
def test_abs_int_uniform(ctx, n):
    ref = uniform_reference(n, True)
    if n >= 255:
        assert ref["num_all"] < uniform_reference(n)["num_all"]   # the truncation joins far more
    same(run(ctx, uniform_input(n), UNI_THR, UNI_ATHR, abs_int=True), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("s_off,q_off", CROSS_OFFSETS)
def test_cross_block_contributions(ctx, s_off, q_off):
    v, g0, g1, g2 = cross_block_input(s_off, q_off)
    ref = vcluster_reference(v, 10, 0.15)
    out = run(ctx, v, 10, 0.15)
    same(out, ref)
    for p, s, q in (g0, g1, g2):
        assert out["labels"][p] == out["labels"][s] == out["labels"][q]


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["forward", "zigzag"])
def test_deep_chain(ctx, order):
    v = chain_input(order)
    ref = vcluster_reference(v, 1.5, 0.15)
    if order == "forward":
        assert ref["num_all"] == 1 and ref["rects"].tolist() == [[0, 0, 600, 1]]
    same(run(ctx, v, 1.5, 0.15), ref)


@pytest.mark.gpu
def test_distance_threshold_edge(ctx):
    """A pair exactly at the threshold does not join (strict <); one ulp above it, it does.  The
    distances include roots that no double holds exactly."""
    pairs = [((0, 0), (3, 4)), ((0, 0), (1, 1)), ((0, 0), (1, 2)), ((0.1, 0.2), (0.4, 0.7)), ((-7.3, 2.9), (11.1, -5.7))]
    for (ax, ay), (bx, by) in pairs:
        v = vecs([polar(ax, ay, 0.3), polar(bx, by, 0.3)])
        dx, dy = np.float64(ax) - np.float64(bx), np.float64(ay) - np.float64(by)
        d = float(np.sqrt(dx * dx + dy * dy))
        for thr, joined in [(d, False), (float(np.nextafter(d, np.inf)), True), (float(np.nextafter(d, 0)), False)]:
            ref = vcluster_reference(v, thr, 0.15)
            assert ref["num_all"] == (1 if joined else 2)
            same(run(ctx, v, thr, 0.15), ref)
    dup = vecs([polar(3, 3, 0.3)] * 7)                       # d = 0 < a tiny threshold
    ref = vcluster_reference(dup, 1e-200, 0.15)
    assert ref["num_all"] == 1 and list(ref["kept"]) == [0]
    same(run(ctx, dup, 1e-200, 0.15), ref)
    same(run(ctx, uniform_input(65), float("inf"), UNI_ATHR), vcluster_reference(uniform_input(65), float("inf"), UNI_ATHR))


@pytest.mark.gpu
@pytest.mark.parametrize("thr,athr", [(0.0, 0.5), (-1.0, 0.5), (60.0, 0.0), (60.0, -1.0), (0.0, 0.0)])
def test_thresholds_not_positive(ctx, thr, athr):
    v = uniform_input(257)
    ref = vcluster_reference(v, thr, athr)
    assert ref["num_all"] == 257                            # every active vector is its own cluster
    ref["margin"] = np.inf                                  # no angular value can pass: nothing to be close to
    same(run(ctx, v, thr, athr), ref)


@pytest.mark.gpu
def test_min_size_edge(ctx):
    for n, nkept in [(5, 0), (6, 1)]:
        ref = vcluster_reference(row(n), 1.5, 0.15)
        assert ref["num_all"] == 1 and len(ref["kept"]) == nkept
        same(run(ctx, row(n), 1.5, 0.15), ref)
    ref = vcluster_reference(row(6), 1.5, 0.15, min_size=6)
    assert len(ref["kept"]) == 0
    same(run(ctx, row(6), 1.5, 0.15, min_size=6), ref)


@pytest.mark.gpu
def test_max_kept_smaller_than_num_kept(ctx):
    v = grid_input(769)
    ref = vcluster_reference(v, GRID_THR, GRID_ATHR, min_size=1)
    assert len(ref["kept"]) >= 3
    for cap in (2, 0):
        out = run(ctx, v, GRID_THR, GRID_ATHR, min_size=1, max_kept=cap)
        assert out["num_kept"] == len(ref["kept"]) > cap
        same(out, ref)                                      # the first `cap` entries, nothing past them


@pytest.mark.gpu
def test_bad_arguments(ctx, mdx):
    from motion_detection_amd._lib import lib
    E = mdx._lib.MDX_EINVAL
    v = uniform_input(65).copy()

    def call(p, n, thr=60.0, athr=0.5, flags=0, max_kept=0):
        return lib().mdx_cluster_vectors(ctx._h, None if p is None else p.ctypes.data_as(C.c_void_p), n, thr, athr, 5,
                                         flags, None, None, None, None, None, max_kept, None)
    assert call(v, -1) == E
    assert call(v, 65, max_kept=-1) == E
    assert call(None, 3) == E
    assert call(None, 0) == 0
    assert call(v, 65, thr=float("nan")) == E
    assert call(v, 65, athr=float("nan")) == E
    assert call(v, mdx._lib.VCLUSTER_MAX_POINTS + 1) == E
    assert call(v, 65, flags=2) == E and call(v, 65, flags=3) == E and call(v, 65, flags=-1) == E
    for col in range(4):
        for bad in (np.nan, np.inf, -np.inf):
            q = v.copy()
            q[40, col] = bad
            assert call(q, 65) == E
    assert call(v, 65) == 0 and call(v, 65, flags=1) == 0   # every output NULL


@pytest.mark.gpu
def test_no_stale_scratch(ctx):
    a = run(ctx, uniform_input(2100), UNI_THR, UNI_ATHR)
    b = run(ctx, uniform_input(65), UNI_THR, UNI_ATHR)
    g = run(ctx, grid_input(513), GRID_THR, GRID_ATHR)
    c = run(ctx, uniform_input(2100), UNI_THR, UNI_ATHR)
    same(a, uniform_reference(2100))
    same(b, uniform_reference(65))
    same(g, grid_reference(513))
    same(c, uniform_reference(2100))


@pytest.mark.gpu
def test_max_points_known_answer(ctx, mdx):
    """The largest call (512 blocks: the largest LDS sets and scan rows), too large for the O(n^2)
    checker: two rows 1000 apart with opposite flow, their vectors 1 apart and interleaved in input
    order, thresholds 1.5 and 0.15 -- two clusters, labels alternating."""
    n = mdx._lib.VCLUSTER_MAX_POINTS
    k = np.arange(n // 2, dtype=np.float64)
    v = np.zeros((n, 4))
    v[0::2] = np.stack([k, np.zeros_like(k), np.full_like(k, 2.0), np.full_like(k, 0.5)], 1)
    v[1::2] = np.stack([k, np.full_like(k, 1000.0), np.full_like(k, -2.0), np.full_like(k, 0.5)], 1)
    r = ctx.cluster_vectors(v, 1.5, 0.15)
    assert (r.num_active, r.num_all, r.num_kept) == (n, 2, 2) and list(r.kept) == [0, 1]
    assert np.array_equal(r.labels, np.arange(n, dtype=np.int32) % 2)
    assert r.rects.tolist() == [[0, 0, n // 2, 1], [0, 1000, n // 2, 1]]


@pytest.mark.gpu
def test_context_method_and_no_active_vector(ctx):
    r = ctx.cluster_vectors(vecs([(3, 4, 0, 0), (-1, -1, 0, 0)]), 10, 0.15)
    assert list(r.labels) == [-1, -1] and (r.num_active, r.num_all, r.num_kept) == (0, 0, 0) and r.rects.shape == (0, 4)
    ref = grid_reference(257)
    r = ctx.cluster_vectors(grid_input(257), GRID_THR, GRID_ATHR)
    assert np.array_equal(r.labels, ref["labels"]) and (r.num_active, r.num_all) == (257, ref["num_all"])
    assert np.array_equal(r.kept, ref["kept"]) and np.array_equal(r.rects, ref["rects"]) and r.num_kept == len(ref["kept"])


@pytest.mark.gpu
def test_flow_clusterer_members(ctx, mdx):
    """FlowClusterer.getClusters on a 160 x 120 Vec4d image: the kept clusters' members."""
    from motion_detection_amd.flow_clusterer import grid_vectors
    rng = np.random.default_rng(5)
    img = np.zeros((120, 160, 4))
    img[..., 0] = rng.uniform(0, 160, (120, 160))           # off-grid pixels hold junk that must not be read
    img[..., 2] = 1.0
    for yy in range(0, 120, 10):
        for xx in range(0, 160, 10):
            ang = (0.4 if xx < 80 else 3.0) + rng.normal(0, 0.05)
            img[yy, xx] = polar(xx + rng.uniform(0, 1), yy + rng.uniform(0, 1), ang) if rng.random() < 0.8 else (xx, yy, 0, 0)
    ref = vcluster_reference(grid_vectors(img, 10), 15.0, 0.15)
    assert ref["margin"] >= MARGIN and len(ref["members"]) >= 2
    fc = mdx.FlowClusterer(context=ctx)
    got = fc.getClusters(img, 10, 15.0, 0.15)
    assert len(got) == len(ref["members"])
    for g, m in zip(got, ref["members"]):
        assert g.dtype == np.float64 and np.array_equal(g, m)
    assert np.array_equal(fc.last.rects, ref["rects"])
    fc.close()
