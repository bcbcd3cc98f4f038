"""The kept clusters' convex hulls in both nodes (``cluster_contours``): showClusterContours'
cv::convexHull behind every clustering stage (ros/src/motion_detection_node.cpp:393 live, :510 run();
common/src/optical_flow_visualizer.cpp:204-221) and MotionLogger::writeContour (:426-429).

The Python node fills ``contours``; host/mdx_node appends the hulls to its cluster files.  Both are compared
with test_hulls.py's oracle (Andrew's monotone chain on Python ints) run on the same result's clusters, on
the 640 x 480 sequence of test_run_mode.py.  With the parameter absent nothing changes: the existing
byte-for-byte tests cover the default runs; here a run with cluster_contours=0 spelled out equals one
without it, and a run with it differs from that only by the hulls.
"""
import struct

import numpy as np
import pytest

from node_io import dir_bytes, node_exe, read_res, rgb8, run_node  # noqa: F401 (node_exe: a fixture)
from test_hulls import cv_round, hull_oracle

W, H, PS, SEED = 640, 480, 10, 20141105
# (name, the parameters that select the clustering stage): run() (:510), the live chain with and without
# egomotion (:393), the pair path's detectOutliers
CASES = {
    "run": dict(use_all_frames=False, distance_threshold=50.0, seed=SEED, pixel_step=PS, num_motions=2),
    "live_ego": dict(distance_threshold=50.0, seed=SEED, pixel_step=PS, num_motions=2, sigma=0.1),
    "live_no_ego": dict(egomotion=False, distance_threshold=15.0, angular_threshold=0.1, pixel_step=PS),
    "detect_outliers": dict(live_chain=False, egomotion=False, detect_outliers=True, distance_threshold=12.0,
                            angular_threshold=1.0, pixel_step=5, min_vector_size=3.5),
}


@pytest.fixture(scope="module")
def frames(mdx, oracle):
    from traj_seq import sequence
    return sequence(mdx, oracle, W, H, 7, seed=33, channels=3)


def run_python(frames, params):
    from motion_detection_amd.node import Image, MotionDetectionNode
    node = MotionDetectionNode(dict(params))
    out = []
    for fi, f in enumerate(frames):
        r = node.image_callback(Image.from_array(f, "rgb8"))
        if not params.get("use_all_frames", True):
            assert r is None
            r = node.run_once()
        if r is not None:
            out.append((fi, r))
    if node.logger is not None:
        node.logger.close()
    node.ofc.close()
    return out


def oracle_hulls(clusters):
    return [hull_oracle(cv_round(np.asarray(c, np.float32)[:, :2])) for c in clusters]


def as_lists(contours):
    return [list(map(tuple, np.asarray(c).tolist())) for c in contours]


@pytest.fixture(scope="module")
def python_runs(frames):
    """Each case with cluster_contours, once for the module."""
    return {name: run_python(frames, dict(p, cluster_contours=True)) for name, p in CASES.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_python_node_carries_contours(frames, python_runs, name):
    got = python_runs[name]
    plain = run_python(frames, CASES[name])
    assert len(got) == len(plain) >= 1
    total = 0
    for (fi, r), (fj, q) in zip(got, plain):
        assert fi == fj and q.contours == []                       # absent: no new call, no new output
        assert len(r.clusters) == len(q.clusters) and all(np.array_equal(a, b) for a, b in zip(r.clusters, q.clusters))
        assert list(r.rectangles) == list(q.rectangles)
        assert len(r.contours) == len(r.clusters)
        assert all(c.dtype == np.int32 and c.ndim == 2 and c.shape[1] == 2 for c in r.contours)
        assert as_lists(r.contours) == oracle_hulls(r.clusters)
        total += len(r.contours)
    assert total >= 1                                              # else the comparison above is vacuous


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["live_ego", "live_no_ego", "detect_outliers"])
def test_motion_log_rectangles_then_contours(frames, tmp_path, name):
    log = tmp_path / "motion.log"
    got = run_python(frames, dict(CASES[name], cluster_contours=True, log_contours=True, log_path=str(log)))
    expect, total = "", 0
    for fi, r in got:
        for i, (x, y, w, h) in enumerate(r.rectangles):
            expect += f"{fi}, {i}, {x}, {y}, {x + w}, {y + h}\n"
        for i, hull in enumerate(oracle_hulls(r.clusters)):
            expect += f"{fi}, {i}" + "".join(f", {x}, {y}" for x, y in hull) + "\n"
        total += len(r.clusters)
    assert total >= 1
    assert log.read_text() == expect


@pytest.mark.gpu
def test_run_once_logs_nothing(frames, tmp_path):
    log = tmp_path / "motion.log"
    got = run_python(frames, dict(CASES["run"], cluster_contours=True, log_contours=True, log_path=str(log)))
    assert sum(len(r.contours) for _, r in got) >= 1
    assert not log.exists()                                        # run() writes no motion.log


def cpp_params(p):
    q = {k: v for k, v in p.items() if k != "live_chain"}
    q["live_path"] = int(p.get("live_chain", True))
    return q


def read_hull_tail(path, name, res):
    """The hulls at the end of a cluster file (host/mdx_node_main.cpp): i32 offsets[num_kept + 1], then
    i32 xy[offsets[num_kept]][2], behind the labels, kept ids and rectangles; also the file's bytes without
    that tail and the kept clusters' (x, y) members."""
    b = open(path, "rb").read()
    if name in ("run", "live_ego"):
        num_all, k = struct.unpack_from("<2i", b, 0)
        pts = res["outliers"]
        o = 8
    else:
        hdr = 16 if name == "live_no_ego" else 64
        n = struct.unpack_from("<i", b, 0)[0]
        k = struct.unpack_from("<i", b, 28 if name == "detect_outliers" else 12)[0]   # num_kept: the last header int
        pts = np.frombuffer(b, np.float64, 4 * n, hdr).reshape(n, 4)[:, :2].astype(np.float32)
        o = hdr + 32 * n + (n if name == "detect_outliers" else 0)
    n = len(pts)
    labels = np.frombuffer(b, np.int32, n, o)
    kept = np.frombuffer(b, np.int32, k, o + 4 * n)
    base = o + 4 * n + 4 * k + 16 * k
    offsets = np.frombuffer(b, np.int32, k + 1, base)
    assert offsets[0] == 0 and np.all(np.diff(offsets) >= 1)
    assert len(b) == base + 4 * (k + 1) + 8 * int(offsets[-1])
    xy = np.frombuffer(b, np.int32, 2 * int(offsets[-1]), base + 4 * (k + 1)).reshape(-1, 2)
    hulls = [list(map(tuple, xy[offsets[i]:offsets[i + 1]].tolist())) for i in range(k)]
    return hulls, b[:base], [pts[labels == int(c)] for c in kept]


FILES = {"run": "clusters", "live_ego": "clusters", "live_no_ego": "vclusters", "detect_outliers": "outliers"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_cpp_node_files_match_the_python_node(node_exe, tmp_path, frames, python_runs, name):
    params = cpp_params(CASES[name])
    (tmp_path / "on").mkdir()
    (tmp_path / "off").mkdir()
    (tmp_path / "zero").mkdir()
    p, out = run_node(node_exe, tmp_path / "on", rgb8(frames), cluster_contours=1, log_contours=1, **params)
    q, off = run_node(node_exe, tmp_path / "off", rgb8(frames), log_contours=1, **params)
    z, zero = run_node(node_exe, tmp_path / "zero", rgb8(frames), cluster_contours=0, log_contours=1, **params)
    assert p.returncode == 0 and q.returncode == 0 and z.returncode == 0, p.stderr + q.stderr + z.stderr
    a, b = dir_bytes(str(out)), dir_bytes(str(off))
    assert dir_bytes(str(zero)) == b and z.stdout == q.stdout      # the parameter at its default: nothing changes
    assert sorted(a) == sorted(b) and p.stdout == q.stdout
    got = python_runs[name]
    assert f"processed {len(got)} of {len(frames)}" in p.stdout
    expect_log, total = "", 0
    for k, (fi, r) in enumerate(got):
        fname = f"{FILES[name]}_{k}.bin"
        res = read_res(out / f"res_{k}.bin", live=name != "detect_outliers")
        hulls, head, members = read_hull_tail(out / fname, name, res)
        assert head == b[fname]                                    # the file grew by its tail, nothing else
        assert hulls == as_lists(r.contours) == oracle_hulls(members)
        total += len(hulls)
        if name != "run":                                          # run() logs nothing
            for i, (x, y, w, h) in enumerate(r.rectangles):
                expect_log += f"{fi}, {i}, {x}, {y}, {x + w}, {y + h}\n"
            for i, hull in enumerate(hulls):
                expect_log += f"{fi}, {i}" + "".join(f", {x}, {y}" for x, y in hull) + "\n"
    assert total >= 1
    assert a["motion.log"].decode() == expect_log
    for n in a:                                                    # every other file is byte-identical
        if not n.startswith(FILES[name]) and n != "motion.log":
            assert a[n] == b[n], n
