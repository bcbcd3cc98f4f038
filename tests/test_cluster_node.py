"""The live chain's last stage in both nodes: clusterEuclidean on fitSubspace's outlier points
(ros/src/motion_detection_node.cpp:355), each kept cluster's rectangle
(common/src/optical_flow_visualizer.cpp:223-240) and MotionLogger::writeBoundingBox (node.cpp:431-434).

The C++ node (host/mdx_node) writes clusters_<k>.bin and motion.log; the Python node fills
LiveResult.clusters / rectangles.  Both are compared with the literal-loop checker of
test_cluster.py run on the same frame's outlier points.  The sequence (160 x 120, sigma 0.1,
threshold 50) was chosen on the CPU (oracle.flow_trajectory + oracle.fit_subspace + the checker) so
that every processed frame has a kept cluster; the tests assert that at least one has.
"""
import os

import numpy as np
import pytest

from node_io import log_lines, node_exe, read_clusters, read_outlier_points, rgb8, run_node  # noqa: F401 (node_exe: a fixture)
from test_cluster import cluster_reference

W, H, PS, NM, SIGMA, SEED, THR = 160, 120, 10, 2, 0.1, 20141105, 50.0
TS = 2 * NM + 1


@pytest.fixture(scope="module")
def sequence(mdx):
    a, b, _ = mdx.synth_pair(11, W, H, 3)
    c, d, _ = mdx.synth_pair(12, W, H, 3)
    return [a, b, a, b, a, c, d]


@pytest.mark.gpu
def test_cpp_node_clusters_and_motion_log(node_exe, tmp_path, sequence):
    from motion_detection_amd.formats import MotionLogger
    p, out = run_node(node_exe, tmp_path, rgb8(sequence), live_path=1, egomotion=1, num_motions=NM, sigma=SIGMA, seed=SEED,
                      pixel_step=PS, distance_threshold=THR, log_contours=1)
    assert p.returncode == 0, p.stderr
    nproc = len(sequence) - TS + 1
    assert f"processed {nproc} of {len(sequence)}" in p.stdout
    lg = MotionLogger(str(tmp_path / "py_motion.log"))
    total_kept = 0
    for k in range(nproc):
        outl = read_outlier_points(out / f"res_{k}.bin")
        ref = cluster_reference(outl, THR)
        num_all, labels, kept, rects = read_clusters(out / f"clusters_{k}.bin", len(outl))
        assert num_all == ref["num_all"]
        assert np.array_equal(labels, ref["labels"])
        assert np.array_equal(kept, ref["kept"])
        assert np.array_equal(rects, ref["rects"])
        total_kept += len(kept)
        frame = TS - 1 + k                         # skip_frames 1: global_frame_count_ = the frame's index
        for i, r in enumerate(ref["rects"]):
            lg.writeBoundingBox(tuple(r), frame, i)
    lg.close()
    assert total_kept >= 1                         # else the comparison above is vacuous
    assert open(out / "motion.log", "rb").read() == open(tmp_path / "py_motion.log", "rb").read()
    assert not (out / f"clusters_{nproc}.bin").exists()


@pytest.mark.gpu
def test_cpp_node_without_threshold_writes_no_cluster_files(node_exe, tmp_path, sequence):
    p, out = run_node(node_exe, tmp_path, rgb8(sequence), live_path=1, egomotion=1, num_motions=NM, sigma=SIGMA, seed=SEED,
                      pixel_step=PS)
    assert p.returncode == 0, p.stderr
    names = os.listdir(out)
    assert "res_0.bin" in names
    assert "motion.log" not in names and not [n for n in names if n.startswith("clusters_")]


@pytest.mark.gpu
def test_cpp_node_log_without_kept_cluster_is_empty(node_exe, tmp_path, sequence):
    """log_contours=1 creates motion.log even when no cluster is kept (a threshold no pair passes)."""
    p, out = run_node(node_exe, tmp_path, rgb8(sequence), live_path=1, egomotion=1, num_motions=NM, sigma=SIGMA, seed=SEED,
                      pixel_step=PS, distance_threshold=1e-3, log_contours=1)
    assert p.returncode == 0, p.stderr
    assert (out / "motion.log").read_bytes() == b""
    outl = read_outlier_points(out / "res_0.bin")
    num_all, labels, kept, rects = read_clusters(out / "clusters_0.bin", len(outl))
    assert num_all == len(outl) and len(kept) == 0 and np.array_equal(labels, np.arange(len(outl)))


@pytest.mark.gpu
def test_python_node_fills_clusters_and_rectangles(mdx, sequence, tmp_path):
    from motion_detection_amd.node import Image, MotionDetectionNode
    log = tmp_path / "motion.log"
    node = MotionDetectionNode({"pixel_step": PS, "num_motions": NM, "sigma": SIGMA, "seed": SEED,
                                "distance_threshold": THR, "log_contours": True, "log_path": str(log)})
    plain = MotionDetectionNode({"pixel_step": PS, "num_motions": NM, "sigma": SIGMA, "seed": SEED})
    total_kept = 0
    lines = []
    for fi, f in enumerate(sequence):
        r = node.image_callback(Image.from_array(f, "rgb8"))
        q = plain.image_callback(Image.from_array(f, "rgb8"))
        if r is None:
            assert q is None
            continue
        assert q.clusters == [] and q.rectangles == []
        assert np.array_equal(np.array(q.outlier_points), np.array(r.outlier_points))
        ref = cluster_reference(np.array(r.outlier_points, np.float32).reshape(-1, 2), THR)
        assert len(r.clusters) == len(ref["members"]) == len(r.rectangles)
        for g, m in zip(r.clusters, ref["members"]):
            assert np.array_equal(g.view(np.uint32), m.view(np.uint32))
        assert np.array_equal(np.array(r.rectangles, np.int32).reshape(-1, 4), ref["rects"])
        assert r.frame_number == fi
        lines.append(log_lines(fi, ref["rects"]))
        total_kept += len(r.rectangles)
    assert total_kept >= 1
    node.logger.close()
    assert log.read_text() == "".join(lines)
