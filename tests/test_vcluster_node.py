"""The live callback without egomotion in both nodes: FlowClusterer::getClusters on the trajectory
pass's Vec4d image (ros/src/motion_detection_node.cpp:375), each kept cluster's points and rectangle
(:376-395) and MotionLogger::writeBoundingBox (:431-434).

The C++ node (host/mdx_node) writes vclusters_<k>.bin and motion.log; the Python node fills
LiveResult.vector_clusters / clusters / rectangles.  Both are compared with the literal-loop checker
of test_vcluster.py run on the vector image the node itself reports, on tests/golden/synth_160x120_rgb
played back and forth.  Thresholds 15 px / 0.1 rad were chosen on the CPU (oracle.flow_trajectory +
the checker) so that every processed frame has several clusters, one of them kept, and no angular
value within 1e-9 of the threshold; the tests assert all of that on what the device reports.
"""
import os

import numpy as np
import pytest

from node_io import ROOT, log_lines, node_exe, read_vclusters, rgb8, run_node  # noqa: F401 (node_exe: a fixture)
from test_vcluster import MARGIN, vcluster_reference

W, H, PS, THR, ATHR = 160, 120, 10, 15.0, 0.1


@pytest.fixture(scope="module")
def sequence():
    g = np.load(os.path.join(ROOT, "tests", "golden", "synth_160x120_rgb.npz"))
    return [g["img1"], g["img2"], g["img1"], g["img2"]]


@pytest.mark.gpu
@pytest.mark.parametrize("abs_int", [0, 1])
def test_cpp_node_vector_clusters_and_motion_log(node_exe, tmp_path, sequence, abs_int):
    p, out = run_node(node_exe, tmp_path, rgb8(sequence), live_path=1, egomotion=0, pixel_step=PS, distance_threshold=THR,
                      angular_threshold=ATHR, abs_int=abs_int, log_contours=1)
    assert p.returncode == 0, p.stderr
    nproc = len(sequence) - 1                          # a ring of 2 frames
    assert f"processed {nproc} of {len(sequence)}" in p.stdout
    expect, total_kept, total_all = "", 0, 0
    for k in range(nproc):
        vec, nact, num_all, labels, kept, rects = read_vclusters(out / f"vclusters_{k}.bin")
        assert len(vec) == (W // PS) * (H // PS) and vec[:3, :2].tolist() == [[0, 0], [10, 0], [20, 0]]   # rows outer
        ref = vcluster_reference(vec, THR, ATHR, abs_int=bool(abs_int))
        assert ref["margin"] >= MARGIN, ref["margin"]
        assert (nact, num_all) == (ref["num_active"], ref["num_all"])
        assert np.array_equal(labels, ref["labels"])
        assert np.array_equal(kept, ref["kept"]) and np.array_equal(rects, ref["rects"])
        total_kept += len(kept)
        total_all += num_all
        expect += log_lines(1 + k, ref["rects"])       # skip_frames 1: global_frame_count_ = the frame's index
    assert total_kept >= 1                             # else the comparison above is vacuous
    if not abs_int:
        assert total_all > nproc                       # more than one cluster: the angle test separates
    assert (out / "motion.log").read_text() == expect
    assert not [n for n in os.listdir(out) if n.startswith("clusters_")]


@pytest.mark.gpu
def test_cpp_node_without_angular_threshold_writes_no_file(node_exe, tmp_path, sequence):
    p, out = run_node(node_exe, tmp_path, rgb8(sequence), live_path=1, egomotion=0, pixel_step=PS, distance_threshold=THR)
    assert p.returncode == 0, p.stderr
    names = os.listdir(out)
    assert "res_0.bin" in names and "motion.log" not in names
    assert not [n for n in names if n.startswith("vclusters_") or n.startswith("clusters_")]


@pytest.mark.gpu
@pytest.mark.parametrize("abs_int", [False, True])
def test_python_node_fills_vector_clusters(mdx, sequence, tmp_path, abs_int):
    from motion_detection_amd.flow_clusterer import grid_vectors
    from motion_detection_amd.node import Image, MotionDetectionNode
    log = tmp_path / "motion.log"
    node = MotionDetectionNode({"pixel_step": PS, "egomotion": False, "distance_threshold": THR,
                                "angular_threshold": ATHR, "abs_int": abs_int, "log_contours": True,
                                "log_path": str(log)})
    plain = MotionDetectionNode({"pixel_step": PS, "egomotion": False, "distance_threshold": THR})
    expect, total_kept = "", 0
    for fi, f in enumerate(sequence):
        r = node.image_callback(Image.from_array(f, "rgb8"))
        q = plain.image_callback(Image.from_array(f, "rgb8"))
        if fi == 0:
            assert r is None and q is None
            continue
        assert q.vector_clusters == [] and q.clusters == [] and q.rectangles == []    # the stage is off
        assert np.array_equal(q.optical_flow_vectors, r.optical_flow_vectors)
        ref = vcluster_reference(grid_vectors(r.optical_flow_vectors, PS), THR, ATHR, abs_int=abs_int)
        assert ref["margin"] >= MARGIN, ref["margin"]
        assert np.array_equal(node.fc.last.labels, ref["labels"])
        assert (node.fc.last.num_active, node.fc.last.num_all) == (ref["num_active"], ref["num_all"])
        assert len(r.vector_clusters) == len(ref["members"]) == len(r.clusters) == len(r.rectangles)
        for g, c, m in zip(r.vector_clusters, r.clusters, ref["members"]):
            assert np.array_equal(g, m)
            assert c.dtype == np.float32 and np.array_equal(c, m[:, :2].astype(np.float32))
        assert np.array_equal(np.array(r.rectangles, np.int32).reshape(-1, 4), ref["rects"])
        assert r.frame_number == fi and r.outlier_points == []
        expect += log_lines(fi, ref["rects"])
        total_kept += len(r.rectangles)
    assert total_kept >= 1
    node.logger.close()
    assert log.read_text() == expect
