"""The pair path's detector in both nodes: MotionDetectionNode::detectOutliers
(ros/src/motion_detection_node.cpp:112-160) -- findOutliers, getOutlierVectors, getClusters on the
pair's Vec4d image -- each kept cluster's rectangle and MotionLogger::writeBoundingBox.

The C++ node (host/mdx_node) writes outliers_<k>.bin and motion.log; the Python node fills
FlowResult.outlier_flags / vector_clusters / clusters / rectangles.  Both are compared with the
literal-loop checker of test_outliers.py chained with test_vcluster.vcluster_reference, run on the
vector image the node itself reports, on tests/golden/synth_160x120_rgb played back and forth.  The
two settings were chosen on the CPU (oracle.calculate_optical_flow + the checkers) so that every
processed pair has outliers and a kept cluster and no angular value within 1e-9 of the threshold:
a dense grid where every vector moves, and a coarser one where min_vector_size zeroes two thirds of
the vectors, which include_zeros then pulls into the statistics (MAD 0: every moving vector is an
outlier).  The tests assert all of that on what the device reports.
"""
import os

import numpy as np
import pytest

from node_io import (ROOT, dir_bytes, log_lines, node_exe, read_outliers, read_regions, rgb8,  # noqa: F401 (node_exe: a fixture)
                     run_node)
from test_outliers import STAT_DOUBLES, STAT_INTS, bits, outliers_reference
from test_vcluster import MARGIN, vcluster_reference

W, H = 160, 120
# pixel_step, min_vector_size, distance_threshold, angular_threshold, include_zeros
SETTINGS = [(4, 1.0, 8.0, 0.5, 0), (5, 3.5, 12.0, 1.0, 0), (5, 3.5, 12.0, 1.0, 1)]


@pytest.fixture(scope="module")
def sequence():
    g = np.load(os.path.join(ROOT, "tests", "golden", "synth_160x120_rgb.npz"))
    return [g["img1"], g["img2"], g["img1"], g["img2"]]


def chain_reference(vec, include_zeros, thr, athr):
    ref = outliers_reference(vec, bool(include_zeros))
    cl = vcluster_reference(ref["outlier_vectors"], thr, athr)
    assert cl["margin"] >= MARGIN, cl["margin"]
    return ref, cl


def same_stats(got, ref):
    for k in STAT_INTS:
        assert int(got[k]) == ref["stats"][k], k
    for k in STAT_DOUBLES:
        if k.startswith("median_") and ref["stats"][k] == 0.0:
            assert float(got[k]) == 0.0, k                          # a zero median: a value, not a sign
        else:
            assert bits(float(got[k])) == bits(ref["stats"][k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("ps,mvs,thr,athr,iz", SETTINGS)
def test_cpp_node_outliers_clusters_and_motion_log(node_exe, tmp_path, sequence, ps, mvs, thr, athr, iz):
    p, out = run_node(node_exe, tmp_path, rgb8(sequence), live_path=0, egomotion=0, pixel_step=ps, min_vector_size=mvs,
                      distance_threshold=thr, angular_threshold=athr, detect_outliers=1, include_zeros=iz, log_contours=1)
    assert p.returncode == 0, p.stderr
    nproc = len(sequence) - 1                          # a ring of 2 frames
    assert f"processed {nproc} of {len(sequence)}" in p.stdout
    expect = ""
    for k in range(nproc):
        vec, stats, flags, nact, num_all, labels, kept, rects = read_outliers(out / f"outliers_{k}.bin")
        assert len(vec) == (W // ps) * (H // ps)
        ref, cl = chain_reference(vec, iz, thr, athr)
        same_stats(stats, ref)
        assert np.array_equal(flags, ref["flags"])
        assert 0 < ref["stats"]["outliers"] < len(vec) and len(cl["kept"]) >= 1     # else the comparison is vacuous
        assert ref["stats"]["selected"] == (len(vec) if iz else np.count_nonzero(vec[:, 2:].any(axis=1)))
        assert (nact, num_all) == (cl["num_active"], cl["num_all"])
        assert np.array_equal(labels, cl["labels"])
        assert np.array_equal(kept, cl["kept"]) and np.array_equal(rects, cl["rects"])
        assert np.all(labels[flags == 0] == -1)        # only outlier vectors are clustered
        expect += log_lines(1 + k, cl["rects"])        # skip_frames 1: global_frame_count_ = the frame's index
    assert (out / "motion.log").read_text() == expect
    assert not [n for n in os.listdir(out) if n.startswith("vclusters_") or n.startswith("clusters_")]


@pytest.mark.gpu
@pytest.mark.parametrize("params", [dict(), dict(live_path=0, egomotion=0, distance_threshold=8.0, angular_threshold=0.5,
                                                 region_min_area=4, log_contours=1)])
def test_cpp_node_defaults_are_unchanged(node_exe, tmp_path, sequence, params):
    """Without detect_outliers the node writes what it wrote before: the same files, byte for byte, as
    with the detector switched off explicitly; include_zeros alone does nothing."""
    seq = rgb8(sequence + [sequence[0]])               # five frames: the default live ring fills once
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir(), (tmp_path / "c").mkdir()
    pa, a = run_node(node_exe, tmp_path / "a", seq, **params)
    pb, b = run_node(node_exe, tmp_path / "b", seq, detect_outliers=0, include_zeros=0, **params)
    pc, c = run_node(node_exe, tmp_path / "c", seq, include_zeros=1, **params)
    assert pa.returncode == 0 and pb.returncode == 0 and pc.returncode == 0, pa.stderr + pb.stderr + pc.stderr
    fa = dir_bytes(a)
    assert "res_0.bin" in fa and not [n for n in fa if n.startswith("outliers_")]
    assert fa == dir_bytes(b) == dir_bytes(c)
    assert pa.stdout == pb.stdout == pc.stdout


@pytest.mark.gpu
def test_cpp_node_needs_both_thresholds(node_exe, tmp_path, sequence):
    p, out = run_node(node_exe, tmp_path, rgb8(sequence), live_path=0, egomotion=0, distance_threshold=8.0, detect_outliers=1)
    assert p.returncode == 0, p.stderr
    assert "res_0.bin" in os.listdir(out) and not [n for n in os.listdir(out) if n.startswith("outliers_")]


@pytest.mark.gpu
@pytest.mark.parametrize("ps,mvs,thr,athr,iz", SETTINGS)
def test_python_node_fills_outliers_and_clusters(mdx, sequence, tmp_path, ps, mvs, thr, athr, iz):
    from motion_detection_amd.flow_clusterer import grid_vectors
    from motion_detection_amd.node import Image, MotionDetectionNode
    log = tmp_path / "motion.log"
    base = {"pixel_step": ps, "min_vector_size": mvs, "egomotion": False, "live_chain": False,
            "distance_threshold": thr, "angular_threshold": athr}
    node = MotionDetectionNode(dict(base, detect_outliers=True, include_zeros=bool(iz), log_contours=True, log_path=str(log)))
    plain = MotionDetectionNode(base)
    off = MotionDetectionNode(dict(base, detect_outliers=False, include_zeros=True))
    expect = ""
    for fi, f in enumerate(sequence):
        r = node.image_callback(Image.from_array(f, "rgb8"))
        q = plain.image_callback(Image.from_array(f, "rgb8"))
        o = off.image_callback(Image.from_array(f, "rgb8"))
        if fi == 0:
            assert r is None and q is None and o is None
            continue
        for d in (q, o):                               # the stage is off: the result is what it was
            assert d.outlier_flags is None and d.vector_clusters == [] and d.clusters == [] and d.rectangles == []
            assert np.array_equal(bits(d.vectors), bits(r.vectors)) and np.array_equal(d.mask, r.mask)
            assert np.array_equal(d.next_pts.view(np.uint32), r.next_pts.view(np.uint32)) and np.array_equal(d.H, r.H)
            assert d.num_vectors == r.num_vectors and d.regions is None
        img = np.zeros((H, W, 4))
        ny = H // ps
        for k, v in enumerate(r.vectors):               # the x-major grid of the flow entry
            img[(k % ny) * ps, (k // ny) * ps] = v
        ref, cl = chain_reference(grid_vectors(img, ps), iz, thr, athr)
        assert 0 < ref["stats"]["outliers"] < len(ref["flags"]) and len(cl["kept"]) >= 1
        assert r.outlier_flags.dtype == np.uint8 and np.array_equal(r.outlier_flags, ref["flags"])
        assert len(r.vector_clusters) == len(cl["members"]) == len(r.clusters) == len(r.rectangles)
        for g, c, m in zip(r.vector_clusters, r.clusters, cl["members"]):
            assert np.array_equal(g, m)
            assert c.dtype == np.float32 and np.array_equal(c, m[:, :2].astype(np.float32))
        assert np.array_equal(np.array(r.rectangles, np.int32).reshape(-1, 4), cl["rects"])
        expect += log_lines(fi, cl["rects"])
    node.logger.close()
    assert log.read_text() == expect
    assert plain.logger is None and off.logger is None


# every optional stage of the pair path at once: the regions and the detector, both logging.  The
# coarser setting: its fit leaves a motion mask with regions (checked on the CPU with the oracle and
# test_regions.regions_reference: 4 and 6 opened regions of 4 pixels and more); the dense one's mask is empty
ALL_PS, ALL_MVS, ALL_THR, ALL_ATHR, ALL_IZ = SETTINGS[1]
ALL_MIN_AREA = 4


@pytest.mark.gpu
def test_cpp_node_all_pair_stages_at_once(node_exe, tmp_path, sequence):
    """Each stage writes the file it writes when it runs alone, and motion.log holds, per frame, the
    regions' lines followed by the outlier clusters' lines."""
    base = dict(live_path=0, egomotion=0, pixel_step=ALL_PS, min_vector_size=ALL_MVS, log_contours=1)
    detector = dict(distance_threshold=ALL_THR, angular_threshold=ALL_ATHR, detect_outliers=1, include_zeros=ALL_IZ)
    for d in ("all", "regions", "detector"):
        (tmp_path / d).mkdir()
    pa, both = run_node(node_exe, tmp_path / "all", rgb8(sequence), region_min_area=ALL_MIN_AREA, **base, **detector)
    pr, regs = run_node(node_exe, tmp_path / "regions", rgb8(sequence), region_min_area=ALL_MIN_AREA, **base)
    pd, dets = run_node(node_exe, tmp_path / "detector", rgb8(sequence), **base, **detector)
    assert pa.returncode == 0 and pr.returncode == 0 and pd.returncode == 0, pa.stderr + pr.stderr + pd.stderr
    nproc = len(sequence) - 1                          # a ring of 2 frames
    assert f"processed {nproc} of {len(sequence)}" in pa.stdout
    fa, fr, fd = dir_bytes(both), dir_bytes(regs), dir_bytes(dets)
    expect = ""
    for k in range(nproc):
        assert fa[f"regions_{k}.bin"] == fr[f"regions_{k}.bin"]
        assert fa[f"outliers_{k}.bin"] == fd[f"outliers_{k}.bin"]
        _, records = read_regions(both / f"regions_{k}.bin")
        rects = read_outliers(both / f"outliers_{k}.bin")[-1]
        assert len(records) >= 1 and len(rects) >= 1   # else the order below is not checked
        expect += log_lines(1 + k, records[:, :4]) + log_lines(1 + k, rects)   # global_frame_count_ = the frame's index
    assert f"regions_{nproc}.bin" not in fa and f"outliers_{nproc}.bin" not in fa
    assert fa["motion.log"].decode() == expect


@pytest.mark.gpu
def test_python_node_all_pair_stages_at_once(mdx, sequence, tmp_path):
    """The same three nodes in Python: FlowResult.regions, outlier_flags and rectangles equal the
    single-stage nodes', and the log holds the regions' lines, then the clusters', per frame."""
    from motion_detection_amd.node import Image, MotionDetectionNode
    base = {"pixel_step": ALL_PS, "min_vector_size": ALL_MVS, "egomotion": False, "live_chain": False,
            "log_contours": True}
    detector = {"distance_threshold": ALL_THR, "angular_threshold": ALL_ATHR, "detect_outliers": True,
                "include_zeros": bool(ALL_IZ)}
    log = tmp_path / "all.log"
    both = MotionDetectionNode(dict(base, region_min_area=ALL_MIN_AREA, log_path=str(log), **detector))
    regs = MotionDetectionNode(dict(base, region_min_area=ALL_MIN_AREA, log_path=str(tmp_path / "regions.log")))
    dets = MotionDetectionNode(dict(base, log_path=str(tmp_path / "detector.log"), **detector))
    expect = ""
    for fi, f in enumerate(sequence):
        r, g, d = (n.image_callback(Image.from_array(f, "rgb8")) for n in (both, regs, dets))
        if fi == 0:
            assert r is None and g is None and d is None
            continue
        assert np.array_equal(r.regions.regions, g.regions.regions)
        assert (r.regions.num_all, r.regions.num_kept) == (g.regions.num_all, g.regions.num_kept)
        assert r.outlier_flags.dtype == np.uint8 and np.array_equal(r.outlier_flags, d.outlier_flags)
        assert r.rectangles == d.rectangles
        assert len(r.regions.rectangles) >= 1 and len(r.rectangles) >= 1   # else the order below is not checked
        expect += log_lines(fi, r.regions.rectangles) + log_lines(fi, r.rectangles)
    for n in (both, regs, dets):
        n.logger.close()
    assert log.read_text() == expect
