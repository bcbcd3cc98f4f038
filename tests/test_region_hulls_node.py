"""The mask regions' convex hulls in both nodes (region_contours): with region_min_area set
the pair path's regions come with their hulls (mdx_mask_region_hulls), and under log_contours each hull is
logged with MotionLogger::writeContour behind that frame's region rectangles.

The C++ node (host/mdx_node) writes region_hulls_<k>.bin and motion.log; the Python node fills
FlowResult.regions.hulls.  Both are compared with the checker of test_region_hulls.py (test_regions'
flood fill, then test_hulls' monotone chain per label) run on that frame's own mask, and with each other.
The sequence is test_regions_node.py's (160 x 120, chosen there so that opened regions of 50 pixels and
more exist).  With the parameter off nothing may change: the files are compared byte for byte with a run
that does not know the parameter.
"""
import os
import struct

import numpy as np
import pytest

from node_io import dir_bytes, log_lines, node_exe, read_mask, read_regions, rgb8, run_node  # noqa: F401 (node_exe: a fixture)
from test_region_hulls import expected_hulls
from test_regions import regions_reference
from test_regions_node import MIN_AREA, PS, sequence  # noqa: F401 (sequence: a fixture)


def read_region_hulls(path):
    b = open(path, "rb").read()
    k = struct.unpack_from("<i", b, 0)[0]
    offsets = np.frombuffer(b, np.int32, k + 1, 4)
    assert len(b) == 4 + 4 * (k + 1) + 8 * offsets[k]
    xy = np.frombuffer(b, np.int32, 2 * offsets[k], 4 + 4 * (k + 1)).reshape(-1, 2)
    return k, offsets, xy


def contour_lines(frame, hulls):
    """MotionLogger::writeContour's lines of one frame's hulls."""
    return "".join(f"{frame}, {i}" + "".join(f", {x}, {y}" for x, y in h) + "\n" for i, h in enumerate(hulls))


@pytest.mark.gpu
@pytest.mark.parametrize("region_open", [1, 0])
def test_both_nodes_region_hulls_and_motion_log(node_exe, tmp_path, mdx, sequence, region_open):
    from motion_detection_amd.node import Image, MotionDetectionNode
    p, out = run_node(node_exe, tmp_path, rgb8(sequence), live_path=0, egomotion=0, pixel_step=PS, region_min_area=MIN_AREA,
                      region_open=region_open, log_contours=1, region_contours=1)
    assert p.returncode == 0, p.stderr
    log = tmp_path / "py_motion.log"
    node = MotionDetectionNode({"pixel_step": PS, "egomotion": False, "live_chain": False, "region_min_area": MIN_AREA,
                                "region_open": bool(region_open), "log_contours": True, "log_path": str(log),
                                "region_contours": True})
    total_vertices, lines, k = 0, [], 0
    for fi, f in enumerate(sequence):
        r = node.image_callback(Image.from_array(f, "rgb8"))
        if r is None:
            continue
        mask = read_mask(out / f"res_{k}.bin")
        assert np.array_equal(mask, r.mask)
        ref = regions_reference(mask, open3=bool(region_open), min_area=MIN_AREA)
        hulls = expected_hulls(ref["labels"], ref["kept"])
        num_all, regs = read_regions(out / f"regions_{k}.bin")
        assert num_all == ref["num_all"] == r.regions.num_all
        assert np.array_equal(regs, ref["kept"]) and np.array_equal(r.regions.regions, ref["kept"])
        n, offsets, xy = read_region_hulls(out / f"region_hulls_{k}.bin")
        assert n == len(hulls) == len(r.regions.hulls)
        assert offsets.tolist() == np.cumsum([0] + [len(h) for h in hulls]).tolist()
        assert xy.tolist() == [list(v) for h in hulls for v in h]
        for got, want in zip(r.regions.hulls, hulls):
            assert got.dtype == np.int32 and got.tolist() == [list(v) for v in want]
        lines.append(log_lines(fi, ref["kept"][:, :4]) + contour_lines(fi, hulls))   # rectangles, then contours
        total_vertices += len(xy)
        k += 1
    assert k == len(sequence) - 1 and total_vertices >= 3        # else the comparison above is vacuous
    node.logger.close()
    assert not (out / f"region_hulls_{k}.bin").exists()
    assert log.read_text() == "".join(lines)
    assert open(out / "motion.log", "rb").read() == log.read_bytes()


@pytest.mark.gpu
def test_parameter_off_changes_nothing(node_exe, tmp_path, mdx, sequence):
    """region_contours=0, and a run that never mentions it: the same listing and the same bytes, no
    region_hulls_* file, motion.log the rectangles alone; the Python node leaves hulls None."""
    from motion_detection_amd.node import Image, MotionDetectionNode
    kw = dict(live_path=0, egomotion=0, pixel_step=PS, region_min_area=MIN_AREA, log_contours=1)
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir()
    pa, a = run_node(node_exe, tmp_path / "a", rgb8(sequence), **kw)
    pb, b = run_node(node_exe, tmp_path / "b", rgb8(sequence), region_contours=0, **kw)
    assert pa.returncode == 0 and pb.returncode == 0, pa.stderr + pb.stderr
    fa, fb = dir_bytes(a), dir_bytes(b)
    assert list(fa) == list(fb) and fa == fb
    assert "regions_0.bin" in fa and not [n for n in fa if n.startswith("region_hulls_")]
    lines = []
    for k in range(len(sequence) - 1):
        ref = regions_reference(read_mask(a / f"res_{k}.bin"), open3=True, min_area=MIN_AREA)
        lines.append(log_lines(k + 1, ref["kept"][:, :4]))
    assert fa["motion.log"].decode() == "".join(lines) != ""     # what the parent commit logs: rectangles only
    log = tmp_path / "py_motion.log"
    node = MotionDetectionNode({"pixel_step": PS, "egomotion": False, "live_chain": False, "region_min_area": MIN_AREA,
                                "log_contours": True, "log_path": str(log)})
    res = [node.image_callback(Image.from_array(f, "rgb8")) for f in sequence]
    assert res[0] is None and all(r.regions is not None and r.regions.hulls is None for r in res[1:])
    node.logger.close()
    assert log.read_bytes() == fa["motion.log"]
