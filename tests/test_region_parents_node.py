"""findContours' RETR_EXTERNAL in both nodes (region_external): with region_min_area set, every
kept region's parent blob comes with the records, and the rectangles and (region_contours) the hulls that are
logged and written cover the external regions only.

The C++ node (host/mdx_node) writes region_parents_<k>.bin next to regions_<k>.bin, region_hulls_<k>.bin and
motion.log; the Python node fills FlowResult.regions with a RegionTreeResult.  Both are compared with
test_region_parents.py's checkers run on that frame's own mask, and with each other.  The sequence (160 x 120) is
a smooth scene that shifts by (2, 1) pixels per frame, so that the fitted warp leaves nothing above the pair
path's threshold; every second frame has a white 6-pixel frame with a white block inside it and a white block
outside it painted in, which the mask then shows: three regions, one nested (chosen on the CPU with
oracle.calculate_optical_flow and the checkers).  The tests assert on the device's own masks that a nested kept
region exists.
"""
import struct

import numpy as np
import pytest

from node_io import dir_bytes, log_lines, node_exe, read_mask, read_regions, rgb8, run_node  # noqa: F401 (node_exe: a fixture)
from test_region_hulls import expected_hulls
from test_region_hulls_node import contour_lines, read_region_hulls
from test_region_parents import NO_PARENT, parents_by_enclosure, parents_by_rule
from test_regions import regions_reference

W, H, PS, MIN_AREA = 160, 120, 10, 50


def scene(dx, dy, painted):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    x, y = x - dx, y - dy
    f = (30 + 25 * np.sin(x / 6.0) * np.cos(y / 7.0) + 4 * np.sin((x + 2 * y) / 3.0)).round().astype(np.uint8)
    if painted:
        m = np.zeros((H, W), bool)
        m[30:100, 50:140] = True
        m[36:94, 56:134] = False
        m[55:75, 85:105] = True
        m[10:20, 10:30] = True
        f[m] = 255
    return np.repeat(f[:, :, None], 3, axis=2)


@pytest.fixture(scope="module")
def sequence():
    return [scene(0, 0, False), scene(2, 1, True), scene(4, 2, False), scene(6, 3, True)]


def read_region_parents(path):
    b = open(path, "rb").read()
    k = struct.unpack_from("<i", b, 0)[0]
    parent = np.frombuffer(b, np.int32, k, 4)
    ne = struct.unpack_from("<i", b, 4 + 4 * k)[0]
    assert len(b) == 8 + 4 * k + 4 * ne
    return parent, np.frombuffer(b, np.int32, ne, 8 + 4 * k)


@pytest.mark.gpu
@pytest.mark.parametrize("contours", [1, 0])
def test_both_nodes_parents_files_and_motion_log(node_exe, tmp_path, mdx, sequence, contours):
    from motion_detection_amd.node import Image, MotionDetectionNode
    p, out = run_node(node_exe, tmp_path, rgb8(sequence), live_path=0, egomotion=0, pixel_step=PS, region_min_area=MIN_AREA,
                      log_contours=1, region_contours=contours, region_external=1)
    assert p.returncode == 0, p.stderr
    log = tmp_path / "py_motion.log"
    node = MotionDetectionNode({"pixel_step": PS, "egomotion": False, "live_chain": False, "region_min_area": MIN_AREA,
                                "log_contours": True, "log_path": str(log), "region_contours": bool(contours),
                                "region_external": True})
    nested, lines, k = 0, [], 0
    for fi, f in enumerate(sequence):
        r = node.image_callback(Image.from_array(f, "rgb8"))
        if r is None:
            continue
        mask = read_mask(out / f"res_{k}.bin")
        assert np.array_equal(mask, r.mask)
        ref = regions_reference(mask, open3=True, min_area=MIN_AREA)
        every = regions_reference(mask, open3=True)["kept"]
        want = parents_by_rule(ref["labels"], ref["kept"])
        assert np.array_equal(want, parents_by_enclosure(ref["labels"], ref["kept"], every))
        idx = np.flatnonzero(want == NO_PARENT)
        num_all, regs = read_regions(out / f"regions_{k}.bin")                 # every kept record, as before
        assert num_all == ref["num_all"] == r.regions.num_all
        assert np.array_equal(regs, ref["kept"]) and np.array_equal(r.regions.regions, ref["kept"])
        parent, ext = read_region_parents(out / f"region_parents_{k}.bin")
        assert np.array_equal(parent, want) and np.array_equal(ext, idx)
        assert isinstance(r.regions, mdx.RegionTreeResult)
        assert np.array_equal(r.regions.parent, want) and np.array_equal(r.regions.external, idx)
        frame_lines = log_lines(fi, ref["kept"][idx, :4])                      # the external rectangles only
        if contours:
            hulls = expected_hulls(ref["labels"], ref["kept"][idx])
            n, offsets, xy = read_region_hulls(out / f"region_hulls_{k}.bin")
            assert n == len(idx) == len(r.regions.hulls)
            assert offsets.tolist() == np.cumsum([0] + [len(h) for h in hulls]).tolist()
            assert xy.tolist() == [list(v) for h in hulls for v in h]
            for got, exp in zip(r.regions.hulls, hulls):
                assert got.tolist() == [list(v) for v in exp]
            frame_lines += contour_lines(fi, hulls)
        else:
            assert r.regions.hulls is None and not (out / f"region_hulls_{k}.bin").exists()
        lines.append(frame_lines)
        nested += int((want >= 0).sum())
        k += 1
    assert k == len(sequence) - 1 and nested >= 2                # else nothing above tells external from kept
    node.logger.close()
    assert not (out / f"region_parents_{k}.bin").exists()
    assert log.read_text() == "".join(lines)
    assert open(out / "motion.log", "rb").read() == log.read_bytes()


@pytest.mark.gpu
def test_parameter_off_changes_nothing(node_exe, tmp_path, mdx, sequence):
    """region_external=0, and a run that never mentions it: the same listing and the same bytes, no
    region_parents_* file, every kept region logged; the Python node returns a plain RegionResult."""
    from motion_detection_amd.node import Image, MotionDetectionNode
    kw = dict(live_path=0, egomotion=0, pixel_step=PS, region_min_area=MIN_AREA, log_contours=1, region_contours=1)
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir()
    pa, a = run_node(node_exe, tmp_path / "a", rgb8(sequence), **kw)
    pb, b = run_node(node_exe, tmp_path / "b", rgb8(sequence), region_external=0, **kw)
    assert pa.returncode == 0 and pb.returncode == 0, pa.stderr + pb.stderr
    fa, fb = dir_bytes(a), dir_bytes(b)
    assert list(fa) == list(fb) and fa == fb
    assert "regions_0.bin" in fa and not [n for n in fa if n.startswith("region_parents_")]
    lines = []
    for k in range(len(sequence) - 1):
        ref = regions_reference(read_mask(a / f"res_{k}.bin"), open3=True, min_area=MIN_AREA)
        lines.append(log_lines(k + 1, ref["kept"][:, :4]) + contour_lines(k + 1, expected_hulls(ref["labels"], ref["kept"])))
    assert fa["motion.log"].decode() == "".join(lines) != ""     # nested regions included, as before
    node = MotionDetectionNode({"pixel_step": PS, "egomotion": False, "live_chain": False, "region_min_area": MIN_AREA,
                                "region_contours": True})
    res = [node.image_callback(Image.from_array(f, "rgb8")) for f in sequence]
    assert res[0] is None and all(type(r.regions) is mdx.RegionResult for r in res[1:])
    assert sum(len(r.regions.hulls) for r in res[1:]) == sum(r.regions.num_kept for r in res[1:]) >= 3
