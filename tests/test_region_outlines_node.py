"""The mask regions' outer border polylines in both nodes (region_outlines): with region_min_area
set, every kept region comes with findContours' own point list; with region_external those of the external
regions only, exactly as region_contours combines with it.

The C++ node (host/mdx_node) writes region_outlines_<k>.bin next to regions_<k>.bin and region_hulls_<k>.bin and,
under log_contours, each outline to motion.log behind the frame's hull lines; the Python node fills
FlowResult.regions.outlines.  Both are compared with test_region_outlines.py's sequential tracer run on that
frame's own mask, the log with formats.py's writeContour rendering of it.  The sequence is
test_region_parents_node.py's: three regions in every second frame's mask, one of them nested.
"""
import numpy as np
import pytest

from node_io import dir_bytes, log_lines, node_exe, read_mask, read_regions, rgb8, run_node  # noqa: F401 (node_exe: a fixture)
from test_region_hulls import expected_hulls
from test_region_hulls_node import contour_lines, read_region_hulls
from test_region_outlines import outlines_of
from test_region_parents import NO_PARENT, parents_by_rule
from test_region_parents_node import MIN_AREA, PS, sequence  # noqa: F401 (sequence: a fixture)
from test_regions import regions_reference


def rendered(tmp_path, frame, outlines):
    """formats.py's writeContour lines of one frame's outlines."""
    from motion_detection_amd.formats import MotionLogger
    path = tmp_path / "render.log"
    lg = MotionLogger(str(path))
    for i, o in enumerate(outlines):
        lg.writeContour(np.array(o, np.int32).reshape(-1, 2), frame, i)
    lg.close()
    return path.read_text()


@pytest.mark.gpu
@pytest.mark.parametrize("external,contours", [(0, 0), (0, 1), (1, 1), (1, 0)])
def test_both_nodes_outline_files_and_motion_log(node_exe, tmp_path, mdx, sequence, external, contours):  # noqa: F811
    from motion_detection_amd.node import Image, MotionDetectionNode
    p, out = run_node(node_exe, tmp_path, rgb8(sequence), live_path=0, egomotion=0, pixel_step=PS, region_min_area=MIN_AREA,
                      log_contours=1, region_contours=contours, region_external=external, region_outlines=1)
    assert p.returncode == 0, p.stderr
    log = tmp_path / "py_motion.log"
    node = MotionDetectionNode({"pixel_step": PS, "egomotion": False, "live_chain": False, "region_min_area": MIN_AREA,
                                "log_contours": True, "log_path": str(log), "region_contours": bool(contours),
                                "region_external": bool(external), "region_outlines": True})
    nested, points, lines, k = 0, 0, [], 0
    for fi, f in enumerate(sequence):
        r = node.image_callback(Image.from_array(f, "rgb8"))
        if r is None:
            continue
        mask = read_mask(out / f"res_{k}.bin")
        assert np.array_equal(mask, r.mask)
        ref = regions_reference(mask, open3=True, min_area=MIN_AREA)
        par = parents_by_rule(ref["labels"], ref["kept"])
        idx = np.flatnonzero(par == NO_PARENT) if external else np.arange(len(ref["kept"]))
        num_all, regs = read_regions(out / f"regions_{k}.bin")                 # every kept record, as before
        assert num_all == ref["num_all"] and np.array_equal(regs, ref["kept"]) and np.array_equal(r.regions.regions, regs)
        assert type(r.regions) is (mdx.RegionTreeResult if external else mdx.RegionResult)
        want = outlines_of(ref["labels"], ref["kept"][idx])
        n, offsets, xy = read_region_hulls(out / f"region_outlines_{k}.bin")   # the hulls' layout
        assert n == len(idx) == len(r.regions.outlines)
        assert offsets.tolist() == np.cumsum([0] + [len(o) for o in want]).tolist()
        assert xy.tolist() == [list(v) for o in want for v in o]
        for got, exp in zip(r.regions.outlines, want):
            assert got.dtype == np.int32 and got.tolist() == [list(v) for v in exp]
        frame_lines = log_lines(fi, ref["kept"][idx, :4])
        if contours:
            frame_lines += contour_lines(fi, expected_hulls(ref["labels"], ref["kept"][idx]))
            assert len(r.regions.hulls) == len(idx)
        else:
            assert r.regions.hulls is None and not (out / f"region_hulls_{k}.bin").exists()
        lines.append(frame_lines + rendered(tmp_path, fi, want))               # behind the hull lines
        nested += int((par >= 0).sum())
        points += sum(len(o) for o in want)
        k += 1
    assert k == len(sequence) - 1 and nested >= 2 and points > 400
    node.logger.close()
    assert not (out / f"region_outlines_{k}.bin").exists()
    assert log.read_text() == "".join(lines)
    assert open(out / "motion.log", "rb").read() == log.read_bytes()


@pytest.mark.gpu
def test_parameter_off_changes_nothing(node_exe, tmp_path, mdx, sequence):  # noqa: F811
    """region_outlines=0, and a run that never mentions it: the same listing and the same bytes, no
    region_outlines_* file; the Python node's regions carry no outlines."""
    from motion_detection_amd.node import Image, MotionDetectionNode
    kw = dict(live_path=0, egomotion=0, pixel_step=PS, region_min_area=MIN_AREA, log_contours=1, region_contours=1,
              region_external=1)
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir()
    pa, a = run_node(node_exe, tmp_path / "a", rgb8(sequence), **kw)
    pb, b = run_node(node_exe, tmp_path / "b", rgb8(sequence), region_outlines=0, **kw)
    assert pa.returncode == 0 and pb.returncode == 0, pa.stderr + pb.stderr
    fa, fb = dir_bytes(a), dir_bytes(b)
    assert list(fa) == list(fb) and fa == fb
    assert "region_hulls_0.bin" in fa and not [n for n in fa if n.startswith("region_outlines_")]
    node = MotionDetectionNode({"pixel_step": PS, "egomotion": False, "live_chain": False, "region_min_area": MIN_AREA,
                                "region_contours": True})
    res = [node.image_callback(Image.from_array(f, "rgb8")) for f in sequence]
    assert res[0] is None and all(r.regions.outlines is None and r.regions.hulls is not None for r in res[1:])
    assert "region_outlines" in node.params and node.params["region_outlines"] is False
