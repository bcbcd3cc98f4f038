"""Background subtraction in both nodes (background_subtraction): every frame that enters the ring
also updates a MOG2 model on the device; with region_min_area set, the external regions of the model's opened mask
go to motion_bg.log, one MotionLogger::writeBoundingBox line each.

Expected: tests/bg_check.cpp's mask of the same frames (test_bg.py's oracle), labelled by test_regions.py's CPU
reference, filtered by test_region_parents.py's rule, rendered by formats.py.  With the parameter off, or never
mentioned, nothing new is written and every other file keeps its bytes.
"""
import numpy as np
import pytest

from node_io import dir_bytes, node_exe, rgb8, run_node  # noqa: F401 (node_exe: a fixture)
from test_bg import cpp_run, needs_gxx, params_of, square_stream
from test_region_parents import NO_PARENT, parents_by_rule
from test_regions import regions_reference

MIN_AREA, PS = 6, 10


def expected_log(tmp_path, frames):
    """formats.py's rendering of the oracle's external regions, frame by frame."""
    from motion_detection_amd.formats import MotionLogger
    masks = cpp_run(frames, params_of())["masks"]
    path = tmp_path / "render.log"
    lg = MotionLogger(str(path))
    total = 0
    for fi, mask in enumerate(masks):
        ref = regions_reference(mask, open3=True, min_area=MIN_AREA)
        par = parents_by_rule(ref["labels"], ref["kept"])
        ext = ref["kept"][np.flatnonzero(par == NO_PARENT)]
        for i, r in enumerate(ext):
            lg.writeBoundingBox(tuple(int(v) for v in r[:4]), fi, i)
        total += len(ext)
    lg.close()
    return path.read_text(), total


@pytest.mark.gpu
@needs_gxx
@pytest.mark.parametrize("live", [0, 1])
def test_both_nodes_write_motion_bg_log(node_exe, tmp_path, mdx, live):  # noqa: F811
    from motion_detection_amd.node import Image, MotionDetectionNode
    frames = square_stream()
    want, total = expected_log(tmp_path, frames)
    assert total >= 2 * (len(frames) - 1)                # both squares, from the second frame on
    p, out = run_node(node_exe, tmp_path, rgb8(frames), live_path=live, egomotion=0, pixel_step=PS, region_min_area=MIN_AREA,
                      background_subtraction=1)
    assert p.returncode == 0, p.stderr
    assert (out / "motion_bg.log").read_text() == want
    log = tmp_path / "py" / "motion.log"
    log.parent.mkdir()
    node = MotionDetectionNode({"pixel_step": PS, "egomotion": False, "live_chain": bool(live), "region_min_area": MIN_AREA,
                                "log_path": str(log), "background_subtraction": True})
    for f in frames:
        node.image_callback(Image.from_array(f, "rgb8"))
    node.bg_logger.close()
    assert (log.parent / "motion_bg.log").read_text() == want
    assert not log.exists()                              # log_contours is off: no motion.log
    node.bs.close()


@pytest.mark.gpu
def test_parameter_off_changes_nothing(node_exe, tmp_path, mdx):  # noqa: F811
    """background_subtraction=0, a run that never mentions it, and a run with it on: the same files with the same
    bytes, plus motion_bg.log only in the last; the Python node builds no model unless asked."""
    from motion_detection_amd.node import Image, MotionDetectionNode
    frames = square_stream(T=4)
    kw = dict(live_path=0, egomotion=0, pixel_step=PS, region_min_area=MIN_AREA, log_contours=1)
    dirs = []
    for name, extra in (("a", {}), ("b", dict(background_subtraction=0)), ("c", dict(background_subtraction=1))):
        (tmp_path / name).mkdir()
        p, out = run_node(node_exe, tmp_path / name, rgb8(frames), **kw, **extra)
        assert p.returncode == 0, p.stderr
        dirs.append(dir_bytes(out))
    a, b, c = dirs
    assert list(a) == list(b) and a == b and "motion_bg.log" not in a
    assert "motion_bg.log" in c and {k: v for k, v in c.items() if k != "motion_bg.log"} == a
    node = MotionDetectionNode({"pixel_step": PS, "egomotion": False, "live_chain": False, "region_min_area": MIN_AREA})
    for f in frames:
        node.image_callback(Image.from_array(f, "rgb8"))
    assert node.params["background_subtraction"] is False and node.bs is None and node.bg_logger is None
