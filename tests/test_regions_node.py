"""The pair path's regions in both nodes: region_min_area labels the motion mask on the device
(mdx_mask_regions) and log_contours logs each kept region's rectangle through
MotionLogger::writeBoundingBox (reference common/src/motion_logger.cpp:43-47).

The C++ node (host/mdx_node) writes regions_<k>.bin and motion.log; the Python node fills
FlowResult.regions.  Both are compared with test_regions.py's flood-fill checker run on that frame's
own mask, and with each other.  The sequence (160 x 120, the pair path's own threshold) was chosen on
the CPU (oracle.calculate_optical_flow + the checker) so that opened regions of 50 pixels and more
exist; the tests assert that at least one is kept.
"""
import os

import numpy as np
import pytest

from node_io import log_lines, node_exe, read_mask, read_regions, rgb8, run_node  # noqa: F401 (node_exe: a fixture)
from test_regions import regions_reference

W, H, PS, MIN_AREA = 160, 120, 10, 50


@pytest.fixture(scope="module")
def sequence(mdx):
    a, b, _ = mdx.synth_pair(20141105, W, H, 1)
    c, d, _ = mdx.synth_pair(11, W, H, 1)
    return [np.repeat(f[:, :, None], 3, axis=2) for f in (a, b, c, d)]   # gray scenes as rgb8 frames


@pytest.mark.gpu
@pytest.mark.parametrize("region_open", [1, 0])
def test_both_nodes_regions_and_motion_log(node_exe, tmp_path, mdx, sequence, region_open):
    from motion_detection_amd.node import Image, MotionDetectionNode
    p, out = run_node(node_exe, tmp_path, rgb8(sequence), live_path=0, egomotion=0, pixel_step=PS, region_min_area=MIN_AREA,
                      region_open=region_open, log_contours=1)
    assert p.returncode == 0, p.stderr
    nproc = len(sequence) - 1
    assert f"processed {nproc} of {len(sequence)}" in p.stdout
    log = tmp_path / "py_motion.log"
    node = MotionDetectionNode({"pixel_step": PS, "egomotion": False, "live_chain": False, "region_min_area": MIN_AREA,
                                "region_open": bool(region_open), "log_contours": True, "log_path": str(log)})
    total_kept, lines, k = 0, [], 0
    for fi, f in enumerate(sequence):
        r = node.image_callback(Image.from_array(f, "rgb8"))
        if r is None:
            continue
        mask = read_mask(out / f"res_{k}.bin")
        assert np.array_equal(mask, r.mask)
        ref = regions_reference(mask, open3=bool(region_open), min_area=MIN_AREA)
        num_all, regs = read_regions(out / f"regions_{k}.bin")
        assert num_all == ref["num_all"] == r.regions.num_all
        assert np.array_equal(regs, ref["kept"]) and np.array_equal(r.regions.regions, ref["kept"])
        assert r.regions.num_kept == len(ref["kept"])
        lines.append(log_lines(fi, ref["kept"][:, :4]))
        total_kept += len(regs)
        k += 1
    assert k == nproc and total_kept >= 1                    # else the comparison above is vacuous
    node.logger.close()
    assert not (out / f"regions_{nproc}.bin").exists()
    assert log.read_text() == "".join(lines)
    assert open(out / "motion.log", "rb").read() == log.read_bytes()


@pytest.mark.gpu
def test_knob_off_writes_no_region_files(node_exe, tmp_path, mdx, sequence):
    from motion_detection_amd.node import Image, MotionDetectionNode
    p, out = run_node(node_exe, tmp_path, rgb8(sequence), live_path=0, egomotion=0, pixel_step=PS)
    assert p.returncode == 0, p.stderr
    names = os.listdir(out)
    assert "res_0.bin" in names
    assert "motion.log" not in names and not [n for n in names if n.startswith("regions_")]
    node = MotionDetectionNode({"pixel_step": PS, "egomotion": False, "live_chain": False})
    res = [node.image_callback(Image.from_array(f, "rgb8")) for f in sequence]
    assert res[0] is None and all(r.regions is None for r in res[1:])


def test_flow_result_positional_construction_is_unchanged(mdx):
    z = np.zeros(1)
    r = mdx.FlowResult(3, z, z, z, None, z, 0)
    assert r.regions is None and r.code == 0
