"""The node's polling caller run() (reference ros/src/motion_detection_node.cpp:457-553; body :464-529),
for use_all_frames = false: every ring frame wider than 320 px halved (cv::resize(.., 0.5, 0.5), :470-474),
the trajectories, fitSubspace(trajectories, outlier_points, 2, residual_threshold) (:494) and
clusterEuclidean(outlier_points, distance_threshold) (:497).

CPU: MotionDetectionNode.run_once() over recording stand-ins, in the style of tests/test_node.py.
GPU: the Python node and host/mdx_node use_all_frames=0 against the oracle on frames halved by
tests/test_resize_half.py's numpy checker, and the rest of the chain against OutlierDetector /
FlowClusterer on those trajectories with the same seed; a default mdx_node run is byte-identical with and
without the new parameters spelled out at their defaults.
"""
import numpy as np
import pytest

from motion_detection_amd.node import Image, MotionDetectionNode
from node_io import dir_bytes, node_exe, read_clusters, read_res, rgb8, run_node  # noqa: F401 (node_exe: a fixture)
from test_resize_half import half_ref, half_size_ref


class RecordingRing:
    """Stand-in for the calculator's ring entries and the detector (GPU work is tested below)."""

    def __init__(self, ntraj=3):
        self.pushes, self.traj_calls, self.fit_calls, self.resets, self.held, self.ntraj = [], [], [], 0, 0, ntraj

    def ring_reset(self):
        self.resets += 1
        self.held = 0

    def ring_push(self, image, keep, half, pixel_step, min_vector_size):
        self.pushes.append((int(image[0, 0, 0]), image.shape, keep, half))
        self.held = min(self.held + 1, keep)
        return self.held, self

    def ring_trajectory(self, w, h, nimg, vec, trajectories, pixel_step, mvs):
        self.traj_calls.append((w, h, nimg, vec.shape, pixel_step, mvs))
        trajectories.extend([np.zeros((nimg, 2), np.float32)] * self.ntraj)
        return 7

    def fitSubspace(self, trajectories, outlier_points, num_motions, sigma):
        self.fit_calls.append((len(trajectories), num_motions, sigma))
        outlier_points.append((1.0, 2.0))
        return trajectories[:1]


def frame(v, w=8, h=6):
    return Image.from_array(np.full((h, w), v, np.uint8), "mono8")


def make_node(ntraj=3, **params):
    params.setdefault("use_all_frames", False)
    n = MotionDetectionNode(params)        # no device work at construction
    n.ofc = n.od = RecordingRing(ntraj)
    return n


def test_run_once_waits_for_the_ring():
    n = make_node()
    assert n.params["residual_threshold"] == 0.2                # node.cpp:491
    for v in range(4):
        assert n.image_callback(frame(v)) is None
        assert n.run_once() is None                             # :459: not before image_received
    assert n.image_callback(frame(4)) is None                   # the callback itself still does no work
    assert not n.ofc.pushes
    res = n.run_once()
    assert res is not None and res.num_vectors == 7 and n.frames_processed == 1
    assert [p[0] for p in n.ofc.pushes] == [0, 1, 2, 3, 4]
    assert all(p[1:] == ((6, 8, 3), 5, False) for p in n.ofc.pushes)   # toCvCopy "rgb8" (:469), keep = the ring
    assert n.ofc.traj_calls == [(8, 6, 5, (6, 8, 4), 10, 1.0)]
    assert res.optical_flow_vectors.shape == (6, 8, 4)
    assert res.outlier_points == [(1.0, 2.0)] and len(res.subspace) == 1
    assert res.clusters == [] and res.rectangles == []          # no distance_threshold: that stage is off


def test_fit_subspace_takes_two_motions_and_the_residual_threshold():
    """fitSubspace(trajectories, outlier_points, 2, residual_threshold) (:494), whatever num_motions says;
    num_motions still sizes the ring (2 * 3 + 1 frames)."""
    n = make_node(num_motions=3, residual_threshold=0.35, sigma=0.9)
    seen = []
    n.on_result = seen.append
    for v in range(7):
        assert n.run_once() is None
        n.image_callback(frame(v))
    res = n.run_once()
    assert n.ofc.fit_calls == [(3, 2, 0.35)]
    assert n.ofc.traj_calls[0][2] == 7 and len(n.ofc.pushes) == 7
    assert seen == [res]


def test_frames_wider_than_320_are_halved():
    for w, h, half in [(320, 240, False), (322, 240, True), (321, 9, True), (640, 480, True)]:
        n = make_node(egomotion=False)                          # a ring of 2
        n.image_callback(frame(1, w, h))
        n.image_callback(frame(2, w, h))
        res = n.run_once()
        assert [p[3] for p in n.ofc.pushes] == [half, half], w  # cols > 320, strictly (:470)
        assert all(p[1] == (h, w, 3) for p in n.ofc.pushes)     # the full frame goes down; the device halves it
        dw, dh = half_size_ref(w, h) if half else (w, h)
        assert n.ofc.traj_calls == [(dw, dh, 2, (dh, dw, 4), 10, 1.0)]
        assert res.optical_flow_vectors.shape == (dh, dw, 4)    # the Vec4d image has the halved size


def test_no_complete_trajectory_means_no_fit():
    n = make_node(ntraj=0, distance_threshold=50.0)
    for v in range(5):
        n.image_callback(frame(v))
    res = n.run_once()
    assert n.ofc.fit_calls == [] and n.fc is None               # neither the fit nor the clustering ran
    assert res.trajectories == [] and res.outlier_points == [] and res.subspace == []
    assert res.clusters == [] and res.rectangles == []
    assert n.frames_processed == 1


def test_a_message_is_pushed_once():
    n = make_node()
    for v in range(5):
        n.image_callback(frame(v))
    n.run_once()
    n.run_once()                                                # no new frame: the same ring, nothing uploaded
    assert [p[0] for p in n.ofc.pushes] == [0, 1, 2, 3, 4]
    assert len(n.ofc.fit_calls) == 2                            # but the fit ran again (a further-advanced rand())
    n.image_callback(frame(5))
    n.image_callback(frame(6))
    n.run_once()
    assert [p[0] for p in n.ofc.pushes] == [0, 1, 2, 3, 4, 5, 6]
    for v in range(7, 13):                                      # the whole ring replaced between two runs
        n.image_callback(frame(v))
    n.run_once()
    assert [p[0] for p in n.ofc.pushes][7:] == [8, 9, 10, 11, 12] and n.ofc.resets == 1
    assert n.run(max_runs=2)[1].num_vectors == 7 and len(n.ofc.pushes) == 12


def test_run_loops_over_run_once():
    n = make_node(egomotion=False)                              # a ring of 2
    assert n.run(max_runs=3) == []                              # no full ring and nothing to deliver frames
    with pytest.raises(ValueError):
        n.run()                                                 # the reference's loop never ends
    pending = [frame(v) for v in range(4)]

    def spin_once():                                            # ros::spinOnce: one pending frame per pass
        if not pending:
            return False
        n.image_callback(pending.pop(0))

    res = n.run(spin_once=spin_once)
    assert len(res) == 3 and n.frames_processed == 3            # the passes after frames 1, 2 and 3
    assert [p[0] for p in n.ofc.pushes] == [0, 1, 2, 3]


def test_use_all_frames_true_leaves_run_once_to_the_caller():
    """Defaults unchanged: with use_all_frames the callback runs the live branch itself."""
    n = MotionDetectionNode()
    assert n.params["use_all_frames"] is True and n.trajectory_size == 5


# ---------------------------------------------------------------- GPU

W, H, PS, SEED, THR, RES = 640, 480, 10, 20141105, 50.0, 0.2


@pytest.fixture(scope="module")
def run_case(mdx, oracle):
    """Seven 640 x 480 rgb frames (three runs of a five-frame ring), the checker's halves, and the oracle's
    trajectories of each ring."""
    from traj_seq import sequence
    frames = sequence(mdx, oracle, W, H, 7, seed=33, channels=3)
    halves = [half_ref(f) for f in frames]
    refs = [oracle.flow_trajectory(halves[e - 5:e], pixel_step=PS, nthreads=8) for e in range(5, 8)]
    return frames, halves, refs


def expected_chain(mdx, refs):
    """What OutlierDetector and FlowClusterer return for the oracle's trajectories, one rand() stream."""
    from motion_detection_amd.flow_clusterer import bounding_rects
    od, fc = mdx.OutlierDetector(seed=SEED), mdx.FlowClusterer()
    out = []
    for ref in refs:
        traj = [np.asarray(t, np.float32) for t in ref["trajectories"]]
        outliers: list = []
        sub = od.fitSubspace(traj, outliers, 2, RES)
        clusters = fc.clusterEuclidean(np.asarray(outliers, np.float32).reshape(-1, 2), THR)
        out.append((traj, outliers, sub, clusters, bounding_rects(clusters)))
    od.close()
    fc.close()
    return out


def vector_image(ref, w, h):
    v = np.zeros((h, w, 4))
    ix = ref["start_pts"].astype(np.int64)
    for i in range(len(ix)):
        x, y = ix[i]
        if 0 <= x < w and 0 <= y < h:
            v[y, x] = ref["vectors"][i]
    return v


@pytest.mark.gpu
def test_python_node_run_mode_matches_oracle(mdx, run_case):
    frames, halves, refs = run_case
    want = expected_chain(mdx, refs)
    n = MotionDetectionNode({"use_all_frames": False, "distance_threshold": THR, "seed": SEED, "pixel_step": PS,
                             "num_motions": 2})
    got = []
    for f in frames:
        assert n.image_callback(Image.from_array(f, "rgb8")) is None
        got.append(n.run_once())
    assert [g is not None for g in got] == [False] * 4 + [True] * 3
    dw, dh = half_size_ref(W, H)
    for g, ref, (traj, outliers, sub, clusters, rects) in zip(got[4:], refs, want):
        assert g.num_vectors == ref["num_vectors"] and len(traj) > 50 and len(outliers) > 0
        assert len(g.trajectories) == len(traj)
        assert np.array_equal(np.array(g.trajectories).view(np.uint32), np.array(traj).view(np.uint32))
        assert g.optical_flow_vectors.shape == (dh, dw, 4)
        assert np.array_equal(g.optical_flow_vectors.view(np.uint64), vector_image(ref, dw, dh).view(np.uint64))
        assert np.array_equal(np.asarray(g.outlier_points, np.float32), np.asarray(outliers, np.float32))
        assert len(g.subspace) == len(sub) and all(np.array_equal(a, b) for a, b in zip(g.subspace, sub))
        assert len(g.clusters) == len(clusters) and all(np.array_equal(a, b) for a, b in zip(g.clusters, clusters))
        assert g.rectangles == rects
    n.ofc.close()


@pytest.mark.gpu
def test_cpp_node_run_mode_matches_oracle(node_exe, tmp_path, mdx, run_case):
    frames, halves, refs = run_case
    want = expected_chain(mdx, refs)
    p, out = run_node(node_exe, tmp_path, rgb8(frames), use_all_frames=0, distance_threshold=THR, seed=SEED,
                      pixel_step=PS, num_motions=2, residual_threshold=RES, log_contours=1)
    assert p.returncode == 0, p.stderr
    assert "processed 3 of 7" in p.stdout, p.stdout
    from motion_detection_amd.formats import write_flow, write_trajectories
    dw, dh = half_size_ref(W, H)
    for k, (ref, (traj, outliers, sub, clusters, rects)) in enumerate(zip(refs, want)):
        r = read_res(out / f"res_{k}.bin", live=True)
        assert (r["num"], r["w"], r["h"]) == (ref["num_vectors"], dw, dh)
        assert np.array_equal(r["traj"].view(np.uint32), np.array(traj, np.float32).view(np.uint32))
        assert np.array_equal(r["outliers"], np.asarray(outliers, np.float32).reshape(-1, 2))
        num_all, labels, kept, rc = read_clusters(out / f"clusters_{k}.bin", len(outliers))
        assert [tuple(x) for x in rc.tolist()] == [tuple(x) for x in rects]
        got_clusters = [r["outliers"][labels == c] for c in kept]
        assert len(got_clusters) == len(clusters) and all(np.array_equal(a, b) for a, b in zip(got_clusters, clusters))
        pyf = str(tmp_path / f"py_{k}")
        write_flow(vector_image(ref, dw, dh), pyf, PS)
        write_trajectories(traj, pyf + "_traj")
        for sfx in ("_h", "_f"):
            assert open(out / f"flow_{k}{sfx}", "rb").read() == open(pyf + sfx, "rb").read()
        assert open(out / f"traj_{k}", "rb").read() == open(pyf + "_traj", "rb").read()
    assert not list(out.glob("pub_*"))                          # run() publishes nothing here
    assert open(out / "motion.log").read() == ""                # and logs nothing (run() has no writeBoundingBox)


@pytest.mark.gpu
def test_default_cpp_node_run_is_unchanged_by_the_new_parameters(node_exe, tmp_path, mdx, oracle):
    from traj_seq import sequence
    frames = rgb8(sequence(mdx, oracle, 320, 240, 6, seed=12, channels=3))
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    pa, oa = run_node(node_exe, tmp_path / "a", frames, seed=SEED, distance_threshold=THR)
    pb, ob = run_node(node_exe, tmp_path / "b", frames, seed=SEED, distance_threshold=THR, use_all_frames=1,
                      residual_threshold=0.2)
    assert pa.returncode == 0 and pb.returncode == 0, pa.stderr + pb.stderr
    a, b = dir_bytes(str(oa)), dir_bytes(str(ob))
    assert "processed 2 of 6" in pa.stdout and pa.stdout == pb.stdout
    assert sorted(a) == sorted(b) and len(a) >= 2 * 6 and all(a[k] == b[k] for k in a)
