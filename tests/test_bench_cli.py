"""bench.py's command line: a plain run is the headline leg alone (every other leg needs --full), and
--dump-outputs writes what the last timed step returned.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the fields of the legs a plain run leaves out
FULL_ONLY = ["value_unpipelined", "parity", "roofline", "cpu_baseline", "cpu_baseline_1core", "cpu_baseline_scalar",
             "full_path_4k", "full_path_ransac", "live_path"]


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE",
                                                             "MASTER_ADDR", "MASTER_PORT")}


def test_dump_outputs_types_budget_and_fixed_sample(tmp_path, monkeypatch):
    """Arrays that fit are written whole (float64 stays, the rest float32); one that does not fit its
    share of the budget is the elements at the seeded sorted indices, the same in every call; the
    files together stay within the budget."""
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)
    rng = np.random.default_rng(1)
    arrs = dict(H=rng.standard_normal((4, 9)), num_vectors=np.arange(4, dtype=np.int32) * 1000,
                status=rng.integers(0, 2, (4, 50)).astype(np.uint8),
                mask=(rng.integers(0, 2, (4, 30, 40)) * 255).astype(np.uint8))
    got = bench.dump_outputs(str(tmp_path / "a"), arrs)
    bench.dump_outputs(str(tmp_path / "b"), arrs)
    files = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in arrs}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{n}.npy" for n in arrs)
    assert files["H"].dtype == np.float64 and np.array_equal(files["H"], arrs["H"])
    for n in ("num_vectors", "status"):
        assert files[n].dtype == np.float32 and np.array_equal(files[n], arrs[n]) and files[n].shape == arrs[n].shape
    m = files["mask"]
    assert m.dtype == np.float32 and m.ndim == 1 and 0 < m.size < arrs["mask"].size
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, arrs["mask"].size, size=m.size))
    assert np.array_equal(m, arrs["mask"].reshape(-1)[idx])
    assert got["mask"] == [m.size, arrs["mask"].size] and got["H"] == [36, 36]
    assert sum(f.nbytes for f in files.values()) <= 4000
    for n in arrs:
        assert np.array_equal(files[n], np.load(tmp_path / "b" / f"{n}.npy"))


def test_dump_outputs_default_budget_is_under_64mb():
    import bench
    assert bench.DUMP_BUDGET_BYTES + 16 * 128 <= 64 * 1000 * 1000      # 128-byte .npy headers


def test_only_roofline_needs_full():
    out = subprocess.run([sys.executable, "bench.py", "--only-roofline"], env=_env(), cwd=ROOT, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 2 and "--full" in out.stderr
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]


@pytest.mark.gpu
def test_steps_beyond_the_stage_event_slots(mdx):
    """--steps sets the number of timed steps also past the 256 calls the library keeps stage events
    for: 260 steps are timed (runs of 256 + 4) and the stage times still cover every step."""
    import bench
    assert bench.TIMED_SLOTS == 256
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "260", "--warmup", "0", "--config", "640",
                          "--batch", "16"], env=_env(), cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert d["steps"] == 260 and d["ms_per_step"] > 0
    st = d["stage_ms_per_step"]
    assert 0 < st["lk"] < st["total"]
    assert d["value"] == pytest.approx(16 * 640 * 480 / 1e6 / (d["ms_per_step"] * 1e-3), rel=2e-3)   # both rounded


@pytest.mark.gpu
def test_plain_run_is_the_headline_leg_and_dumps_its_outputs(mdx, tmp_path):
    """`bench.py --gpus 1 --steps 2 --warmup 1` at 640x480 x 16: one JSON line whose steps and
    ms_per_step describe the timed steps, the --full legs absent, and the dumped arrays equal to the
    same pairs through the host entry of the path (one pair per call)."""
    import bench
    w, h, B = 640, 480, 16
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--config", "640",
                          "--batch", str(B), "--dump-outputs", str(tmp_path)], env=_env(), cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "Mpixels/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(B * w * h / 1e6 / (d["ms_per_step"] * 1e-3), rel=2e-3)   # both rounded
    for k in FULL_ONLY:
        assert d[k] is None, k
    assert d["dominant_kernel"]["roofline"] is None and d["parity_checked_pairs"] == 0
    n = mdx.grid_count(w, h, 10)
    files = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert sorted(files) == ["H", "mask", "next_pts", "num_vectors", "status", "vectors"]
    assert {k: list(v.shape) for k, v in files.items()} == dict(H=[B, 9], mask=[B, h, w], next_pts=[B, n, 2],
                                                                 num_vectors=[B], status=[B, n], vectors=[B, n, 4])
    assert all(v.dtype == (np.float64 if k in ("H", "vectors") else np.float32) for k, v in files.items())
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64 * 1000 * 1000
    assert d["dumped_outputs"] == {k: [v.size, v.size] for k, v in files.items()}
    assert int(files["num_vectors"][0]) == d["num_vectors_pair0"]
    with mdx.Context(0, w, h, 1, pixel_step=10, min_vector_size=1.0) as c:
        for i in range(B):
            a, b, _ = mdx.synth_pair(bench.SEED0 + i, w, h, 1, 16)
            r = c.flow_warp_diff(a, b)
            assert files["num_vectors"][i] == r.num_vectors, i
            np.testing.assert_array_equal(files["status"][i], r.status, err_msg=f"pair {i}")
            np.testing.assert_array_equal(files["next_pts"][i].view(np.uint32), r.next_pts.view(np.uint32),
                                          err_msg=f"pair {i}")
            np.testing.assert_array_equal(files["H"][i].view(np.uint64), np.asarray(r.H).ravel().view(np.uint64),
                                          err_msg=f"pair {i}")
            np.testing.assert_array_equal(files["mask"][i], r.mask, err_msg=f"pair {i}")
