"""Driving host/mdx_node from a test and reading what it wrote (test helper, not a test module).

The binary's input stream and every output file are laid out as the comment at the top of
host/mdx_node_main.cpp says; the parsers here check each file's length against its header.  A test
module that runs the binary imports the `node_exe` fixture by name.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "host")
EXE = os.path.join(HOST, "mdx_node")


@pytest.fixture(scope="module")
def node_exe(mdx):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    return EXE


def write_frames(path, frames):
    """frames: list of (array, encoding); the binary's MDXF stream of sensor_msgs/Image records."""
    with open(path, "wb") as f:
        f.write(b"MDXF" + struct.pack("<I", len(frames)))
        for a, enc in frames:
            a = np.ascontiguousarray(a, np.uint8)
            h, w = a.shape[:2]
            step = a.strides[0]
            f.write(struct.pack("<4I", h, w, step, len(enc)) + enc.encode() + a.tobytes())


def rgb8(seq):
    """A list of (h, w, 3) arrays as run_node's frames."""
    return [(a, "rgb8") for a in seq]


def run_node(exe, tmp_path, frames, **params):
    fpath = tmp_path / "frames.bin"
    write_frames(str(fpath), frames)
    out = tmp_path / "out"
    out.mkdir()
    args = [exe, str(fpath), str(out)] + [f"{k}={int(v) if isinstance(v, bool) else v}" for k, v in params.items()]
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    return p, out


def log_lines(frame, rects):
    """MotionLogger::writeBoundingBox's lines of one frame's rectangles (x, y, width, height)."""
    return "".join(f"{frame}, {i}, {x}, {y}, {x + w}, {y + h}\n" for i, (x, y, w, h) in enumerate(np.asarray(rects).tolist()))


def dir_bytes(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def read_res(path, live):
    b = open(path, "rb").read()
    num, rc, w, h, npts, ntraj, tl, nout = struct.unpack_from("<8i", b, 0)
    o = 32
    H = np.frombuffer(b, np.float64, 9, o).reshape(3, 3)
    o += 72
    r = dict(num=num, rc=rc, w=w, h=h, npts=npts, H=H)
    if not live:
        r["next_pts"] = np.frombuffer(b, np.float32, 2 * npts, o).reshape(npts, 2)
        o += 8 * npts
        r["status"] = np.frombuffer(b, np.uint8, npts, o)
        o += npts
        r["mask"] = np.frombuffer(b, np.uint8, w * h, o).reshape(h, w)
    else:
        r["traj"] = np.frombuffer(b, np.float32, ntraj * tl * 2, o).reshape(ntraj, tl, 2)
        o += ntraj * tl * 8
        r["outliers"] = np.frombuffer(b, np.float32, nout * 2, o).reshape(nout, 2)
        o += nout * 8
        nc = struct.unpack_from("<i", b, o)[0]
        r["columns"] = np.frombuffer(b, np.int32, nc, o + 4)
    return r


def read_outlier_points(path):
    """fitSubspace's outlier points of a live res_<k>.bin."""
    return read_res(path, live=True)["outliers"].copy()


def read_mask(path):
    """The motion mask of a pair-path res_<k>.bin."""
    return read_res(path, live=False)["mask"].copy()


def read_clusters(path, nout):
    b = open(path, "rb").read()
    num_all, num_kept = struct.unpack_from("<2i", b, 0)
    assert len(b) == 8 + 4 * nout + 4 * num_kept + 16 * num_kept
    labels = np.frombuffer(b, np.int32, nout, 8)
    kept = np.frombuffer(b, np.int32, num_kept, 8 + 4 * nout)
    rects = np.frombuffer(b, np.int32, 4 * num_kept, 8 + 4 * nout + 4 * num_kept).reshape(num_kept, 4)
    return num_all, labels, kept, rects


def read_vclusters(path):
    b = open(path, "rb").read()
    n, nact, num_all, num_kept = struct.unpack_from("<4i", b, 0)
    assert len(b) == 16 + 32 * n + 4 * n + 4 * num_kept + 16 * num_kept
    vec = np.frombuffer(b, np.float64, 4 * n, 16).reshape(n, 4)
    o = 16 + 32 * n
    labels = np.frombuffer(b, np.int32, n, o)
    kept = np.frombuffer(b, np.int32, num_kept, o + 4 * n)
    rects = np.frombuffer(b, np.int32, 4 * num_kept, o + 4 * n + 4 * num_kept).reshape(num_kept, 4)
    return vec, nact, num_all, labels, kept, rects


def read_outliers(path):
    b = open(path, "rb").read()
    n, sel, fa, fm, nout, nact, num_all, num_kept = struct.unpack_from("<8i", b, 0)
    med_a, mad_a, med_m, mad_m = struct.unpack_from("<4d", b, 32)
    assert len(b) == 64 + 32 * n + n + 4 * n + 4 * num_kept + 16 * num_kept
    vec = np.frombuffer(b, np.float64, 4 * n, 64).reshape(n, 4)
    o = 64 + 32 * n
    flags = np.frombuffer(b, np.uint8, n, o)
    labels = np.frombuffer(b[o + n:o + 5 * n], np.int32)
    kept = np.frombuffer(b[o + 5 * n:o + 5 * n + 4 * num_kept], np.int32)
    rects = np.frombuffer(b[o + 5 * n + 4 * num_kept:], np.int32).reshape(num_kept, 4)
    stats = dict(selected=sel, flagged_angle=fa, flagged_magnitude=fm, outliers=nout, median_angle=med_a,
                 mad_angle=mad_a, median_magnitude=med_m, mad_magnitude=mad_m)
    return vec, stats, flags, nact, num_all, labels, kept, rects


def read_regions(path):
    b = open(path, "rb").read()
    num_all, num_kept = struct.unpack_from("<2i", b, 0)
    assert len(b) == 8 + 32 * num_kept
    return num_all, np.frombuffer(b, np.int32, 8 * num_kept, 8).reshape(num_kept, 8)
