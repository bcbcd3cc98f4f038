#!/usr/bin/env python3
"""Time mdx_find_outliers against the reference's loop shape on one host thread.

    python scripts/outliers_timing.py [--out profiles/outliers_timing.txt] [--device 0] [--no-trace]

Input: the first n = 256, 2,048 and 20,736 vectors of a 1080p grid at pixel_step 10 whose flow is a
global translation, three moving patches and noise (3 % of the vectors point anywhere), one field per
call, and 32 such fields (different noise) of 20,736 vectors in one call.  Per case: the wall time of
one mdx_find_outliers call, its host atan2 pass and its copies included (median of 20 after 3
warm-ups), and the same input through scripts/micro/outliers_cpu.cpp (g++ -O2, one thread, built here
into scripts/micro/bin/) on this machine's host, which also times the atan2 pass alone: that pass is
paid on both sides.  Both must produce the same counts.  Every case is also run with MDX_OL_REG=0,
the kernel variant that re-reads its values on every pass where the default keeps them in registers.

Every device step is a child process of its own under `timeout`, and the first one that fails ends
the run (the steps are chained as with &&).  The last step, unless --no-trace, is a separate
`rocprofv3 --kernel-trace --stats` run of each case for the kernel's own time.
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((1, 256), (1, 2048), (1, 20736), (32, 20736))      # (batch, n)
WARMUP, REPS = 3, 20
STEP_TIMEOUT = 240          # seconds per device step


def flow_field(n, seed=0):
    """(n, 4) float64: the first n grid vectors of 1920 x 1080 at step 10, rows outer."""
    rng = np.random.default_rng(20736 + seed)
    ys, xs = np.meshgrid(np.arange(0, 1080, 10.0), np.arange(0, 1920, 10.0), indexing="ij")
    x, y = xs.ravel(), ys.ravel()
    dx, dy = np.full(x.shape, 3.0), np.full(x.shape, 1.0)                  # global translation
    for (x0, y0, x1, y1), (u, v) in [((200, 100, 520, 400), (-4.0, 2.0)), ((900, 300, 1300, 700), (1.0, -5.0)),
                                     ((1400, 600, 1800, 1000), (-2.0, -3.0)), ((0, 0, 700, 20), (-3.0, 0.5))]:
        m = (x >= x0) & (x < x1) & (y >= y0) & (y < y1)                    # moving patches (the last one
        dx[m], dy[m] = u, v                                                 # reaches the smallest case too)
    dx += rng.normal(0, 0.2, x.shape)
    dy += rng.normal(0, 0.2, x.shape)
    bad = rng.random(x.shape) < 0.03                                        # mistracked points: any direction
    ang = rng.uniform(0, 2 * np.pi, x.shape)
    dx[bad], dy[bad] = (3.0 * np.cos(ang))[bad], (3.0 * np.sin(ang))[bad]
    return np.ascontiguousarray(np.stack([x, y, dx, dy], 1)[:n])


def fields(batch, n):
    return np.ascontiguousarray(np.stack([flow_field(n, b) for b in range(batch)]))


def device_step(batch, n, device, reps):
    import motion_detection_amd as m
    from motion_detection_amd._lib import MdxOutlierStats, lib
    vec = fields(batch, n)
    flags = np.zeros((batch, n), np.uint8)
    out = np.zeros((batch, n, 4))
    stats = np.zeros(batch, np.dtype(MdxOutlierStats))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    ts = []
    with m.Context(device, 64, 64, 1) as ctx:
        for it in range(WARMUP + reps):
            t0 = time.perf_counter()
            rc = lib().mdx_find_outliers(ctx._h, vp(vec), batch, n, 0, vp(flags), vp(out), vp(stats))
            t1 = time.perf_counter()
            if rc != 0:
                raise SystemExit(f"mdx_find_outliers: {rc} {lib().mdx_last_error(ctx._h)}")
            if it >= WARMUP:
                ts.append((t1 - t0) * 1e3)
    info = m._lib.build_info()
    print(json.dumps(dict(batch=batch, n=n, ms=float(np.median(ts)), min=min(ts), max=max(ts),
                          selected=int(stats["selected"].sum()), angle=int(stats["flagged_angle"].sum()),
                          magnitude=int(stats["flagged_magnitude"].sum()), outliers=int(stats["outliers"].sum()),
                          sha=info["src_sha256"], matches=info["matches_tree"])))


def run_step(args, batch, n, prefix=(), reread=False):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--step", str(n), "--batch", str(batch),
                          "--device", str(args.device)]
    env = dict(os.environ, MDX_OL_REG="0" if reread else "1")
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT)] + cmd, capture_output=True, text=True, env=env)
    if p.returncode != 0:
        raise SystemExit(f"device step batch={batch} n={n} reread={reread} ended with {p.returncode}; nothing more is run\n"
                         + p.stdout[-2000:] + p.stderr[-2000:])
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def build_cpu():
    src = os.path.join(ROOT, "scripts", "micro", "outliers_cpu.cpp")
    bindir = os.path.join(ROOT, "scripts", "micro", "bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, "outliers_cpu")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", exe, src], check=True)
    return exe


def kernel_us(args, batch, n, reread):
    """Device time of k_outliers per call in one traced run of a case (its warm-ups included)."""
    d = tempfile.mkdtemp(prefix="outliers_kt_")
    run_step(args, batch, n, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format",
                                     "csv", "--"], reread=reread)
    tot, cnt = 0, 0
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            if "k_outliers" in r["Kernel_Name"]:
                tot += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
                cnt += 1
    return tot / 1e3 / max(cnt, 1), cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outliers_timing.txt"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--step", type=int, default=0, help="(internal) run one device step of this n")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    if args.step:
        device_step(args.batch, args.step, args.device, REPS)
        return
    exe = build_cpu()
    rows = []
    tmp = os.path.join(ROOT, "scripts", "micro", "bin", "outliers_vectors.f64")
    sha = None
    for batch, n in CASES:
        r = run_step(args, batch, n)
        rr = run_step(args, batch, n, reread=True)
        sha = (r["sha"], r["matches"])
        fields(batch, n).tofile(tmp)
        out = subprocess.run([exe, tmp, str(batch), str(n), "0", "20" if batch == 1 else "5"], capture_output=True,
                             text=True, check=True).stdout.split()
        cpu = dict(selected=int(out[5]), angle=int(out[7]), magnitude=int(out[9]), outliers=int(out[11]),
                   ms=float(out[13]), atan2_ms=float(out[15]))
        for k in ("selected", "angle", "magnitude", "outliers"):
            if cpu[k] != r[k] or cpu[k] != rr[k]:
                raise SystemExit(f"batch={batch} n={n}: device {k} {r[k]} / re-reading {rr[k]}, CPU loop {cpu[k]}")
        rows.append((batch, n, r, rr, cpu))
    os.remove(tmp)
    lines = [f"mdx_find_outliers vs the reference's loop shape (one host thread, g++ -O2); library src_sha256 {sha[0]} "
             f"(matches tree: {sha[1]})",
             f"first n vectors (rows outer) of a 1080p grid at step 10: translation + 3 moving patches + noise; device: wall "
             f"ms of one call, host atan2 pass and copies included, median of {REPS} after {WARMUP} warm-ups; one launch "
             f"per call; re-read ms: the same with MDX_OL_REG=0; atan2 ms: the host's atan2 pass alone (paid on both "
             f"sides), and its share of the device call",
             f"{'batch':>5} {'n':>7} {'device ms':>10} {'min':>8} {'max':>8} {'re-read ms':>10} {'cpu ms':>10} {'cpu/device':>10} "
             f"{'atan2 ms':>9} {'share':>6} {'outliers':>8}"]
    for batch, n, r, rr, cpu in rows:
        lines.append(f"{batch:>5} {n:>7} {r['ms']:>10.4f} {r['min']:>8.4f} {r['max']:>8.4f} {rr['ms']:>10.4f} {cpu['ms']:>10.4f} "
                     f"{cpu['ms'] / r['ms']:>10.2f} {cpu['atan2_ms']:>9.4f} {cpu['atan2_ms'] / r['ms']:>6.0%} {r['outliers']:>8}")
    if not args.no_trace:
        lines.append("k_outliers, device us per call, from a separate rocprofv3 --kernel-trace --stats run of each case "
                     "(launches counted): values in registers (the default at these sizes), re-read on every pass")
        for batch, n in CASES:
            us, cnt = kernel_us(args, batch, n, False)
            us0, cnt0 = kernel_us(args, batch, n, True)
            lines.append(f"{batch:>5} {n:>7} {us:>10.1f} ({cnt}) {us0:>10.1f} ({cnt0})")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
