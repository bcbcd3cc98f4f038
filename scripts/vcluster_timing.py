#!/usr/bin/env python3
"""Time mdx_cluster_vectors against the reference's loop shape on one host thread.

    python scripts/vcluster_timing.py [--out profiles/vcluster_timing.txt] [--device 0] [--no-trace]

Input: the first N = 256, 2,048 and 20,736 vectors, in visiting order (rows outer), of a 1080p grid at
pixel_step 10 whose flow is a global translation, three moving patches and noise (3 % of the vectors
point anywhere); thresholds 50 px and 0.15 rad (the launch files' values); with and without
MDX_VCLUSTER_ABS_INT.  Per case: the wall time
of one mdx_cluster_vectors call, its copies included (median of 20 after 3 warm-ups), and the same
input through scripts/micro/vcluster_cpu.cpp (g++ -O2, one thread, built here into
scripts/micro/bin/) on this machine's host.  Both must produce the same counts.

Every device step is a child process of its own under `timeout`, and the first one that fails ends
the run (the steps are chained as with &&).  The last step, unless --no-trace, is a separate
`rocprofv3 --kernel-trace --stats` run of the largest case, from whose kernel records the report
splits the device time between the scan, gather and walk launches.
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

SIZES = (256, 2048, 20736)
THR, ATHR = 50.0, 0.15
WARMUP, REPS = 3, 20
STEP_TIMEOUT = 240          # seconds per device step


def flow_field(n):
    """(n, 4) float64: the first n grid vectors of 1920 x 1080 at step 10, rows outer."""
    rng = np.random.default_rng(20736)
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


def device_step(n, abs_int, device, reps):
    import motion_detection_amd as m
    from motion_detection_amd._lib import VCLUSTER_ABS_INT, lib
    vec = flow_field(n)
    labels = np.zeros(n, np.int32)
    cap = n // 6
    kept = np.zeros(cap, np.int32)
    rects = np.zeros((cap, 4), np.int32)
    nact, nall, nkept = C.c_int(0), C.c_int(0), C.c_int(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    ts = []
    with m.Context(device, 64, 64, 1) as ctx:
        for it in range(WARMUP + reps):
            t0 = time.perf_counter()
            rc = lib().mdx_cluster_vectors(ctx._h, vp(vec), n, THR, ATHR, 5, VCLUSTER_ABS_INT if abs_int else 0,
                                           vp(labels), C.byref(nact), C.byref(nall), vp(kept), vp(rects), cap,
                                           C.byref(nkept))
            t1 = time.perf_counter()
            if rc != 0:
                raise SystemExit(f"mdx_cluster_vectors: {rc} {lib().mdx_last_error(ctx._h)}")
            if it >= WARMUP:
                ts.append((t1 - t0) * 1e3)
    info = m._lib.build_info()
    print(json.dumps(dict(n=n, abs_int=abs_int, ms=float(np.median(ts)), min=min(ts), max=max(ts), active=nact.value,
                          all=nall.value, kept=nkept.value, sha=info["src_sha256"], matches=info["matches_tree"])))


def run_step(args, n, abs_int, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--step", str(n), "--abs-int", str(int(abs_int)),
                          "--device", str(args.device)]
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT)] + cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit(f"device step n={n} abs_int={abs_int} ended with {p.returncode}; nothing more is run\n"
                         + p.stdout[-2000:] + p.stderr[-2000:])
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def build_cpu():
    src = os.path.join(ROOT, "scripts", "micro", "vcluster_cpu.cpp")
    bindir = os.path.join(ROOT, "scripts", "micro", "bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, "vcluster_cpu")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", exe, src], check=True)
    return exe


def kernel_split(args, n):
    """Device time per kernel of one traced run of the largest case (its warm-ups included)."""
    d = tempfile.mkdtemp(prefix="vcluster_kt_")
    run_step(args, n, False, prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run", "--output-format",
                                     "csv", "--"])
    tot, cnt = {}, {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r["Kernel_Name"].split("(")[0].split("::")[-1]
            tot[name] = tot.get(name, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            cnt[name] = cnt.get(name, 0) + 1
    return tot, cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vcluster_timing.txt"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--step", type=int, default=0, help="(internal) run one device step of this size")
    ap.add_argument("--abs-int", type=int, default=0)
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    if args.step:
        device_step(args.step, bool(args.abs_int), args.device, REPS)
        return
    exe = build_cpu()
    rows = []
    tmp = os.path.join(ROOT, "scripts", "micro", "bin", "vcluster_vectors.f64")
    sha = None
    for abs_int in (False, True):
        for n in SIZES:
            r = run_step(args, n, abs_int)
            sha = (r["sha"], r["matches"])
            flow_field(n).tofile(tmp)
            out = subprocess.run([exe, tmp, str(n), repr(THR), repr(ATHR), str(int(abs_int)), "20" if n <= 2048 else "1"],
                                 capture_output=True, text=True, check=True).stdout.split()
            cpu = dict(active=int(out[3]), all=int(out[5]), kept=int(out[7]), ms=float(out[9]))
            if (cpu["active"], cpu["all"], cpu["kept"]) != (r["active"], r["all"], r["kept"]):
                raise SystemExit(f"N={n} abs_int={abs_int}: device {r['active']}/{r['all']}/{r['kept']}, CPU loop "
                                 f"{cpu['active']}/{cpu['all']}/{cpu['kept']} (active / clusters / kept)")
            rows.append((n, abs_int, r, cpu))
    os.remove(tmp)
    lines = [f"mdx_cluster_vectors vs the reference's loop shape (one host thread, g++ -O2); library src_sha256 {sha[0]} "
             f"(matches tree: {sha[1]})",
             f"first N vectors (rows outer) of a 1080p grid at step 10: translation + 3 moving patches + noise; thresholds "
             f"{THR:g} px, {ATHR:g} rad; device: wall ms of one call, copies included, median of {REPS} after {WARMUP} "
             f"warm-ups; launches = 3 * ceil(active / 256) - 1",
             f"{'N':>7} {'abs_int':>7} {'launches':>8} {'device ms':>10} {'min':>8} {'max':>8} {'cpu ms':>11} "
             f"{'cpu/device':>10} {'clusters':>8} {'kept':>5}"]
    for n, abs_int, r, cpu in rows:
        lines.append(f"{n:>7} {int(abs_int):>7} {3 * -(-r['active'] // 256) - 1:>8} {r['ms']:>10.4f} {r['min']:>8.4f} "
                     f"{r['max']:>8.4f} {cpu['ms']:>11.4f} {cpu['ms'] / r['ms']:>10.2f} {r['all']:>8} {r['kept']:>5}")
    if not args.no_trace:
        tot, cnt = kernel_split(args, SIZES[-1])
        calls = WARMUP + REPS
        lines.append(f"kernel records of a separate rocprofv3 --kernel-trace --stats run, N = {SIZES[-1]}, abs_int 0, "
                     f"{calls} calls: device us per call (launches per call)")
        for k in sorted(tot):
            if "vcluster" in k:
                lines.append(f"  {k:<20} {tot[k] / 1e3 / calls:>10.1f} ({cnt[k] // calls})")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
