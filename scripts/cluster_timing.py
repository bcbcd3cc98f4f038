#!/usr/bin/env python3
"""Time mdx_cluster_euclidean against the literal greedy loop on one host thread.

    python scripts/cluster_timing.py [--out profiles/cluster_timing.txt] [--device 0]

For N = 256, 2,048 and 20,736 (1080p grid points at pixel_step 10) uniform random points in
1920 x 1080, threshold 50: the wall time of one mdx_cluster_euclidean call, its copies included
(median of 20 after 3 warm-ups), and the same input through scripts/micro/cluster_cpu.cpp (the
reference's loop, g++ -O2, one thread, built here into scripts/micro/bin/) on this machine's host.
Both must produce the same cluster counts.  The report carries the library's src_sha256.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (256, 2048, 20736)
THR = 50.0
WARMUP, REPS = 3, 20


def build_cpu():
    src = os.path.join(ROOT, "scripts", "micro", "cluster_cpu.cpp")
    bindir = os.path.join(ROOT, "scripts", "micro", "bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, "cluster_cpu")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", exe, src], check=True)
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_timing.txt"))
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import motion_detection_amd as m
    from motion_detection_amd._lib import lib
    exe = build_cpu()
    info = m._lib.build_info()
    lines = [f"mdx_cluster_euclidean vs the literal greedy loop (one host thread, g++ -O2); library src_sha256 "
             f"{info['src_sha256']} (matches tree: {info['matches_tree']})",
             f"uniform random points in 1920 x 1080, threshold {THR:g}; device: wall ms of one call, copies included, "
             f"median of {REPS} after {WARMUP} warm-ups; launches = ceil(N / 256)",
             f"{'N':>7} {'launches':>8} {'device ms':>10} {'min':>8} {'max':>8} {'cpu ms':>10} {'cpu/device':>10} "
             f"{'clusters':>8} {'kept':>5}"]
    tmp = os.path.join(ROOT, "scripts", "micro", "bin", "cluster_points.f32")
    with m.Context(args.device, 64, 64, 1) as ctx:
        for n in SIZES:
            pts = np.random.default_rng(n).uniform(0, [1920, 1080], (n, 2)).astype(np.float32)
            labels = np.zeros(n, np.int32)
            cap = n // 6
            kept = np.zeros(cap, np.int32)
            rects = np.zeros((cap, 4), np.int32)
            nall, nkept = C.c_int(0), C.c_int(0)
            vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
            ts = []
            for it in range(WARMUP + REPS):
                t0 = time.perf_counter()
                rc = lib().mdx_cluster_euclidean(ctx._h, vp(pts), n, THR, 5, vp(labels), C.byref(nall), vp(kept),
                                                 vp(rects), cap, C.byref(nkept))
                t1 = time.perf_counter()
                if rc != 0:
                    raise SystemExit(f"mdx_cluster_euclidean: {rc}")
                if it >= WARMUP:
                    ts.append((t1 - t0) * 1e3)
            pts.tofile(tmp)
            cpu_reps = REPS if n <= 2048 else 3
            out = subprocess.run([exe, tmp, str(n), repr(THR), str(cpu_reps)], capture_output=True, text=True,
                                 check=True).stdout.split()
            cpu_all, cpu_kept, cpu_ms = int(out[3]), int(out[5]), float(out[7])
            if (cpu_all, cpu_kept) != (nall.value, nkept.value):
                raise SystemExit(f"N={n}: device {nall.value}/{nkept.value} clusters, CPU loop {cpu_all}/{cpu_kept}")
            dev = float(np.median(ts))
            lines.append(f"{n:>7} {-(-n // 256):>8} {dev:>10.4f} {min(ts):>8.4f} {max(ts):>8.4f} {cpu_ms:>10.4f} "
                         f"{cpu_ms / dev:>10.2f} {nall.value:>8} {nkept.value:>5}")
    os.remove(tmp)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
