#!/usr/bin/env python3
"""Time mdx_mask_regions_dev against what a caller does without it: copy the masks to the host and
label them on one host thread.

    python scripts/regions_timing.py [--out profiles/regions_timing.txt] [--device 0] [--cases 1080p,4k]

At 1920 x 1080 x 32 and 3840 x 2160 x 8, on two inputs -- the masks of the end-to-end recipe
(mdx_flow_warp_diff_batch_dev with the true homography and thresh 30 on synthetic pairs) and
0.45-density random masks, those with and without the 3x3 opening (the opening reduces noise to specks;
without it the mask is one giant component among thousands) -- min_area 50:
  device ms   one mdx_mask_regions_dev call (records and counts only) between two HIP events on the
              context's stream, median of 20 after 3 warm-ups
  d2h ms      the device-to-host copy of the same masks into page-locked memory, by events, median of 20
  cpu ms      the same masks through scripts/micro/regions_cpu.cpp (opening + two-pass union-find, g++
              -O2, one thread, built here into scripts/micro/bin/), median of 3
Both sides must count the same components.  Per-kernel times come from a kernel trace of this script
(--reps 3 keeps it short); the report carries the library's src_sha256.
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"1080p": (1920, 1080, 32), "4k": (3840, 2160, 8)}
MIN_AREA, WARMUP = 50, 3


def build_cpu():
    src = os.path.join(ROOT, "scripts", "micro", "regions_cpu.cpp")
    bindir = os.path.join(ROOT, "scripts", "micro", "bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, "regions_cpu")
    subprocess.run(["g++", "-O2", "-o", exe, src], check=True)
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions_timing.txt"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--cases", default="1080p,4k")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    import motion_detection_amd as m
    exe = None if args.no_cpu else build_cpu()
    info = m._lib.build_info()
    lines = [f"mdx_mask_regions_dev vs D2H copy + opening + two-pass union-find on one host thread (g++ -O2); library "
             f"src_sha256 {info['src_sha256']} (matches tree: {info['matches_tree']})",
             f"min_area {MIN_AREA}; device and d2h: HIP events on the context stream, median of {args.reps} after "
             f"{WARMUP} warm-ups; cpu: median of 3; all times are for the whole batch",
             f"{'case':>6} {'input':>8} {'open3':>5} {'batch':>5} {'device ms':>10} {'min':>8} {'max':>8} {'d2h ms':>8} {'cpu ms':>10} "
             f"{'(d2h+cpu)/device':>16} {'components':>10} {'kept':>7}"]
    tmp = os.path.join(ROOT, "scripts", "micro", "bin", "regions_masks.u8")
    for case in args.cases.split(","):
        w, h, B = CASES[case]
        N = w * h
        with m.Context(args.device, w, h, B, fit_mode=m.FIT_EXTERNAL, thresh=30) as c:
            stream = torch.cuda.ExternalStream(c.stream, device=args.device)
            pairs = [m.synth_pair(20141105 + i, w, h, 1, nthreads=16) for i in range(B)]
            g1, g2 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
            Hs = np.stack([p[2] for p in pairs]).astype(np.float64)
            n = m.grid_count(w, h, c.params.pixel_step)
            cap = 4096
            d = dict(i1=c.dev_alloc(g1.nbytes), i2=c.dev_alloc(g2.nbytes), H=c.dev_alloc(Hs.nbytes), np=c.dev_alloc(B * n * 8),
                     st=c.dev_alloc(B * n), mask=c.dev_alloc(B * N), regs=c.dev_alloc(B * cap * 32), nall=c.dev_alloc(B * 4),
                     nkept=c.dev_alloc(B * 4))
            c.h2d(d["i1"], g1), c.h2d(d["i2"], g2), c.h2d(d["H"], Hs)
            c.flow_warp_diff_batch_dev(B, d["i1"], d["i2"], w, h, w, w * h, m.FMT_GRAY8, d["np"], d["st"], 0, d["mask"],
                                       0, d["H"], 0)
            c.sync()
            host = m.host_empty((B, h, w), np.uint8)
            rnd = np.where(np.random.default_rng(45).random((B, h, w)) < 0.45, 255, 0).astype(np.uint8)
            for name, op in (("recipe", True), ("random", True), ("random", False)):
                if name == "random" and op:
                    c.h2d(d["mask"], rnd)
                ts, cs = [], []
                for it in range(WARMUP + args.reps):
                    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                    e0.record(stream)
                    c.mask_regions_dev(B, d["mask"], w, h, w, N, op, MIN_AREA, d["regs"], cap, d["nall"], d["nkept"])
                    e1.record(stream)
                    c.d2h(host, d["mask"])
                    e2.record(stream)
                    c.sync()
                    if it >= WARMUP:
                        ts.append(e0.elapsed_time(e1))
                        cs.append(e1.elapsed_time(e2))
                nall, nkept = np.zeros(B, np.int32), np.zeros(B, np.int32)
                c.d2h(nall, d["nall"]), c.d2h(nkept, d["nkept"])
                dev, d2h = float(np.median(ts)), float(np.median(cs))
                cpu_ms = float("nan")
                if exe:
                    np.asarray(host).tofile(tmp)
                    out = subprocess.run([exe, tmp, str(w), str(h), str(B), str(int(op)), str(MIN_AREA), "3"], capture_output=True,
                                         text=True, check=True).stdout.split()
                    if (int(out[3]), int(out[5])) != (int(nall.sum()), int(nkept.sum())):
                        raise SystemExit(f"{case} {name}: device {nall.sum()}/{nkept.sum()} components, CPU {out[3]}/{out[5]}")
                    cpu_ms = float(out[7])
                lines.append(f"{case:>6} {name:>8} {int(op):>5} {B:>5} {dev:>10.4f} {min(ts):>8.4f} {max(ts):>8.4f} {d2h:>8.4f} "
                             f"{cpu_ms:>10.2f} {(d2h + cpu_ms) / dev:>16.2f} {int(nall.sum()):>10} {int(nkept.sum()):>7}")
                print(lines[-1], flush=True)
            for p in d.values():
                c.dev_free(p)
    if exe and os.path.exists(tmp):
        os.remove(tmp)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
