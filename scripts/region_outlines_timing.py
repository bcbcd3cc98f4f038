#!/usr/bin/env python3
"""Time mdx_region_outlines_dev against mdx_mask_regions_dev on the same masks, and against what a caller does
without it: copy the label images to the host and follow each blob's border on one host thread.

    python scripts/region_outlines_timing.py [--out profiles/region_outlines_timing.txt] [--device 0] [--cases 1080p,4k]

At 1920 x 1080 x 32 and 3840 x 2160 x 8, on five inputs, min_area 50, 4,096 records per image:
  recipe   the end-to-end recipe's opened masks (mdx_flow_warp_diff_batch_dev with the true homography and
           thresh 30 on synthetic pairs): almost all background
  blob     one frame-wide blob per frame (a 0.60-density random mask without the opening)
  noise    0.45-density random masks without the opening: one giant blob among thousands, thousands of holes
  rings    frame-filling nested rings, 8 pixels apart, 3 thick
  serp     a full-frame one-pixel serpentine: one outline of about w * h points, the longest looked for
Columns, all for the whole batch:
  outlines ms  one mdx_region_outlines_dev call (offsets, points and counts; room for 2 * w * h points per image)
               between two HIP events on the context's stream, median of 20 after 3 warm-ups; min and max next to it
  regions ms   one mdx_mask_regions_dev call (records, counts and labels) on the same masks in the same run, the
               same way
  setup .. scatter  the call's four parts (the five set-up kernels, the rounds, the offsets, the scatter), from
               mdx_enable_timing's events: mean over the same calls
  launches     kernel launches the call queues (fixed by w and h); scratch MB: the context's scratch for the batch
  states/img   the states ranked per image (mean over the batch), counted on the host from the labels
  d2h ms       the device-to-host copy of the label images into page-locked memory, by events, median of 20
  cpu ms       scripts/micro/region_outlines_cpu.cpp on them (g++ -O2, one thread, built here into
               scripts/micro/bin/), median of 3
Both sides must count the same points.  The report carries the library's src_sha256.
"""
import argparse
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"1080p": (1920, 1080, 32), "4k": (3840, 2160, 8)}
MIN_AREA, WARMUP, CAP = 50, 3, 4096
PARTS = ["setup", "rounds", "offsets", "scatter"]


def build_cpu():
    src = os.path.join(ROOT, "scripts", "micro", "region_outlines_cpu.cpp")
    bindir = os.path.join(ROOT, "scripts", "micro", "bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, "region_outlines_cpu")
    subprocess.run(["g++", "-O2", "-o", exe, src], check=True)
    return exe


def rings(B, h, w):
    y, x = np.mgrid[0:h, 0:w]
    inset = np.minimum(np.minimum(x, w - 1 - x), np.minimum(y, h - 1 - y))
    return np.broadcast_to(np.where(inset % 8 < 3, 255, 0).astype(np.uint8), (B, h, w)).copy()


def serpentine(B, h, w):
    y, x = np.mgrid[0:h, 0:w]
    s = (y % 2 == 0) | ((y % 4 == 1) & (x == w - 1)) | ((y % 4 == 3) & (x == 0))
    return np.broadcast_to(np.where(s, 255, 0).astype(np.uint8), (B, h, w)).copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_outlines_timing.txt"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--cases", default="1080p,4k")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import ctypes as C
    import torch
    import motion_detection_amd as m
    exe = None if args.no_cpu else build_cpu()
    info = m._lib.build_info()
    lines = [f"mdx_region_outlines_dev vs mdx_mask_regions_dev on the same masks, and vs D2H copy of the labels + border "
             f"following on one host thread (g++ -O2); library src_sha256 {info['src_sha256']} (matches tree: "
             f"{info['matches_tree']})",
             f"min_area {MIN_AREA}, {CAP} records per image, room for 2*w*h points per image; device and d2h: HIP events on the "
             f"context stream, median of {args.reps} after {WARMUP} warm-ups; parts: mean over the same calls; cpu: median of "
             f"3; all times are ms for the whole batch",
             f"{'case':>6} {'input':>7} {'batch':>5} {'outlines':>9} {'min':>8} {'max':>8} {'regions':>9} {'out/reg':>7} "
             + " ".join(f"{k:>8}" for k in PARTS) + f" {'launches':>8} {'scratch MB':>10} {'states/img':>10} {'d2h':>8} {'cpu':>10} "
             f"{'(d2h+cpu)/outlines':>18} {'kept':>7} {'points':>10}"]
    tmp = os.path.join(ROOT, "scripts", "micro", "bin", "region_outlines_labels.i32")
    for case in args.cases.split(","):
        w, h, B = CASES[case]
        N = w * h
        maxp = 2 * N
        launches = 7 + math.ceil(math.log2(7 * N))
        scratch = B * (61 * N + 4 * ((N + 255) // 256) + 260) + 765
        with m.Context(args.device, w, h, B, fit_mode=m.FIT_EXTERNAL, thresh=30) as c:
            stream = torch.cuda.ExternalStream(c.stream, device=args.device)
            pairs = [m.synth_pair(20141105 + i, w, h, 1, nthreads=16) for i in range(B)]
            g1, g2 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
            Hs = np.stack([p[2] for p in pairs]).astype(np.float64)
            n = m.grid_count(w, h, c.params.pixel_step)
            d = dict(i1=c.dev_alloc(g1.nbytes), i2=c.dev_alloc(g2.nbytes), H=c.dev_alloc(Hs.nbytes), np=c.dev_alloc(B * n * 8),
                     st=c.dev_alloc(B * n), mask=c.dev_alloc(B * N), regs=c.dev_alloc(B * CAP * 32), nall=c.dev_alloc(B * 4),
                     nkept=c.dev_alloc(B * 4), labels=c.dev_alloc(B * N * 4), off=c.dev_alloc(B * (CAP + 1) * 4),
                     xy=c.dev_alloc(B * maxp * 8), npts=c.dev_alloc(B * 4))
            c.h2d(d["i1"], g1), c.h2d(d["i2"], g2), c.h2d(d["H"], Hs)
            c.flow_warp_diff_batch_dev(B, d["i1"], d["i2"], w, h, w, w * h, m.FMT_GRAY8, d["np"], d["st"], 0, d["mask"],
                                       0, d["H"], 0)
            c.sync()
            host = m.host_empty((B, h, w), np.int32)
            rng = np.random.default_rng(45)
            inputs = (("recipe", True, None),
                      ("blob", False, lambda: np.where(rng.random((B, h, w)) < 0.60, 255, 0).astype(np.uint8)),
                      ("noise", False, lambda: np.where(rng.random((B, h, w)) < 0.45, 255, 0).astype(np.uint8)),
                      ("rings", False, lambda: rings(B, h, w)),
                      ("serp", False, lambda: serpentine(B, h, w)))
            for name, op, make in inputs:
                if make is not None:
                    c.h2d(d["mask"], make())
                to, tr, tc = [], [], []
                for it in range(WARMUP + args.reps):
                    if it == WARMUP:
                        c.sync()
                        c.enable_timing(True)
                    e0, e1, e2, e3 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
                    e0.record(stream)
                    c.mask_regions_dev(B, d["mask"], w, h, w, N, op, MIN_AREA, d["regs"], CAP, d["nall"], d["nkept"],
                                       d["labels"])
                    e1.record(stream)
                    c.region_outlines_dev(B, d["labels"], w, h, d["regs"], CAP, d["nkept"], d["off"], d["xy"], maxp, d["npts"])
                    e2.record(stream)
                    c.d2h(host, d["labels"])
                    e3.record(stream)
                    c.sync()
                    if it >= WARMUP:
                        tr.append(e0.elapsed_time(e1)), to.append(e1.elapsed_time(e2)), tc.append(e2.elapsed_time(e3))
                parts = []
                for i in range(len(PARTS)):
                    ms = C.c_float(0)
                    c._check(m.lib().mdx_stage_ms(c._h, i, C.byref(ms)))
                    parts.append(ms.value / max(m.lib().mdx_timing_calls(c._h), 1))
                c.enable_timing(False)
                nkept, npts = np.zeros(B, np.int32), np.zeros(B, np.int32)
                c.d2h(nkept, d["nkept"]), c.d2h(npts, d["npts"])
                out_ms, reg, d2h = float(np.median(to)), float(np.median(tr)), float(np.median(tc))
                cpu_ms, states = float("nan"), float("nan")
                if exe:
                    np.asarray(host).tofile(tmp)
                    res = subprocess.run([exe, tmp, str(w), str(h), str(B), str(MIN_AREA), str(CAP), "3"], capture_output=True,
                                         text=True, check=True).stdout.split()
                    if int(res[1]) != int(npts.astype(np.int64).sum()):
                        raise SystemExit(f"{case} {name}: device {npts.sum()} points, CPU {res[1]}")
                    states, cpu_ms = int(res[3]) / B, float(res[5])
                lines.append(f"{case:>6} {name:>7} {B:>5} {out_ms:>9.4f} {min(to):>8.4f} {max(to):>8.4f} {reg:>9.4f} "
                             f"{out_ms / reg:>7.2f} " + " ".join(f"{k:>8.4f}" for k in parts)
                             + f" {launches:>8} {scratch / 1e6:>10.1f} {states:>10.0f} {d2h:>8.3f} {cpu_ms:>10.2f} "
                             f"{(d2h + cpu_ms) / out_ms:>18.1f} {int(np.minimum(nkept, CAP).sum()):>7} "
                             f"{int(npts.astype(np.int64).sum()):>10}")
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
