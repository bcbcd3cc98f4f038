#!/usr/bin/env python3
"""Time mdx_region_hulls_dev against what a caller does without it: copy the label images to the host,
gather each region's pixels and run sort + monotone chain per region on one host thread.

    python scripts/region_hulls_timing.py [--out profiles/region_hulls_timing.txt] [--device 0] [--cases 1080p,4k]

At 1920 x 1080 x 32 and 3840 x 2160 x 8, max_regions 2048, on four inputs:
  recipe   the masks of the end-to-end recipe (mdx_flow_warp_diff_batch_dev with the true homography and
           thresh 30 on synthetic pairs), opened, min_area 50
  blob     one frame-wide blob per frame (the ellipse inscribed in the frame), min_area 50
  noise    0.45-density random masks without the opening, min_area chosen on frame 0 so that about 256
           regions are kept (one giant component among them)
  stripes  the adversarial overlap case: diagonal stripes 3 px apart ((x + y) % 3 == 0), min_area 50; every
           stripe is a region whose rectangle covers a large part of the frame, so every workgroup re-reads it
Per input:
  device ms   one mdx_region_hulls_dev call (its three launches) between two HIP events on the context's
              stream, median of 20 after 3 warm-ups
  k_hull ms   k_region_hull alone (mdx_enable_timing, stage 3), median of 20 further calls
  d2h ms      the device-to-host copy of d_labels into page-locked memory, by events, median of 20
  cpu ms      the label images through the host program below: one pass that groups the pixel coordinates by
              region, then scripts/hull_timing.py's host hull (cvRound, std::sort, std::unique, Andrew's
              monotone chain in int64) per region -- g++ -O2, one thread, timed inside the program without
              its file reads, min of its repetitions
Both sides must produce the same number of vertices.  The report carries the library's src_sha256.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from hull_timing import HOST_SRC  # noqa: E402  (its cross() and hull(), reused as they are)

CASES = {"1080p": (1920, 1080, 32), "4k": (3840, 2160, 8)}
MIN_AREA, WARMUP, CAP = 50, 3, 2048

HOST_MAIN = r"""
// region_hull_cpu <labels.i32> <w> <h> <batch> <records.i32> <cap> <reps>: records.i32 holds per image the
// number of records then cap records of 8 ints.  Per image: the pixels grouped by region in one pass over the
// labels (counting sort on the record index), then hull() per region.
int main(int argc, char** argv)
{
    if (argc < 8) return 2;
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), B = std::atoi(argv[4]), cap = std::atoi(argv[6]),
              reps = std::atoi(argv[7]);
    const size_t N = (size_t)w * h;
    std::vector<int32_t> lab(N * B), rec((size_t)B * (1 + 8 * (size_t)cap));
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp || std::fread(lab.data(), 4, lab.size(), fp) != lab.size()) return 1;
    std::fclose(fp);
    fp = std::fopen(argv[5], "rb");
    if (!fp || std::fread(rec.data(), 4, rec.size(), fp) != rec.size()) return 1;
    std::fclose(fp);
    std::vector<P> p, hl;
    std::vector<int32_t> slot;
    std::vector<size_t> start;
    std::vector<float> pts;
    double best = 1e30;
    size_t total = 0;
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        total = 0;
        for (int b = 0; b < B; b++) {
            const int32_t* L = lab.data() + N * b;
            const int32_t* R = rec.data() + (size_t)b * (1 + 8 * (size_t)cap);
            const int k = R[0];
            int32_t max_id = -1;
            for (int j = 0; j < k; j++) max_id = std::max(max_id, R[1 + 8 * j + 7]);
            slot.assign((size_t)max_id + 2, -1);
            for (int j = 0; j < k; j++) slot[R[1 + 8 * j + 7]] = j;
            start.assign((size_t)k + 1, 0);
            for (size_t i = 0; i < N; i++)
                if (L[i] >= 0 && L[i] <= max_id && slot[L[i]] >= 0) start[slot[L[i]] + 1]++;
            for (int j = 0; j < k; j++) start[j + 1] += start[j];
            pts.resize(2 * start[k]);
            std::vector<size_t> fill(start.begin(), start.end() - 1);
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) {
                    const int32_t v = L[(size_t)y * w + x];
                    if (v < 0 || v > max_id || slot[v] < 0) continue;
                    const size_t at = fill[slot[v]]++;
                    pts[2 * at] = (float)x, pts[2 * at + 1] = (float)y;
                }
            for (int j = 0; j < k; j++)
                if (start[j + 1] > start[j]) total += hull(pts.data() + 2 * start[j], (int)(start[j + 1] - start[j]), p, hl);
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        best = std::min(best, ms);
    }
    std::printf("vertices %zu ms %.6f\n", total, best);
    return 0;
}
"""


def build_cpu():
    bindir = os.path.join(ROOT, "scripts", "micro", "bin")
    os.makedirs(bindir, exist_ok=True)
    src, exe = os.path.join(bindir, "region_hull_cpu.cpp"), os.path.join(bindir, "region_hull_cpu")
    with open(src, "w") as f:
        f.write(HOST_SRC[:HOST_SRC.index("int main(")] + HOST_MAIN)
    subprocess.run(["g++", "-O2", "-o", exe, src], check=True)
    return exe


def inputs(w, h, B):
    """(name, masks or None for the recipe's, open3) of the synthetic inputs."""
    y, x = np.mgrid[0:h, 0:w]
    blob = ((2 * x - (w - 1)) / w) ** 2 + ((2 * y - (h - 1)) / h) ** 2 <= 1.0
    yield "recipe", None, True
    yield "blob", np.broadcast_to(np.where(blob, 255, 0).astype(np.uint8), (B, h, w)), False
    yield "noise", np.where(np.random.default_rng(45).random((B, h, w)) < 0.45, 255, 0).astype(np.uint8), False
    yield "stripes", np.broadcast_to(np.where((x + y) % 3 == 0, 255, 0).astype(np.uint8), (B, h, w)), False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_hulls_timing.txt"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--cases", default="1080p,4k")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    import motion_detection_amd as m
    from motion_detection_amd._lib import lib
    exe = None if args.no_cpu else build_cpu()
    info = m._lib.build_info()
    lines = [f"mdx_region_hulls_dev vs D2H copy of the labels + grouping + sort + monotone chain per region on one host thread "
             f"(g++ -O2); library src_sha256 {info['src_sha256']} (matches tree: {info['matches_tree']})",
             f"max_regions {CAP}; device, k_hull and d2h: HIP events on the context stream, median of {args.reps} after "
             f"{WARMUP} warm-ups; cpu: min of its repetitions; all times are for the whole batch",
             f"{'case':>6} {'input':>8} {'batch':>5} {'min_area':>8} {'device ms':>10} {'min':>8} {'max':>8} {'k_hull ms':>10} "
             f"{'d2h ms':>8} {'cpu ms':>10} {'(d2h+cpu)/device':>16} {'regions':>8} {'vertices':>8}"]
    bindir = os.path.join(ROOT, "scripts", "micro", "bin")
    tmp_l, tmp_r = os.path.join(bindir, "region_labels.i32"), os.path.join(bindir, "region_records.i32")
    for case in args.cases.split(","):
        w, h, B = CASES[case]
        N = w * h
        maxv = min(N, 2 * min(w, h) * CAP)
        with m.Context(args.device, w, h, B, fit_mode=m.FIT_EXTERNAL, thresh=30) as c:
            stream = torch.cuda.ExternalStream(c.stream, device=args.device)
            pairs = [m.synth_pair(20141105 + i, w, h, 1, nthreads=16) for i in range(B)]
            g1, g2 = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
            Hs = np.stack([p[2] for p in pairs]).astype(np.float64)
            n = m.grid_count(w, h, c.params.pixel_step)
            d = dict(i1=c.dev_alloc(g1.nbytes), i2=c.dev_alloc(g2.nbytes), H=c.dev_alloc(Hs.nbytes), np=c.dev_alloc(B * n * 8),
                     st=c.dev_alloc(B * n), mask=c.dev_alloc(B * N), regs=c.dev_alloc(B * CAP * 32), nall=c.dev_alloc(B * 4),
                     nkept=c.dev_alloc(B * 4), labels=c.dev_alloc(B * N * 4), offsets=c.dev_alloc(B * (CAP + 1) * 4),
                     xy=c.dev_alloc(B * maxv * 8), nv=c.dev_alloc(B * 4))
            c.h2d(d["i1"], g1), c.h2d(d["i2"], g2), c.h2d(d["H"], Hs)
            c.flow_warp_diff_batch_dev(B, d["i1"], d["i2"], w, h, w, w * h, m.FMT_GRAY8, d["np"], d["st"], 0, d["mask"],
                                       0, d["H"], 0)
            c.sync()
            host = m.host_empty((B, h, w), np.int32)
            for name, masks, op in inputs(w, h, B):
                if masks is not None:
                    c.h2d(d["mask"], np.ascontiguousarray(masks))
                min_area = MIN_AREA
                if name == "noise":                   # the area of frame 0's 256th largest component
                    areas = np.sort(c.mask_regions(masks[0], open3=False).regions[:, 4])[::-1]
                    min_area = int(areas[min(255, len(areas) - 1)])
                c.mask_regions_dev(B, d["mask"], w, h, w, N, op, min_area, d["regs"], CAP, d["nall"], d["nkept"], d["labels"])
                c.sync()
                ts, cs = [], []
                for it in range(WARMUP + args.reps):
                    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
                    e0.record(stream)
                    c.region_hulls_dev(B, d["labels"], w, h, d["regs"], CAP, d["nkept"], d["offsets"], d["xy"], maxv, d["nv"])
                    e1.record(stream)
                    c.d2h(host, d["labels"])
                    e2.record(stream)
                    c.sync()
                    if it >= WARMUP:
                        ts.append(e0.elapsed_time(e1))
                        cs.append(e1.elapsed_time(e2))
                kerns = []
                for it in range(args.reps):           # the same call again, one event set each
                    c._check(lib().mdx_enable_timing(c._h, 1))
                    c.region_hulls_dev(B, d["labels"], w, h, d["regs"], CAP, d["nkept"], d["offsets"], d["xy"], maxv, d["nv"])
                    kern = C.c_float(0)
                    c._check(lib().mdx_stage_ms(c._h, 3, C.byref(kern)))
                    kerns.append(kern.value)
                c._check(lib().mdx_enable_timing(c._h, 0))
                nkept, nv = np.zeros(B, np.int32), np.zeros(B, np.int32)
                regs = np.zeros((B, CAP, 8), np.int32)
                c.d2h(nkept, d["nkept"]), c.d2h(nv, d["nv"]), c.d2h(regs, d["regs"])
                if nkept.max() > CAP:
                    raise SystemExit(f"{case} {name}: {nkept.max()} regions kept, more than max_regions {CAP}")
                dev, d2h = float(np.median(ts)), float(np.median(cs))
                cpu_ms = float("nan")
                if exe:
                    np.asarray(host).tofile(tmp_l)
                    np.concatenate([nkept.reshape(B, 1), regs.reshape(B, -1)], 1).astype(np.int32).tofile(tmp_r)
                    reps = "1" if name in ("blob", "noise") else "3"
                    out = subprocess.run([exe, tmp_l, str(w), str(h), str(B), tmp_r, str(CAP), reps], capture_output=True,
                                         text=True, check=True).stdout.split()
                    if int(out[1]) != int(nv.sum()):
                        raise SystemExit(f"{case} {name}: device {nv.sum()} vertices, host chain {out[1]}")
                    cpu_ms = float(out[3])
                lines.append(f"{case:>6} {name:>8} {B:>5} {min_area:>8} {dev:>10.4f} {min(ts):>8.4f} {max(ts):>8.4f} "
                             f"{np.median(kerns):>10.4f} {d2h:>8.4f} {cpu_ms:>10.2f} {(d2h + cpu_ms) / dev:>16.2f} "
                             f"{int(nkept.sum()):>8} {int(nv.sum()):>8}")
                print(lines[-1], flush=True)
            for p in d.values():
                c.dev_free(p)
    for t in (tmp_l, tmp_r):
        if exe and os.path.exists(t):
            os.remove(t)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
