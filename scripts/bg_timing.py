#!/usr/bin/env python3
"""Time background subtraction (mdx_bg_apply_dev, mdx_bg_image_dev, the getMotionContours chain) at 1920 x 1080 rgb8.

    python scripts/bg_timing.py [--out profiles/bg_timing.txt] [--device 0] [--streams 1,8] [--no-cpu]

Input: a noisy static scene (+-3 per byte) with a 96 x 96 bright patch moving 7 px a frame, as a pool of 32 frames per
stream (stream s starts 4 * s frames into it), resident on the device.  Every model first takes the pool 19 times round
(608 frames, T = 32), so the timed frames are frames 609+: the steady state, alphaT = 1 / 500.
Rows:
  apply T   32 frames as 32 / T calls of T frames, between two HIP events on the context's stream, per frame; median,
            min and max of 10 rounds, the three T's taking turns inside every round, each on the same 32 frames
  bytes     what one frame of that launch moves per pixel, from the model's own `modes` after the run: the count byte,
            modes * 4 * (2 + channels) of state read, 4 * modes of weights and one slot's 4 * (1 + channels) of mean and
            variance written (the fitted slot; the figure is a LOWER BOUND: slots rewritten by swaps and new modes add), all of it once per launch,
            hence / T; plus the frame's 3 bytes and the mask byte
  of 8 TB/s those bytes over the time, as a share of the datasheet rate; of copy: the time of a device copy moving the
            same bytes (half read, half written; torch copy_ between two events, same run) over the time
  image     mdx_bg_image_dev, the same way
  chain     mdx_bg_apply_dev (T = 1) -> mdx_mask_regions_dev(OPEN3) -> mdx_region_parents_dev ->
            mdx_region_outlines_dev per frame, between two events (stream 0 of a one-stream model)
  cpu       scripts/micro/bg_cpu.cpp: tests/bg_check.cpp's loop -- a restatement of the same contract, NOT OpenCV -- on
            the same pool after the same 19 rounds of it (608 frames), g++ -O2 -ffp-contract=off, one thread and 16
The report carries the library's src_sha256.
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, CN, POOL, WARM_ROUNDS, ROUNDS = 1920, 1080, 3, 32, 19, 10


def make_pool(seed=7):
    rng = np.random.default_rng(seed)
    base = rng.integers(40, 200, (H, W, CN)).astype(np.int16)
    pool = np.empty((POOL, H, W, CN), np.uint8)
    for t in range(POOL):
        f = base + rng.integers(-3, 4, (H, W, CN), dtype=np.int16)
        x, y = (7 * t) % (W - 96), 200 + 5 * t
        f[y:y + 96, x:x + 96] = 250
        pool[t] = np.clip(f, 0, 255).astype(np.uint8)
    return pool


def build_cpu():
    bindir = os.path.join(ROOT, "scripts", "micro", "bin")
    os.makedirs(bindir, exist_ok=True)
    exe = os.path.join(bindir, "bg_cpu")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-pthread", "-I", os.path.join(ROOT, "tests"),
                    os.path.join(ROOT, "scripts", "micro", "bg_cpu.cpp"), "-o", exe], check=True)
    return exe


def med(v):
    return float(np.median(v)), float(np.min(v)), float(np.max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bg_timing.txt"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--streams", default="1,8")
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch
    import motion_detection_amd as m
    info = m._lib.build_info()
    N, fb = W * H, W * H * CN
    pool = make_pool()
    lines = [f"background subtraction at {W} x {H} rgb8, defaults (5 mixtures, history 500), frames 609+ of a noisy static "
             f"scene with a moving patch; library src_sha256 {info['src_sha256']} (matches tree: {info['matches_tree']})",
             f"HIP events on the context stream; ms per frame (all streams together); median min max of {ROUNDS} rounds, "
             f"the variants taking turns in every round",
             f"{'row':>10} {'streams':>7} {'T':>3} {'ms/frame':>9} {'min':>8} {'max':>8} {'vs T=1':>7} {'B/px/frame':>10} "
             f"{'GB/s':>8} {'of 8 TB/s':>9} {'copy ms':>8} {'of copy':>7} {'modes/px':>8}"]
    L = m.lib()
    for S in (int(v) for v in args.streams.split(",")):
        with m.Context(args.device, W, H, 1) as c:
            stream = torch.cuda.ExternalStream(c.stream, device=args.device)
            d_frames, d_mask, d_img = c.dev_alloc(S * POOL * fb), c.dev_alloc(S * POOL * N), c.dev_alloc(S * fb)
            for s in range(S):
                c.h2d(d_frames + s * POOL * fb, np.roll(pool, -4 * s, axis=0))
            bg = c.bg_create(S, W, H, CN)

            def run(T):
                for t0 in range(0, POOL, T):
                    c.bg_apply_dev(bg, T, d_frames + t0 * fb, W * CN, fb, POOL * fb, -1.0,
                                   d_mask + t0 * N)

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                c.sync()
                return e0.elapsed_time(e1)
            # the mask of a T-frame call is [streams][T][h][w]: with T < POOL each call's masks get their own slot
            for _ in range(WARM_ROUNDS):
                c.bg_apply_dev(bg, POOL, d_frames, W * CN, fb, POOL * fb, -1.0, d_mask)
            c.sync()
            times = {1: [], 8: [], 32: [], "image": []}
            for _ in range(ROUNDS):
                for T in (1, 8, 32):
                    times[T].append(timed(lambda: run(T)) / POOL)
                times["image"].append(timed(lambda: c.bg_image_dev(bg, d_img)))
            modes = np.empty((H, W), np.uint8)
            c._check(L.mdx_bg_get_state(c._h, C.c_void_p(bg), 0, None, None, None, modes.ctypes.data_as(C.c_void_p), None))
            mean_modes = float(modes.mean())
            base_ms = med(times[1])[0]
            for T in (1, 8, 32):
                per_launch = 1 + mean_modes * 4 * (2 + CN) + 4 * mean_modes + 4 * (1 + CN)
                bpp = per_launch / T + CN + 1
                total = bpp * N * S
                src = torch.empty(int(total / 2), dtype=torch.uint8, device=f"cuda:{args.device}")
                dst = torch.empty_like(src)
                with torch.cuda.stream(stream):
                    for _ in range(3):
                        dst.copy_(src)
                    cp = []
                    for _ in range(ROUNDS):
                        cp.append(timed(lambda: dst.copy_(src)))
                del src, dst
                ms, lo, hi = med(times[T])
                gbs = total / ms / 1e6
                lines.append(f"{'apply':>10} {S:>7} {T:>3} {ms:>9.4f} {lo:>8.4f} {hi:>8.4f} {ms / base_ms:>7.3f} {bpp:>10.2f} "
                             f"{gbs:>8.1f} {gbs / 8000:>9.3f} {med(cp)[0]:>8.4f} {med(cp)[0] / ms:>7.3f} {mean_modes:>8.3f}")
            ms, lo, hi = med(times["image"])
            bpp = 1 + 4 * (1 + CN) + CN     # the count, the first mode's weight and mean (it holds > 0.9), the pixel
            lines.append(f"{'image':>10} {S:>7} {'':>3} {ms:>9.4f} {lo:>8.4f} {hi:>8.4f} {'':>7} {bpp:>10.2f} "
                         f"{bpp * N * S / ms / 1e6:>8.1f} {bpp * N * S / ms / 1e6 / 8000:>9.3f}")
            if S == 1:
                cap, maxp = 4096, N // 2
                d = dict(labels=c.dev_alloc(4 * N), regs=c.dev_alloc(32 * cap), ext=c.dev_alloc(32 * cap), cnt=c.dev_alloc(16),
                         off=c.dev_alloc(4 * (cap + 1)), xy=c.dev_alloc(8 * maxp))

                def chain(t):
                    c.bg_apply_dev(bg, 1, d_frames + t * fb, W * CN, fb, 0, -1.0, d_mask)
                    c.mask_regions_dev(1, d_mask, W, H, W, N, True, 50, d["regs"], cap, d["cnt"], d["cnt"] + 4, d["labels"])
                    c.region_parents_dev(1, d["labels"], W, H, d["regs"], cap, d["cnt"] + 4, 0, d["ext"], d["cnt"] + 8)
                    c.region_outlines_dev(1, d["labels"], W, H, d["ext"], cap, d["cnt"] + 8, d["off"], d["xy"], maxp,
                                          d["cnt"] + 12)
                for t in range(3):
                    chain(t)
                ch = [timed(lambda: chain(t)) for t in range(POOL)]
                cnt = np.zeros(4, np.int32)
                c.d2h(cnt, d["cnt"])
                c.sync()
                ms, lo, hi = med(ch)
                lines.append(f"{'chain':>10} {S:>7} {1:>3} {ms:>9.4f} {lo:>8.4f} {hi:>8.4f}   (min_area 50; the last frame: "
                             f"{cnt[0]} components, {cnt[1]} kept, {cnt[2]} external, {cnt[3]} outline points)")
            c.sync()
            c.bg_destroy(bg)
    if not args.no_cpu:
        exe = build_cpu()
        path = os.path.join(ROOT, "scripts", "micro", "bin", "bg_frames.u8")
        pool.tofile(path)
        try:
            out = subprocess.run([exe, path, str(W), str(H), str(CN), str(POOL), str(WARM_ROUNDS), "16"], check=True, capture_output=True,
                                 text=True).stdout.split("\n")
        finally:
            os.remove(path)
        sums = set()
        for ln in out:
            if ln.strip():
                nt, ms, sm = ln.split()
                sums.add(sm)
                lines.append(f"{'cpu':>10} {1:>7} {1:>3} {float(ms):>9.3f}   restatement (tests/bg_check.cpp, not OpenCV), {nt} "
                             f"thread(s), frames 609+")
        assert len(sums) == 1, sums
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
