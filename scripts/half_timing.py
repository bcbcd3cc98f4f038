#!/usr/bin/env python3
"""Time k_half (half-size ingest) by HIP events, beside a device-to-device copy of the
same byte total, and one mdx_ring_push_half against one mdx_ring_push.

    python scripts/half_timing.py [--out profiles/half_timing.txt] [--device 0]

Kernel cases: 1 x 1080p, 32 x 1080p and 32 x 4K rgb8 frames at their packed pitch (a multiple of 4: the
vector path), one mdx_resize_half_dev call (one launch) between two events on the context's stream;
median of 20 timed calls after 20 untimed ones; a 512 MB device copy queued in front of the first event
keeps host time out of the interval and the frames out of the caches.  Bytes: source plus destination.  The copy: one
hipMemcpyAsync, device to device, of half that total (so that it reads and writes the same total),
timed the same way in the same process.  The same frames at a pitch one byte longer take the byte path.
Ring: wall time from the call to the return of mdx_sync for one 1080p rgb8 frame in page-locked memory,
median of 20 after 5, mdx_ring_push_half (ring of 960 x 540) and mdx_ring_push (ring of 1920 x 1080).

Every device step is a child process of its own under `timeout`, and the first one that fails ends the
run (the steps are chained as with &&).
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((1, 1920, 1080), (32, 1920, 1080), (32, 3840, 2160))     # (batch, w, h), rgb8
WARMUP, REPS = 20, 20
PEAK = 8e12                 # bytes per second the fraction is quoted against
BUSY = 512 << 20            # bytes of the copy queued in front of every timed interval
STEP_TIMEOUT = 240          # seconds per device step


def _hip():
    L = C.CDLL("libamdhip64.so")
    vp = C.c_void_p
    L.hipEventCreate.argtypes = [C.POINTER(vp)]
    L.hipEventRecord.argtypes = [vp, vp]
    L.hipEventSynchronize.argtypes = [vp]
    L.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
    L.hipEventDestroy.argtypes = [vp]
    L.hipMemcpyAsync.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
    return L


def timed(hip, stream, fn, busy):
    """Median, min and max ms of fn() between two events on the stream, REPS calls after WARMUP.  busy()
    queues device work in front of the first event, so that fn()'s work is queued before that event
    completes: the interval holds no host time, and the caches hold none of fn()'s data."""
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    ts = []
    for it in range(WARMUP + REPS):
        busy()
        assert hip.hipEventRecord(e0, stream) == 0
        fn()
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        if it >= WARMUP:
            ts.append(ms.value)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    return float(np.median(ts)), min(ts), max(ts)


def kernel_step(batch, w, h, device):
    import motion_detection_amd as m
    hip = _hip()
    dw, dh = m.half_size(w, h)
    out = {}
    with m.Context(device, 64, 64, 1) as ctx:
        pre = [ctx.dev_alloc(BUSY), ctx.dev_alloc(BUSY)]
        busy = lambda: hip.hipMemcpyAsync(pre[1], pre[0], BUSY, 3, ctx.stream)   # noqa: E731
        for name, pad in (("vector", 0), ("byte", 1)):
            stride, dstride = 3 * w + pad, 3 * dw + pad
            sbytes, dbytes = stride * h * batch, dstride * dh * batch
            src, dst = ctx.dev_alloc(sbytes), ctx.dev_alloc(dbytes)
            rng = np.random.default_rng(w + batch)
            one = rng.integers(0, 256, stride * h, dtype=np.uint8)
            for b in range(batch):
                ctx.h2d(src + b * stride * h, one)
            k = timed(hip, ctx.stream, lambda: ctx.resize_half_dev(batch, src, w, h, stride, stride * h, 3, dst, dstride,
                                                                   dstride * dh), busy)
            total = 3 * w * h * batch + 3 * dw * dh * batch          # the bytes the kernel touches
            out[name] = dict(ms=k[0], min=k[1], max=k[2], bytes=total)
            if name == "vector":
                half = total // 2
                a, b2 = ctx.dev_alloc(half), ctx.dev_alloc(half)
                c = timed(hip, ctx.stream, lambda: hip.hipMemcpyAsync(b2, a, half, 3, ctx.stream), busy)
                out["copy"] = dict(ms=c[0], min=c[1], max=c[2], bytes=2 * half)
                ctx.dev_free(a)
                ctx.dev_free(b2)
            ctx.dev_free(src)
            ctx.dev_free(dst)
    info = m._lib.build_info()
    print(json.dumps(dict(batch=batch, w=w, h=h, sha=info["src_sha256"], matches=info["matches_tree"], **out)))


def ring_step(device):
    import motion_detection_amd as m
    w, h = 1920, 1080
    frame = m.host_empty((h, w, 3))
    frame[...] = np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8)
    out = {}
    for name, half in (("half", True), ("full", False)):
        with m.Context(device, w, h, 1) as ctx:
            ts = []
            for it in range(5 + REPS):
                t0 = time.perf_counter()
                ctx.ring_push(frame, 5, half=half)
                ctx.sync()
                t1 = time.perf_counter()
                if it >= 5:
                    ts.append((t1 - t0) * 1e3)
            out[name] = dict(ms=float(np.median(ts)), min=min(ts), max=max(ts))
    print(json.dumps(out))


def run_step(args, *step):
    cmd = [sys.executable, os.path.abspath(__file__), "--device", str(args.device), "--step"] + [str(s) for s in step]
    p = subprocess.run(["timeout", "-k", "10", str(STEP_TIMEOUT)] + cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit(f"device step {step} ended with {p.returncode}; nothing more is run\n" + p.stdout[-2000:]
                         + p.stderr[-2000:])
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "half_timing.txt"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--step", nargs="+", help="(internal) one device step: `ring`, or batch w h")
    args = ap.parse_args()
    if args.step:
        if args.step[0] == "ring":
            ring_step(args.device)
        else:
            kernel_step(*[int(v) for v in args.step], args.device)
        return
    rows = [run_step(args, *c) for c in CASES]
    ring = run_step(args, "ring")
    gbs = lambda r: r["bytes"] / (r["ms"] * 1e-3)   # noqa: E731
    lines = [f"k_half (mdx_resize_half_dev, rgb8, one launch per call) by HIP events; library src_sha256 {rows[0]['sha']} "
             f"(matches tree: {rows[0]['matches']})",
             f"median of {REPS} calls after {WARMUP} untimed (min .. max); bytes: source + destination; of peak: of 8 TB/s; "
             f"copy: one device-to-device hipMemcpyAsync reading and writing the same byte total, same run; byte path: the "
             f"same frames at a pitch one byte longer",
             f"{'batch':>5} {'w':>5} {'h':>5} {'MB':>8} {'k_half ms':>10} {'min':>8} {'max':>8} {'TB/s':>6} {'of peak':>7} "
             f"{'copy ms':>8} {'TB/s':>6} {'k_half/copy rate':>16} {'byte path ms':>12}"]
    for r in rows:
        v, c, b = r["vector"], r["copy"], r["byte"]
        lines.append(f"{r['batch']:>5} {r['w']:>5} {r['h']:>5} {v['bytes'] / 1e6:>8.1f} {v['ms']:>10.4f} {v['min']:>8.4f} "
                     f"{v['max']:>8.4f} {gbs(v) / 1e12:>6.2f} {gbs(v) / PEAK:>7.0%} {c['ms']:>8.4f} {gbs(c) / 1e12:>6.2f} "
                     f"{gbs(v) / gbs(c):>16.2f} {b['ms']:>12.4f}")
    lines.append(f"one 1080p rgb8 frame from page-locked memory into the ring, wall ms from the call to mdx_sync's return, "
                 f"median of {REPS} after 5 (min .. max):")
    for name, label in (("half", "mdx_ring_push_half (ring of 960 x 540)"), ("full", "mdx_ring_push (ring of 1920 x 1080)")):
        r = ring[name]
        lines.append(f"  {label:<40} {r['ms']:.3f} ({r['min']:.3f} .. {r['max']:.3f})")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
