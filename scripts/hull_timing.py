#!/usr/bin/env python3
"""Time mdx_cluster_hulls against a monotone chain on one host thread.

    python scripts/hull_timing.py [--out profiles/hull_timing.txt] [--device 0]

Shapes: one cluster of 256, 2,048, 20,736 and 262,144 uniform random members in 1920 x 1080; 300 clusters
of 64 members; and the 8192-column tail input ((x, -(x - 4096)^2) for x = 0..8190 under (8191, 10^8), whose
max-y candidates become removable one per simultaneous round, so k_hull's sequential tail finishes it).
Per shape: the wall time of one mdx_cluster_hulls call, grouping and copies included (median of 20 after 3
warm-ups), the device time of k_hull alone and of upload + kernel + readback by HIP events on the
context's stream (mdx_enable_timing: stages 3 and 6, median of 20 further calls), and the same members
through the host implementation below: cvRound, std::sort of (x, y), std::unique, Andrew's monotone chain
popping on cross <= 0 in int64 -- HOST_SRC, g++ -O2, one thread, built into scripts/micro/bin/, timed on
this machine's host inside the program (min of its repetitions), the members already grouped by cluster.
Both must produce the same vertex counts.  The report carries the library's src_sha256.
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

WARMUP, REPS = 3, 20

HOST_SRC = r"""
// hull_cpu <points.f32> <n> <members per cluster> <reps>: hulls of consecutive clusters, one thread
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>
typedef std::pair<int32_t, int32_t> P;
static long long cross(const P& o, const P& a, const P& b)
{
    return (long long)(a.first - o.first) * (b.second - o.second) - (long long)(a.second - o.second) * (b.first - o.first);
}
static size_t hull(const float* f, int m, std::vector<P>& p, std::vector<P>& h)
{
    p.resize(m);
    for (int i = 0; i < m; i++) p[i] = P((int32_t)std::lrint((double)f[2 * i]), (int32_t)std::lrint((double)f[2 * i + 1]));
    std::sort(p.begin(), p.end());
    p.erase(std::unique(p.begin(), p.end()), p.end());
    if (p.size() == 1) return 1;
    h.clear();
    for (int pass = 0; pass < 2; pass++) {
        const size_t base = h.size();
        for (size_t i = 0; i < p.size(); i++) {
            const P& q = pass ? p[i] : p[p.size() - 1 - i];
            while (h.size() >= base + 2 && cross(h[h.size() - 2], h[h.size() - 1], q) <= 0) h.pop_back();
            h.push_back(q);
        }
        h.pop_back();
    }
    return h.size();
}
int main(int argc, char** argv)
{
    if (argc < 5) return 2;
    const int n = std::atoi(argv[2]), m = std::atoi(argv[3]), reps = std::atoi(argv[4]);
    std::vector<float> f((size_t)2 * n);
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp || std::fread(f.data(), 4, f.size(), fp) != f.size()) return 1;
    std::fclose(fp);
    std::vector<P> p, h;
    double best = 1e30;
    size_t total = 0;
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        total = 0;
        for (int c = 0; c + m <= n; c += m) total += hull(f.data() + 2 * (size_t)c, m, p, h);
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
    src, exe = os.path.join(bindir, "hull_cpu.cpp"), os.path.join(bindir, "hull_cpu")
    with open(src, "w") as f:
        f.write(HOST_SRC)
    subprocess.run(["g++", "-O2", "-o", exe, src], check=True)
    return exe


def shapes():
    for n in (256, 2048, 20736, 262144):
        pts = np.random.default_rng(n).uniform(0, [1919, 1079], (n, 2)).astype(np.float32)
        yield f"1 x {n}", pts, n
    rng = np.random.default_rng(300)
    centre = rng.uniform(100, 1800, (300, 1, 2))
    yield "300 x 64", (centre + rng.normal(0, 30, (300, 64, 2))).astype(np.float32).reshape(-1, 2), 64
    x = np.arange(8191, dtype=np.int64)
    tail = np.concatenate([np.stack([x, -(x - 4096) ** 2], 1), [(8191, 10 ** 8)]]).astype(np.float32)
    yield "tail 8192", tail, len(tail)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hull_timing.txt"))
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import motion_detection_amd as m
    from motion_detection_amd._lib import lib
    exe = build_cpu()
    info = m._lib.build_info()
    lines = [f"mdx_cluster_hulls vs sort + monotone chain (one host thread, g++ -O2, this file's HOST_SRC); library "
             f"src_sha256 {info['src_sha256']} (matches tree: {info['matches_tree']})",
             f"device wall: ms of one call, grouping and copies included, median of {REPS} after {WARMUP} warm-ups; "
             f"k_hull and up+k+down: HIP events on the context's stream, median of {REPS} more calls; cpu: min of "
             f"its repetitions, members already grouped",
             f"{'shape':>12} {'members':>8} {'device ms':>10} {'min':>8} {'max':>8} {'k_hull ms':>10} {'up+k+down':>10} "
             f"{'cpu ms':>10} {'cpu/device':>10} {'vertices':>8}"]
    tmp = os.path.join(ROOT, "scripts", "micro", "bin", "hull_points.f32")
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    with m.Context(args.device, 64, 64, 1) as ctx:
        for name, pts, per in shapes():
            n = len(pts)
            k = n // per
            labels = np.repeat(np.arange(k, dtype=np.int32), per)
            ids = np.arange(k, dtype=np.int32)
            offsets = np.zeros(k + 1, np.int32)
            xy = np.zeros((n, 2), np.int32)
            total = C.c_int(0)
            def call():
                rc = lib().mdx_cluster_hulls(ctx._h, vp(pts), vp(labels), n, vp(ids), k, vp(offsets), vp(xy), n,
                                             C.byref(total))
                if rc != 0:
                    raise SystemExit(f"mdx_cluster_hulls: {rc}")
            ts = []
            for it in range(WARMUP + REPS):           # wall times with event recording off
                t0 = time.perf_counter()
                call()
                t1 = time.perf_counter()
                if it >= WARMUP:
                    ts.append((t1 - t0) * 1e3)
            kerns, wholes = [], []
            for it in range(REPS):                    # the same call again, one event set each
                ctx._check(lib().mdx_enable_timing(ctx._h, 1))
                call()
                kern, whole = C.c_float(0), C.c_float(0)
                ctx._check(lib().mdx_stage_ms(ctx._h, 3, C.byref(kern)))
                ctx._check(lib().mdx_stage_ms(ctx._h, 6, C.byref(whole)))
                if lib().mdx_timing_calls(ctx._h) != 1:
                    raise SystemExit("expected one timed call")
                kerns.append(kern.value)
                wholes.append(whole.value)
            ctx._check(lib().mdx_enable_timing(ctx._h, 0))
            pts.tofile(tmp)
            cpu_reps = REPS if n <= 20736 else 5
            out = subprocess.run([exe, tmp, str(n), str(per), str(cpu_reps)], capture_output=True, text=True,
                                 check=True).stdout.split()
            cpu_vertices, cpu_ms = int(out[1]), float(out[3])
            if cpu_vertices != total.value:
                raise SystemExit(f"{name}: device {total.value} vertices, host chain {cpu_vertices}")
            dev = float(np.median(ts))
            lines.append(f"{name:>12} {n:>8} {dev:>10.4f} {min(ts):>8.4f} {max(ts):>8.4f} {np.median(kerns):>10.4f} "
                         f"{np.median(wholes):>10.4f} {cpu_ms:>10.4f} {cpu_ms / dev:>10.2f} {total.value:>8}")
    os.remove(tmp)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
