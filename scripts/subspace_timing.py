#!/usr/bin/env python3
"""Time mdx_fit_subspace, one library against another (a refactor's "not slower" check).

    python scripts/subspace_timing.py --parent PATH/libmdx.so [--rounds 3] [--out profiles/subspace_timing.txt]

Rows: both precisions x N = 20,736 (a 1080p grid at step 10) and 2,048 trajectories x the shapes
(T = 5, num_motions = 2) and (T = 9, num_motions = 4).  Per row: the wall time of one mdx_fit_subspace
call by host clock (the call ends in a stream synchronise; upload, the 50 host-side draws and the
readback included), generator re-seeded before every call so each call does the same work, median of
20 after 3 warm-ups.  The parent's library and this tree's alternate, each run in a fresh child
process (MDX_LIB_PATH) under its own time limit; the first child that fails ends the job.  Per side the
report gives the median of its runs' medians and their spread (max - min across its runs).  A row
passes when new <= parent + the parent's spread.  The report carries both libraries' src_sha256.
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

WARMUP, REPS = 3, 20
SIGMA = 0.5
ROWS = [(p, N, T, nm) for p in (0, 1) for N in (20736, 2048) for T, nm in ((5, 2), (9, 4))]
CHILD_TIMEOUT = 120


def trajectories(N, T):
    """Background under a per-frame similarity, one translating object (1 in 8), 2% erratic; 0.05 px noise."""
    rng = np.random.default_rng(N + T)
    p = rng.uniform([20, 20], [1900, 1060], (N, 2))
    out = np.zeros((N, T, 2))
    fg, bad = np.arange(N) % 8 == 0, np.arange(N) % 50 == 1
    for t in range(T):
        a = np.radians(0.4 * t)
        A = 1.01 ** t * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        out[:, t] = p @ A.T + np.array([2.5 * t, -1.2 * t])
        out[fg, t] = p[fg] + np.array([-6.0 * t, 4.0 * t])
        if t:
            out[bad, t] = p[bad] + rng.normal(0, 4.0, (int(bad.sum()), 2))
    return (out + rng.normal(0, 0.05, out.shape)).astype(np.float32)


def child(device):
    """Time every row on the library MDX_LIB_PATH names (or the tree's); one JSON line."""
    import motion_detection_amd as m
    from motion_detection_amd._lib import MdxRandState, lib
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rows = []
    with m.Context(device, 64, 64, 1) as ctx:
        for precision, N, T, nm in ROWS:
            ctx.set_params(subspace_precision=precision)
            traj = trajectories(N, T)
            cols, out = np.zeros(4 * nm, np.int32), np.zeros(N, np.uint8)
            res, pts, nout = np.zeros(N, np.float64), np.zeros((N, 2), np.float32), C.c_int(0)
            ps = MdxRandState()
            ts = []
            for it in range(WARMUP + REPS):
                lib().mdx_srand(C.byref(ps), 1)
                t0 = time.perf_counter()
                rc = lib().mdx_fit_subspace(ctx._h, vp(traj), N, T, nm, SIGMA, C.byref(ps), vp(cols), vp(out), vp(res),
                                            vp(pts), C.byref(nout))
                t1 = time.perf_counter()
                if rc != 0:
                    raise SystemExit(f"mdx_fit_subspace: {rc}")
                if it >= WARMUP:
                    ts.append((t1 - t0) * 1e3)
            if cols.min() < 0:
                raise SystemExit(f"no winner at precision {precision} N {N} T {T}")
            rows.append({"median": float(np.median(ts)), "min": min(ts), "max": max(ts), "outliers": nout.value,
                         "columns": cols.tolist()})
    print(json.dumps({"src_sha256": m._lib.build_info()["src_sha256"], "rows": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the parent commit's libmdx.so")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subspace_timing.txt"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.device)
    if not args.parent or args.rounds < 3:
        ap.error("--parent is required, and at least 3 rounds")
    from motion_detection_amd._lib import LIB_PATH
    sides = {"parent": os.path.abspath(args.parent), "new": LIB_PATH}
    runs = {"parent": [], "new": []}
    for rnd in range(args.rounds):
        for side, path in sides.items():
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--device", str(args.device)],
                               env=dict(os.environ, MDX_LIB_PATH=path), capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT)
            if p.returncode != 0:      # nothing more is started on the device
                raise SystemExit(f"round {rnd} {side}: exit {p.returncode}\n{p.stdout}\n{p.stderr}")
            runs[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(f"round {rnd} {side}: " + " ".join(f"{r['median']:.4f}" for r in runs[side][-1]["rows"]), flush=True)
    sha = {s: {r["src_sha256"] for r in runs[s]} for s in runs}
    if any(len(v) != 1 for v in sha.values()):
        raise SystemExit(f"a side changed its library between runs: {sha}")
    lines = [f"mdx_fit_subspace, parent library src_sha256 {sha['parent'].pop()} against new {sha['new'].pop()}",
             f"ms of one call by host clock (upload, host draws, kernels, readback; ends in a stream synchronise), "
             f"median of {REPS} after {WARMUP} warm-ups per run; {args.rounds} runs per side, alternating parent / new, "
             f"each in a fresh process; median and spread (max - min) of each side's run medians; "
             f"pass: new <= parent + parent's spread",
             f"{'mode':>4} {'N':>6} {'T':>3} {'nm':>3} {'parent ms':>10} {'spread':>8} {'new ms':>10} {'spread':>8} "
             f"{'new/parent':>10} {'verdict':>8}   parent runs | new runs"]
    ok = True
    for i, (precision, N, T, nm) in enumerate(ROWS):
        med = {s: [r["rows"][i]["median"] for r in runs[s]] for s in runs}
        same = {(r["rows"][i]["outliers"], tuple(r["rows"][i]["columns"])) for s in runs for r in runs[s]}
        if len(same) != 1:
            raise SystemExit(f"row {ROWS[i]}: the libraries' results differ: {same}")
        pm, nw = float(np.median(med["parent"])), float(np.median(med["new"]))
        ps, ns = max(med["parent"]) - min(med["parent"]), max(med["new"]) - min(med["new"])
        passed = nw <= pm + ps
        ok = ok and passed
        lines.append(f"{'F32' if precision else 'F64':>4} {N:>6} {T:>3} {nm:>3} {pm:>10.4f} {ps:>8.4f} {nw:>10.4f} {ns:>8.4f} "
                     f"{nw / pm:>10.3f} {'pass' if passed else 'SLOWER':>8}   "
                     + " ".join(f"{v:.4f}" for v in med["parent"]) + " | " + " ".join(f"{v:.4f}" for v in med["new"]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
