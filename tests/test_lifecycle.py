"""Context lifetime: create -> every entry family -> destroy, three times over.

The context owns about 45 device buffers, two pinned blocks, three streams and six event arrays
(csrc/mdx_ctx.h); a buffer that is freed twice, moved while a kernel still reads it or left behind by
mdx_destroy shows as a fault, a wrong result in a later cycle or a failing destroy.  Each cycle runs,
on 96x64 gray frames of the synthetic sequence (70 grid points; by the reference's rule -- the next
level must be larger than the 40-px window -- a single-level pyramid), on one context with
call_pipelining=1 and batch 16:

  a host pair call; two batched device calls of 16 pairs (one per pyramid half); a five-frame
  trajectory; six ring pushes with keep=5 (the sixth grows the ring, moving the five held slots) and
  the ring's trajectory; fit_subspace on that trajectory; cluster_euclidean on 300 points (two
  blocks); one band-flow + band-fit-warp pair on the upper half of the frame.

Every output of cycles 2 and 3 is byte-identical to cycle 1's; cycle 1's pair, batched, trajectory and
cluster outputs equal the oracle / the literal checker the families' own tests use; every
mdx_destroy returns MDX_OK, also right after create, with and without call_pipelining.

Not covered here, because a single-level pyramid never reaches them: the LK level loop below the
coarsest level, and the dataflow half of the launch descriptor (second iteration stream, flow / redo
events, retire counters).  test_bench_path_gpu.py and test_parity_gpu.py run those on multi-level frames.
"""
import ctypes as C
from contextlib import ExitStack

import numpy as np
import pytest

from motion_detection_amd import rowtile
from oracle_check import (OutputSet, assert_batch_equals_oracle, assert_pair_equals_oracle, assert_traj_equals_oracle,
                          uploaded)
from test_cluster import same as same_clusters, uniform_points, uniform_reference
from traj_seq import sequence

W, H, PS, B = 96, 64, 10, 16


def _bytes(*values):
    return b"".join(np.asarray(v).tobytes() for v in values)


def _destroy(mdx, c):
    rc = mdx.lib().mdx_destroy(c._h)
    c._h = None
    return rc


def _cycle(mdx, frames, slots):
    """One context's life.  Returns (outputs as bytes by name, the objects the oracle checks read)."""
    n = mdx.grid_count(W, H, PS)
    out, obj = {}, {}
    c = mdx.Context(0, W, H, B, pixel_step=PS, min_vector_size=1.0, call_pipelining=1)
    try:
        # host pair call
        obj["pair"] = r = c.flow_warp_diff(frames[0], frames[1])
        out["pair"] = _bytes(r.next_pts, r.status, r.vectors, r.mask, r.H, r.num_vectors)

        # two batched device calls back to back, one per pyramid half
        dev = []
        with ExitStack() as stack:
            outs = []
            for sl in slots:
                d1, d2 = stack.enter_context(uploaded(c, np.stack([frames[s] for s in sl]),
                                                      np.stack([frames[s + 1] for s in sl])))
                outs.append(stack.enter_context(OutputSet(c, B, W, H, n)))
                outs[-1].prefill()
                outs[-1].call(d1, d2)
            c.sync()
            obj["batch"] = [o.read() for o in outs]
        for j, got in enumerate(obj["batch"]):
            out[f"batch{j}"] = _bytes(*(got[k] for k in sorted(got)))

        # trajectories: the list entry, then the ring (six pushes, five kept)
        def traj_bytes(t):
            return _bytes(t.traj, t.traj_len, t.start_pts, t.vectors, t.num_vectors)
        obj["traj"] = c.flow_trajectory(frames[:5])
        out["traj"] = traj_bytes(obj["traj"])
        for k, f in enumerate(frames[:6]):
            assert c.ring_push(f, 5) == min(k + 1, 5)
        obj["ring"] = c.ring_trajectory(W, H, 5)
        out["ring"] = traj_bytes(obj["ring"])

        # subspace fit on the ring's trajectories, clustering on 300 points
        rng = mdx._lib.MdxRandState()
        mdx.lib().mdx_srand(C.byref(rng), 3)
        s = c.fit_subspace(obj["ring"].traj, 1, 0.5, rng)
        out["subspace"] = _bytes(s.columns, s.is_outlier, s.residuals, s.outlier_points)
        obj["cluster"] = k = c.cluster_euclidean(uniform_points(300), 20.0)
        out["cluster"] = _bytes(k.labels, k.kept, k.rects, k.num_all, k.num_kept)

        # one row band: its flow, then its fit + warp from its own record
        y0, y1 = rowtile.band_rows(H, 2, 0)
        host = dict(np=np.zeros((n, 2), np.float32), st=np.zeros(n, np.uint8), vec=np.zeros((n, 4)),
                    cand=np.zeros(rowtile.BAND_CAND_BYTES, np.uint8), mask=np.zeros((y1 - y0, W), np.uint8),
                    H=np.zeros(9), num=np.zeros(1, np.int32))
        d = {name: c.dev_alloc(a.nbytes) for name, a in host.items()}
        d["f0"], d["f1"] = c.dev_alloc(frames[0].nbytes), c.dev_alloc(frames[1].nbytes)
        dev += list(d.values())
        for name, a in host.items():
            c.h2d(d[name], a)                      # rows outside the band are never written
        c.h2d(d["f0"], frames[0])
        c.h2d(d["f1"], frames[1])
        c.band_flow_dev(d["f0"], d["f1"], W, H, W, mdx.FMT_GRAY8, y0, y1, d["np"], d["st"], d["cand"], d["vec"])
        c.band_fit_warp_dev(1, d["cand"], y0, y1, d["mask"], d["H"], d["num"])
        c.sync()
        for name, a in host.items():
            c.d2h(a, d[name])
        out["band"] = _bytes(*(host[name] for name in sorted(host)))
        for p in dev:
            c.dev_free(p)
    except BaseException:
        c.close()
        raise
    assert _destroy(mdx, c) == mdx.MDX_OK
    return out, obj


@pytest.mark.gpu
def test_three_context_lifetimes_give_the_same_bytes(mdx, oracle):
    frames = sequence(mdx, oracle, W, H, 6, seed=23, channels=1)
    slots = [[i % 5 for i in range(B)], [(3 * i + 1) % 5 for i in range(B)]]

    for cp in (0, 1):                              # nothing but create and destroy
        c = mdx.Context(0, W, H, B, call_pipelining=cp)
        assert _destroy(mdx, c) == mdx.MDX_OK

    first, obj = _cycle(mdx, frames, slots)
    refs = [oracle.calculate_optical_flow(frames[s], frames[s + 1], pixel_step=PS, min_vector_size=1.0)
            for s in range(5)]
    assert_pair_equals_oracle(obj["pair"], refs[0], "host pair")
    for j, got in enumerate(obj["batch"]):
        assert_batch_equals_oracle(got, [refs[s] for s in slots[j]], f"batched call {j}")
    assert_traj_equals_oracle(obj["traj"], oracle.flow_trajectory(frames[:5], pixel_step=PS), "list entry")
    assert_traj_equals_oracle(obj["ring"], oracle.flow_trajectory(frames[1:6], pixel_step=PS), "ring")
    same_clusters(obj["cluster"], uniform_reference(300))

    for cycle in (2, 3):
        again, _ = _cycle(mdx, frames, slots)
        assert again.keys() == first.keys()
        for name in first:
            assert again[name] == first[name], f"cycle {cycle}: {name} differs from cycle 1"
