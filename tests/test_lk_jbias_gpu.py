"""k_lk_iter's J - I by mantissa bias (lk_jd512, mdx_plan.h; the class planes' C word carries the float
bias 0x4B400000) at both ends of its range, against the oracle bit for bit.

Frames are 200x160 gray at pixel_step 10, the shape of test_lk_fma_gpu.py: the smallest frame that puts
level 1 on k_lk_iter<4, 56> and level 0 on k_lk_iter<8, 112>; two levels, 320 grid points.  Frame 1 is
the 0/255 board of 8-pixel blocks and frame 2 its photographic negative (as it stands, moved 3 px in x,
moved 3 px in y), so (J - I) * 32 sits at +-8160; a fourth case is the smooth pair of test_lk_fma_gpu.py
(seed 11), whose small |J - I| put x near 0 and just below multiples of 512 on either side.  Every case
runs with the default body choice and with MDX_LK_FMA=0, as batch 1 (levels in sequence, the DF = false
kernels) and as batch 16 with call pipelining (the dataflow kernels, DF = true), and next_pts (as
uint32), status, num_vectors, H (as uint64) and the mask are compared with the oracle's.

So that no case passes on points that never iterate, the oracle's own result must leave at least 250 of
the 320 points of each negative case away from their grid position (CPU oracle: 259, 320 and 320, status
1 on all 320 in every case).
"""
import functools

import numpy as np
import pytest

from lk_scenes import PS, H, W, board, smooth_pair
from oracle_check import assert_batch_equals_oracle, lk_env, run_batch, without

pytestmark = pytest.mark.gpu

CASES = ("negative", "negative_dx3", "negative_dy3", "smooth")


@functools.lru_cache(maxsize=None)
def _pair(name):
    if name == "smooth":
        return smooth_pair(11)
    b = board()
    a = np.ascontiguousarray(b[:H, :W])
    moved = {"negative": b[:H, :W], "negative_dx3": b[:H, 3:3 + W], "negative_dy3": b[3:3 + H, :W]}[name]
    return a, np.ascontiguousarray(255 - moved)


@functools.lru_cache(maxsize=None)
def _ref(name):
    from oracle import pyoracle
    a, b = _pair(name)
    return pyoracle.calculate_optical_flow(a, b, pixel_step=PS, min_vector_size=1.0)


def _grid():
    """The grid points in point order (column major: pt = gx * ny + gy)."""
    nx, ny = (W + PS - 1) // PS, (H + PS - 1) // PS
    gx, gy = np.divmod(np.arange(nx * ny), ny)
    return np.stack([gx * PS, gy * PS], axis=1).astype(np.float32)


def _run(mdx, pair, batch, pipelined):
    return run_batch(mdx, np.stack([pair[0]] * batch), np.stack([pair[1]] * batch),
                     create=dict(pixel_step=PS, min_vector_size=1.0, call_pipelining=int(pipelined)), vectors=False,
                     calls=2 if pipelined else 1, back_to_back=True)


def _check(got, ref, label):
    assert_batch_equals_oracle(got, [ref] * len(got["num_vectors"]), label, fields=without("vectors"))


@pytest.mark.parametrize("name", CASES[:3])
def test_negative_cases_iterate(oracle, name):
    """The oracle's own result: the points of the negative cases move, so their windows went through the
    Newton iterations with J - I at the ends of its range."""
    ref = _ref(name)
    moved = int((ref["next_pts"] != _grid()).any(axis=1).sum())
    print(f"{name}: {moved} of {len(ref['status'])} points moved, status 1 on {int(ref['status'].sum())}")
    assert len(ref["status"]) == 320 and moved >= 250


@pytest.mark.parametrize("fma_env", ["1", "0"])
@pytest.mark.parametrize("name", CASES)
def test_bit_exact_vs_oracle(mdx, oracle, monkeypatch, name, fma_env):
    assert mdx.grid_count(W, H, PS) % 16 == 0                    # the dataflow's condition
    lk_env(monkeypatch, fma=fma_env)
    pair, ref = _pair(name), _ref(name)
    _check(_run(mdx, pair, 1, pipelined=False), ref, f"{name} fma={fma_env} batch 1")
    _check(_run(mdx, pair, 16, pipelined=True), ref, f"{name} fma={fma_env} batch 16")
