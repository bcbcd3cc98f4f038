"""k_lk_iter's row loop addressing (mdx_lk.hip): the union and J streams' descriptors advance row by
row (base up, size down: the shrinking size is the only clamp at the end of the class slab and of the
frame-2 pyramid), the lanes that must not fetch are masked by an offset outside every descriptor, and
each row's wait stands at its end.  Every case compares next_pts (as uint32) and status of every point
with the oracle, and H, the mask and num_vectors too; every output buffer is prefilled with 0xAA and
compared whole.

Shapes, the smallest where that addressing can go wrong:
 * 164 x 244 gray: the smallest width with three pyramid levels (41 x 61 at level 2).  The bottom grid
   row's windows end in the planes' last rows, and the last pair's are the last of the slab.  Run as one
   pair (the plain instantiations), as 16 pairs at pixel_step 10 (425 points: not a multiple of 16, so
   the levels run in sequence over several pairs) and as 16 pairs at pixel_step 16 (176 points: the
   level dataflow, the <.., true> instantiations).
 * 320 x 240, 16 pairs, at pixel_step 3 (many residue classes, union widths other than 56 and 112, a
   different partial last DMA piece) and at 10, on a pair whose motion bursts outwards from the centre:
   points leave the frame on all four sides (checked below from the oracle's exit reasons), so windows
   lie partly outside the level in rows and in columns, and iterations stop out of range.
Each shape runs once with the default bodies and once with MDX_LK_FMA=0 (the exact body everywhere).
That the three dataflow shapes do take the level dataflow is shown by its fault injection
(MDX_LK_SPIN_MAX=-1, as tests/test_bench_path_gpu.py uses it): every gate gives up and every level below
the coarsest is recomputed, which can only happen where the dataflow launches ran; the other shapes'
counts stay zero under it.  Without it, every count is zero.
"""
import functools

import numpy as np
import pytest

import hostile_frames as hf
from oracle_check import NO_FALLBACKS, assert_batch_equals_oracle, lk_env, run_batch, without

pytestmark = pytest.mark.gpu

# name -> (w, h, pixel_step, batch)
SHAPES = {
    "164x244_one": (164, 244, 10, 1),
    "164x244_x16_seq": (164, 244, 10, 16),
    "164x244_x16_flow": (164, 244, 16, 16),
    "320x240_x16_ps3": (320, 240, 3, 16),
    "320x240_x16_ps10": (320, 240, 10, 16),
}
NPAIRS = 4            # distinct pairs; slot i of a batch holds pair i % NPAIRS
NLEV = 3              # both frame sizes: levels 0 .. 2


def burst_pair(w, h, zoom, seed):
    """A texture over the smooth low-frequency pattern (hostile_frames), and the same scene magnified
    by `zoom` about the centre: every point moves outwards, the border points past the frame."""
    a = 0.5 * hf.texture(w, h, seed).astype(np.float64) + 0.5 * hf.smooth(w, h).astype(np.float64)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    cx, cy = (w - 1) / 2, (h - 1) / 2
    sx, sy = cx + (x - cx) / zoom, cy + (y - cy) / zoom      # inside the frame for zoom >= 1
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    fx, fy = sx - x0, sy - y0
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    b = ((1 - fx) * (1 - fy) * a[y0, x0] + fx * (1 - fy) * a[y0, x1] + (1 - fx) * fy * a[y1, x0]
         + fx * fy * a[y1, x1])
    u8 = lambda v: np.ascontiguousarray(np.clip(np.rint(v), 0, 255).astype(np.uint8))  # noqa: E731
    return u8(a), u8(b)


@functools.lru_cache(maxsize=None)
def _pairs(w, h):
    return [burst_pair(w, h, 1.2 + 0.02 * i, 31 + i) for i in range(NPAIRS)]


@functools.lru_cache(maxsize=None)
def _refs(w, h, ps):
    """The oracle's results of the NPAIRS pairs, computed once per (frame size, pixel_step)."""
    from oracle import pyoracle
    return [pyoracle.calculate_optical_flow(a, b, nthreads=8, pixel_step=ps, min_vector_size=1.0, why=True)
            for a, b in _pairs(w, h)]


CALLS = 2             # per _run


def _run(mdx, w, h, ps, batch):
    """The batch entry (call pipelining on, as the bench path has it), CALLS times, every output
    prefilled with 0xAA before each call."""
    pairs = _pairs(w, h)
    g1 = np.stack([pairs[i % NPAIRS][0] for i in range(batch)])
    g2 = np.stack([pairs[i % NPAIRS][1] for i in range(batch)])
    return run_batch(mdx, g1, g2, create=dict(pixel_step=ps, min_vector_size=1.0, call_pipelining=1), vectors=False,
                     calls=CALLS)


def _compare(got, refs, batch, label):
    assert_batch_equals_oracle(got, [refs[i % NPAIRS] for i in range(batch)], label, fields=without("vectors"))


@pytest.mark.parametrize("fma", ["1", "0"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_rowloop_addressing(mdx, oracle, monkeypatch, shape, fma):
    w, h, ps, batch = SHAPES[shape]
    n = mdx.grid_count(w, h, ps)
    if shape.endswith("_seq"):
        assert n % 16 != 0                       # the dataflow's condition fails: levels in sequence
    elif batch >= 16:
        assert n % 16 == 0 and batch % 8 == 0    # the dataflow's conditions hold
    lk_env(monkeypatch, fma=fma)
    got = _run(mdx, w, h, ps, batch)
    assert got["fallbacks"] == NO_FALLBACKS, got["fallbacks"]
    _compare(got, _refs(w, h, ps), batch, f"{shape} fma={fma}")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_which_shapes_take_the_dataflow(mdx, oracle, monkeypatch, shape):
    """With every dataflow wait and gate made to give up at once (MDX_LK_SPIN_MAX=-1, read at mdx_create),
    a shape whose launches are the dataflow's (k_lk_iter<.., true>, gates, recompute launches) counts
    one gate give-up and one recomputed level per level below the coarsest and call; a shape whose
    levels run in sequence counts nothing.  Bit-exact either way."""
    w, h, ps, batch = SHAPES[shape]
    flow = batch >= 16 and not shape.endswith("_seq")
    lk_env(monkeypatch, spin_max="-1")
    got = _run(mdx, w, h, ps, batch)
    print(shape, "fallbacks", got["fallbacks"])
    if flow:
        assert got["fallbacks"]["gate_giveups"] == CALLS * (NLEV - 1), got["fallbacks"]
        assert got["fallbacks"]["levels_recomputed"] == CALLS * (NLEV - 1), got["fallbacks"]
    else:
        assert got["fallbacks"] == NO_FALLBACKS, got["fallbacks"]
    _compare(got, _refs(w, h, ps), batch, f"{shape} spin -1")


@pytest.mark.parametrize("ps", [3, 10])
def test_burst_pair_leaves_on_all_four_sides(oracle, ps):
    """The 320 x 240 pairs do their job: on each of them, at both steps, points stop out of range beyond
    the left, right, top and bottom edge, before the first iteration and in mid-iteration; some fail
    the final level-0 check; and some windows reach a level's last row or column (tainted)."""
    w, h = 320, 240
    first = mid = final = taint = 0
    for i, r in enumerate(_refs(w, h, ps)):
        why, p = r["why"], r["next_pts"]
        oor = (why & oracle.WHY_OUT_OF_RANGE) != 0
        sides = [int((oor & m).sum()) for m in (p[:, 0] < 0, p[:, 0] >= w, p[:, 1] < 0, p[:, 1] >= h)]
        print(f"ps {ps} pair {i}: {why.size} points, out of range {int(oor.sum())}, left/right/top/bottom {sides}")
        assert min(sides) > 0, (ps, i, sides)
        bit = {name: b for b, name in oracle.WHY_NAMES.items()}
        first += int(((why & bit["next_oor_first"]) != 0).sum())
        mid += int(((why & bit["next_oor_iter"]) != 0).sum())
        final += int(((why & bit["final_oor"]) != 0).sum())
        taint += int(((why & oracle.WHY_TAINT) != 0).sum())
    print(f"ps {ps}: first {first}, mid-iteration {mid}, final check {final}, tainted {taint}")
    assert first > 0 and mid > 0 and final > 0 and taint > 0
