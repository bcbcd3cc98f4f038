"""GPU parity of the front end alone: every padded pyramid level the HIP path leaves in HBM
(k_front = gray + pad + level-1 pyrDown, then k_front's level mode for the coarser levels) equals
the oracle's buildOpticalFlowPyramid images byte for byte, borders included (lkpyramid.cpp:
buildOpticalFlowPyramid with BORDER_REFLECT_101, withDerivatives; reference call at
optical_flow_calculator.cpp:71).  Both the split-frame launch of the pair path (first frames,
then second frames) and the both-frames launch of the trajectory path are covered.

What is pinned: front_reach() restates the launch rule of k_front (band height by the LDS a band
needs, one-row bands for launches of few workgroups), and test_cases_reach_every_k_front asserts
that the cases below together run all nine k_front<band height, mode> kernels: band height 4 by the
164x244 batch of 32 (mono8 and rgb8; the coarser level steps in level mode), 2 by the 4864x164 pair
(two level steps, mono8 and rgb8) and by 4K's level 0, 1 by every other case up to 1080p -- at
1080p a band of 4 rows fits 32 KB of LDS, but one or two pairs are under 512 such bands, so they run
one-row bands -- and by the 12000x100 row, whose one-row band needs more than 64 KB of LDS.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KPAD, KXOFF, KWIN = 40, 64, 40


def geometry(w, h, max_level):
    levels, off = [], 0
    sw, sh = w, h
    for _ in range(max_level + 1):
        pitch = (KXOFF + sw + KPAD + 16 + 63) // 64 * 64
        rows = KPAD + sh + KPAD
        levels.append((sw, sh, pitch, off))
        off += pitch * rows
        sw, sh = (sw + 1) // 2, (sh + 1) // 2
        if sw <= KWIN or sh <= KWIN:
            break
    return levels, (off + 255) // 256 * 256


MONO, COLOR, LEVEL = "mono", "colour", "level"


def front_reach(w, h, ch, nz, max_level=5):
    """launch_front_bands' rule (mdx_front.hip) restated: the (band height, mode) of every level step
    of a w x h frame.  nz: frame sides per launch -- the batch on the pair path (first and second
    frames are launched separately), twice the pair count on the trajectory path."""
    levels, _ = geometry(w, h, max_level)
    last_chunk16 = lambda lw: (KXOFF + lw + KPAD - 1) // 16
    out = []
    for step in range(len(levels) - 1):
        lp = 16 * (last_chunk16(levels[step][0]) + 1)          # LDS bytes per staged source row
        lp1 = 16 * (last_chunk16(levels[step + 1][0]) + 1)     # ... per destination row of the row buffer
        lds_of = lambda rb: (2 * rb + 3) * lp + rb * lp1
        rb = 4 if lds_of(4) <= 32 * 1024 else 2 if lds_of(2) <= 64 * 1024 else 1
        h1 = levels[step + 1][1]
        if rb == 4 and nz * ((h1 + 3) // 4) < 512:
            rb = 1
        out.append((rb, LEVEL if step else (MONO if ch == 1 else COLOR)))
    return out


def padded_levels(slab, levels, pair, img_bytes):
    out = []
    for sw, sh, pitch, off in levels:
        base = pair * img_bytes + off
        a = slab[base:base + pitch * (sh + 2 * KPAD)].reshape(sh + 2 * KPAD, pitch)
        out.append(a[:, KXOFF - KPAD:KXOFF + sw + KPAD])
    return out


def frames(w, h, ch, seed):
    rng = np.random.default_rng(seed)
    shape = (h, w) if ch == 1 else (h, w, 3)
    a = rng.integers(0, 256, shape, dtype=np.uint8)
    b = np.roll(a, (3, -2), (0, 1))
    return a, b


def check(mdx, c, oracle, gray_frames, which_slabs, npairs):
    levels, img_bytes = geometry(gray_frames[0].shape[1], gray_frames[0].shape[0], c.params.max_level)
    for slab_id, frames_of_slab in which_slabs:
        slab = np.empty(img_bytes * npairs, np.uint8)
        mdx.lib().mdx_debug_copy(c._h, slab_id, slab.ctypes.data, slab.nbytes)
        for pair in range(npairs):
            got = padded_levels(slab, levels, pair, img_bytes)
            ml, ref, _ = oracle.build_pyramid(frames_of_slab[pair], KWIN, c.params.max_level, with_deriv=False)
            assert len(ref) == len(got), (len(ref), len(got))
            for lv, (g, r) in enumerate(zip(got, ref)):
                bad = np.argwhere(g != r)
                assert bad.size == 0, f"slab {slab_id} pair {pair} level {lv}: {len(bad)} bytes differ, first {bad[:4]}"


CASES = [
    (160, 120, 1, 1),
    (333, 241, 1, 2),
    (81, 83, 1, 3),
    (320, 240, 3, 4),
    (641, 483, 3, 5),
    (1920, 1080, 1, 6),
    (1921, 1081, 3, 7),
    (3840, 2160, 1, 8),
    (12000, 100, 1, 11),      # a 12K-wide row: one level-1 row per band, > 64 KB of LDS requested
    (4864, 164, 1, 12),       # band height 2 at both level steps (4864 -> 2432 -> 1216 wide)
    (4864, 164, 3, 13),
]
TRAJECTORY_CASES = [(333, 241, 1, 9), (1920, 1080, 3, 10)]
BATCH_CASES = [(640, 480, 3, 3), (1920, 1080, 1, 2), (164, 244, 1, 32), (164, 244, 3, 32)]


def test_front_reach_rule():
    """The rule on the shapes it is used for here, worked by hand from launch_front_bands."""
    assert front_reach(164, 244, 1, 32) == [(4, MONO), (4, LEVEL)]        # 3.7 KB bands; 32 * 31, 32 * 16 bands
    assert front_reach(164, 244, 3, 32) == [(4, COLOR), (4, LEVEL)]
    assert front_reach(4864, 164, 1, 1) == [(2, MONO), (2, LEVEL)]        # 4 rows: 63.4 KB, then 32.5 KB
    assert front_reach(333, 241, 1, 1)[:2] == [(1, MONO), (1, LEVEL)]     # 31 bands of 4 rows < 512
    assert front_reach(1920, 1080, 1, 1)[0] == (1, MONO)                  # 135 bands of 4 rows < 512
    assert front_reach(1920, 1080, 1, 2)[0] == (1, MONO) and front_reach(1920, 1080, 3, 2)[0] == (1, COLOR)   # 270 < 512
    assert front_reach(3840, 2160, 1, 1)[0] == (2, MONO)
    assert front_reach(12000, 100, 1, 1) == [(1, MONO)]


def test_cases_reach_every_k_front():
    reached = set()
    for w, h, ch, _ in CASES:
        reached.update(front_reach(w, h, ch, 1))
    for w, h, ch, _ in TRAJECTORY_CASES:
        reached.update(front_reach(w, h, ch, 2))
    for w, h, ch, B in BATCH_CASES:
        reached.update(front_reach(w, h, ch, B))
    assert reached == {(rb, m) for rb in (4, 2, 1) for m in (MONO, COLOR, LEVEL)}, sorted(reached)


@pytest.mark.parametrize("w,h,ch,seed", CASES)
def test_pair_path_pyramids(mdx, oracle, w, h, ch, seed):
    a, b = frames(w, h, ch, seed)
    with mdx.Context(0, w, h, 1) as c:
        c.flow_warp_diff(a, b)
        c.sync()
        g1, g2 = oracle.to_gray(a), oracle.to_gray(b)
        check(mdx, c, oracle, [g1], [(2, [g1]), (3, [g2])], 1)


@pytest.mark.parametrize("w,h,ch,seed", TRAJECTORY_CASES)
def test_trajectory_path_pyramids(mdx, oracle, w, h, ch, seed):
    a, b = frames(w, h, ch, seed)
    with mdx.Context(0, w, h, 1) as c:
        c.flow_trajectory([a, b])
        c.sync()
        g1, g2 = oracle.to_gray(a), oracle.to_gray(b)
        check(mdx, c, oracle, [g1], [(2, [g1]), (3, [g2])], 1)


@pytest.mark.parametrize("w,h,ch,B", BATCH_CASES)
def test_batch_path_pyramids(mdx, oracle, w, h, ch, B):
    """Batched device entry: one k_front launch per frame side over B pairs (pair index in the grid)."""
    pairs = [frames(w, h, ch, 100 + i) for i in range(B)]
    fmt = mdx.FMT_GRAY8 if ch == 1 else mdx.FMT_RGB8
    fb = w * h * ch
    with mdx.Context(0, w, h, B) as c:
        d1, d2 = c.dev_alloc(fb * B), c.dev_alloc(fb * B)
        try:
            c.h2d(d1, np.stack([p[0] for p in pairs]))
            c.h2d(d2, np.stack([p[1] for p in pairs]))
            c.flow_warp_diff_batch_dev(B, d1, d2, w, h, w * ch, fb, fmt)
            c.sync()
            g1 = [oracle.to_gray(p[0]) for p in pairs]
            g2 = [oracle.to_gray(p[1]) for p in pairs]
            check(mdx, c, oracle, g1, [(2, g1), (3, g2)], B)
        finally:
            c.dev_free(d1)
            c.dev_free(d2)
