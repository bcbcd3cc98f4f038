"""CPU checks of the warp tests' exact-value probe (tests/test_warp_gpu.py): that it would notice a
warp whose coordinates are one 1/32-px unit off, that the observable it replaces would not, and
that its reference is the same under both CPU restatements.  No GPU needed.

The probe feeds k_warp_diff gray2 := the oracle's warped image of a uniform-noise source (+-1 on a
sparse set) at thresh 0, so each mask byte is an equality check of the warped value.  Here the numpy
restatement's warp_perspective is given a deliberately wrong coordinate (every pixel's rounded X or Y
moved by one unit) and the mask such a kernel would write is compared with the expected one.

Measured (this file prints the figures): over the probe's kinds at (132, 65) and (388, 200) and the
four one-unit offsets, the share of in-frame pixels whose mask byte changes for at least one of
the three sources is 0.990-1.000 (bar: 0.90).  The mask the other warp tests look at, |warped - gray2| > 190
on mdx_synth_pair frames, changes at 0.000-0.008 % of its bytes under the same offsets, i.e.
0-23 bytes of a 640 x 480 mask (bar: under 0.1 %).
"""
import numpy as np
import pytest

import np_reference as npr
import test_warp_gpu as wg

OFFSETS = [(1, 0), (-1, 0), (0, 1), (0, -1)]
SIZES = [(132, 65), (388, 200)]


def _inside(X, Y, w, h):
    sx, sy = X >> 5, Y >> 5
    return (sx >= 0) & (sx + 1 < w) & (sy >= 0) & (sy + 1 < h)


def test_probe_kinds_are_what_they_claim(mdx, oracle):
    """The new kinds reach what they are there for, under the oracle's own inverse."""
    for w, h in SIZES + [(68, 33)]:
        M = oracle.invert3x3(wg.probe_H(mdx, "w_zero", w, h)).ravel()
        xs = np.arange(w, dtype=np.float64)
        xb = (xs // 64) * 64
        for y in (0, h - 1):      # the reference's W = (M6 xb + M7 y + M8) + M6 x1
            W = (M[6] * xb + M[7] * y + M[8]) + M[6] * (xs - xb)
            assert (W == 0.0).any() and (W > 0).any() and (W < 0).any()
        M = oracle.invert3x3(wg.probe_H(mdx, "neg_w", w, h)).ravel()
        ys, xs = np.mgrid[0:h, 0:w]
        assert (M[6] * xs + M[7] * ys + M[8] < 0).all()
        M = oracle.invert3x3(wg.probe_H(mdx, "proj_y", w, h)).ravel()
        assert M[6] == 0.0 and M[7] != 0.0
        M = oracle.invert3x3(wg.probe_H(mdx, "clamp", w, h)).ravel()
        fX = (M[0] * np.arange(w) + M[2]) * (32.0 / M[8])
        assert fX.min() < -2.0 ** 31 and M[6] == 0.0 and M[7] == 0.0
        X, _ = npr.warp_coords(w, h, M)
        assert X.min() == -2 ** 31
        if w > 72:      # INT_MAX from column 72 on
            assert fX.max() > 2.0 ** 31 and X.max() == 2 ** 31 - 1


@pytest.mark.parametrize("w,h", SIZES + [(150, 10), (131, 65)])
def test_probe_reference_same_in_both_restatements(mdx, oracle, w, h):
    """Every reference image the probe compares the kernel with: the C oracle and the numpy
    restatement agree byte for byte, the new kinds and the h < 16 blocking included."""
    cases = [(k, wg.probe_H(mdx, k, w, h)) for k in wg.PROBE_KINDS]
    if (w, h) == (388, 200):
        cases += [(f"random_projective_{i}", H) for i, H in enumerate(wg._random_projective())]
    for key, H in cases:
        Minv = oracle.invert3x3(H)
        for j in range(wg.NSRC):
            ref = wg.probe_ref(oracle, w, h, key, H, j)
            assert np.array_equal(ref, npr.warp_perspective(wg.probe_source(w, h, j), Minv)), (key, j)


@pytest.mark.parametrize("w,h", SIZES)
def test_probe_notices_a_one_unit_coordinate_error(mdx, oracle, w, h):
    """A warp whose every X (or Y) is one 1/32-px unit off changes the probe's mask, for at least one
    of the three sources, at >= 90 % of the pixels whose four taps lie inside the image for the true
    and the wrong coordinate (kinds with at least 100 such pixels)."""
    low = []
    for i, kind in enumerate(wg.PROBE_KINDS):
        H = wg.probe_H(mdx, kind, w, h)
        Minv = oracle.invert3x3(H)
        X, Y = npr.warp_coords(w, h, Minv)
        refs = [wg.probe_ref(oracle, w, h, kind, H, j) for j in range(wg.NSRC)]
        g2 = [wg.probe_gray2(refs[j], j, "sparse", 0, (w, h, i)) for j in range(wg.NSRC)]
        hit = np.zeros((h, w), int)
        for j in range(wg.NSRC):
            hit += g2[j] != refs[j]
        assert hit.max() <= 1 and hit.any()      # >= 2 of 3 sources check equality at every pixel
        for off in OFFSETS:
            inside = _inside(X, Y, w, h) & _inside(X + off[0], Y + off[1], w, h)
            seen = np.zeros((h, w), bool)
            for j in range(wg.NSRC):
                wrong = npr.warp_perspective(wg.probe_source(w, h, j), Minv, offset=off)
                seen |= wg.probe_expected(wrong, g2[j], 0) != wg.probe_expected(refs[j], g2[j], 0)
            n = int(inside.sum())
            share = float(seen[inside].mean()) if n else float("nan")
            print(f"probe sensitivity {w}x{h} {kind} offset {off}: {share:.4f} of {n} in-frame pixels")
            if n >= 100 and share < 0.90:
                low.append((kind, off, n, share))
    assert not low, low


@pytest.mark.parametrize("w,h", [(640, 480), (132, 65)])
def test_threshold_190_mask_does_not_notice(mdx, oracle, w, h):
    """Why the probe exists: the same one-unit error changes under 0.1 % of the bytes of the mask
    the other warp tests compare (|warped - gray2| > 190 on the synthetic pair)."""
    a, b, Ht = mdx.synth_pair(510, w, h, 1)
    for kind in ("true", "projective"):
        Minv = oracle.invert3x3(wg._H(kind, w, h, Ht))
        mask = wg.probe_expected(npr.warp_perspective(a, Minv), b, 190)
        assert np.array_equal(mask, wg.probe_expected(oracle.warp_perspective(a, Minv), b, 190))
        for off in OFFSETS:
            wrong = wg.probe_expected(npr.warp_perspective(a, Minv, offset=off), b, 190)
            changed = int((wrong != mask).sum())
            print(f"mask@190 {w}x{h} {kind} offset {off}: {changed} of {w * h} bytes change "
                  f"({100.0 * changed / (w * h):.4f} %)")
            assert changed < 0.001 * w * h, (kind, off, changed)
