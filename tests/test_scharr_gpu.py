"""GPU parity of the derivative planes alone: every padded level of the Scharr planes that
k_scharr_levels leaves in HBM equals the oracle's calcSharrDeriv planes word for word, the
CONSTANT-0 border included (lkpyramid.cpp buildOpticalFlowPyramid withDerivatives: calcSharrDeriv
into a copyMakeBorder ... BORDER_CONSTANT buffer; reference call at optical_flow_calculator.cpp:71).

flow_trajectory of three frames builds whole planes of both pairs in one k_scharr_levels launch and
leaves them in the context's derivative buffer.  The per-level launches of the class-plane LK
(k_scharr, rows [vlo, vhi + 1) only) and the fused class kernel (k_lk_class_fused, derivatives
never stored) are not compared here: their planes are partial or absent.  All three apply the one
per-pixel stencil (scharr_word, mdx_dev.h) this test pins, and their own indexing stays covered by
the bit-exact next_pts of test_parity_gpu.py (at pixel_step 10, levels >= 3 take k_scharr and
levels 0-2 the fused kernel).
"""
import numpy as np
import pytest

from test_pyramid_gpu import KPAD, KWIN, KXOFF, frames, geometry

pytestmark = pytest.mark.gpu


def der_planes(der, levels, pair, der_words):
    """A pair's padded (h + 80) x (w + 80) derivative words per level.  Layout (make_geometry): a
    level's word offset in the pair's slab equals its byte offset in the image slab, with the same
    pitch; pairs are der_words apart."""
    out = []
    for sw, sh, pitch, off in levels:
        base = pair * der_words + off
        a = der[base:base + pitch * (sh + 2 * KPAD)].reshape(sh + 2 * KPAD, pitch)
        out.append(a[:, KXOFF - KPAD:KXOFF + sw + KPAD])
    return out


# 81x83: two levels, the smallest frame with a level 1.  333x241 rgb8: three levels, widths that are
# no multiples of 4, so the last chunk's px < L.w edge runs.
@pytest.mark.parametrize("w,h,ch,seed", [(81, 83, 1, 21), (333, 241, 3, 22)])
def test_scharr_levels_planes(mdx, oracle, w, h, ch, seed):
    a, b = frames(w, h, ch, seed)
    c3 = np.roll(b, (-1, 4), (0, 1))
    with mdx.Context(0, w, h, 1) as c:
        c.flow_trajectory([a, b, c3])
        c.sync()
        levels, _ = geometry(w, h, c.params.max_level)
        total = sum(pitch * (sh + 2 * KPAD) for _, sh, pitch, _ in levels)
        der_words = (total + 63) // 64 * 64
        der = np.empty(2 * der_words, np.uint32)
        assert mdx.lib().mdx_debug_copy(c._h, 4, der.ctypes.data, der.nbytes) == 0
        for pair, first in enumerate((a, b)):
            got = der_planes(der, levels, pair, der_words)
            _, _, ref = oracle.build_pyramid(oracle.to_gray(first), KWIN, c.params.max_level, with_deriv=True)
            assert len(ref) == len(got) == len(levels), (len(ref), len(got))
            for lv, (g, r) in enumerate(zip(got, ref)):
                r = np.ascontiguousarray(r).view(np.uint32)[..., 0]   # (Ix int16 | Iy int16 << 16)
                assert r.shape == g.shape, (r.shape, g.shape)
                bad = np.argwhere(g != r)
                assert bad.size == 0, f"pair {pair} level {lv}: {len(bad)} words differ, first {bad[:4]}"
