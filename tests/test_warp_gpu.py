"""GPU parity of the fused warp + absdiff + threshold kernel (rows A8-A10) over the geometries
and thresholds its fast path special-cases, through the C-ABI entry `mdx_warp_diff_dev`.

Reference: common/src/optical_flow_calculator.cpp:124-127 (warpPerspective, absdiff,
threshold(., 190, 255, THRESH_BINARY)).  The checker is the oracle's warp_perspective
(OpenCV 2.4 WarpPerspectiveInvoker restated) + numpy absdiff/threshold; the bar is bit-exact.

Cases: frame widths that are / are not multiples of the 128-px tile (partial reference blocks),
band-edge rows, homographies whose 1/32-px coordinates fall exactly on rounding ties
(translation by 1/64 px), flips (M0 < 0), zoom in/out (footprint larger than the LDS staging
buffer -> general path), projective and singular M, and thresholds -1, 0, 10, 190, 254, 255, 300.

Two observables.  The older tests (test_warp_geometries, _thresholds, _4k_*, and the 1080p half of
_projective_random) compare the mask at thresh 190 on mdx_synth_pair frames: blurred frames whose
|warped - gray2| is almost never near 190, so that mask barely depends on the coordinates -- a warp
whose every X or Y is one 1/32-px unit off changes 0.000-0.035 % of its bytes (0-23 bytes of a
640 x 480 mask; tests/test_warp_probe.py measures and asserts < 0.1 %).  The exact-value probe
(_probe, test_warp_probe_*) is the exactness check of k_warp_diff's arithmetic: gray2 := the oracle's
warped image of uniform noise at thresh 0, every mask byte an equality check of the warped value.
The same one-unit error changes the probe's mask at 0.990-1.000 of the in-frame pixels for every
kind (bar 0.90; same CPU test).  The path report (mdx_debug_warp_paths) says which rows each tile
ran -- general, fixed-point, affine FP64 or projective -- and the tests assert that each kind
reaches the rows it is there for, so a fast path that quietly fell back cannot pass untested.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _rot(deg, s=1.0, tx=0.0, ty=0.0, cx=0.0, cy=0.0):
    c, si = math.cos(math.radians(deg)) * s, math.sin(math.radians(deg)) * s
    # rotate/scale about (cx, cy), then translate
    return np.array([[c, -si, cx - c * cx + si * cy + tx], [si, c, cy - si * cx - c * cy + ty], [0.0, 0.0, 1.0]])


def _H(kind, w, h, Ht):
    return {
        "true": Ht,
        "identity": np.eye(3),
        "tie_translation": np.array([[1.0, 0.0, 1.0 / 64], [0.0, 1.0, -3.0 / 64], [0.0, 0.0, 1.0]]),
        "tie_scale_half": np.array([[0.5, 0.0, 0.25 / 32], [0.0, 2.0, 0.0], [0.0, 0.0, 1.0]]),
        "rot5": _rot(5.0, 1.0, 2.3, -1.1, w / 2, h / 2),
        "flip_x": np.array([[-1.0, 0.0, w - 1.0 + 0.3], [0.0, 1.0, 0.7], [0.0, 0.0, 1.0]]),
        "zoom_in": _rot(0.0, 1.6, 0.0, 0.0, w / 2, h / 2),
        "zoom_out": _rot(0.0, 0.6, 0.0, 0.0, w / 2, h / 2),
        "far_away": np.array([[1.0, 0.0, -5000.0], [0.0, 1.0, 12.0], [0.0, 0.0, 1.0]]),
        "m8_not_pow2": np.array([[1.01, 0.002, 3.2], [-0.003, 0.99, -1.7], [0.0, 0.0, 1.3]]),
        "projective": np.array([[1.002, 0.013, -2.5], [-0.011, 0.995, 1.75], [2.1e-5, -1.3e-5, 1.0]]),
        "singular": np.zeros((3, 3)),
        # fixed-point screening (warp_rows_fx): rows y = 32 mod 64 sit exactly on rounding ties
        # (X = 32 x + y / 64), the others 1/64 px away; and coordinates 2^-23 px past a tie
        "tie_rows": np.array([[1.0, 1.0 / 2048, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]),
        "near_tie": np.array([[1.0, 0.0, 0.5 / 32 + 2.0 ** -28], [0.0, 1.0, -0.5 / 32 - 2.0 ** -29], [0.0, 0.0, 1.0]]),
        "near_tie_rot": _rot(0.25, 1.0, 0.5 / 32 + 2.0 ** -27, 0.5 / 32 - 2.0 ** -26, w / 2, h / 2),
        # projective fast path (per-pixel W and 32 / W): perspective in x and y; a tiny perspective term
        # on a 1/64-px translation, so X sits within ~x^2 2^-35 px of a rounding tie (the division's
        # last bits decide); and a horizon (W = 0) inside the frame, where tiles fall back
        "proj_xy": np.array([[0.98, 0.021, 4.5], [-0.017, 1.01, -3.25], [-3.1e-5, 2.4e-5, 1.0]]),
        "proj_near_tie": np.linalg.inv(np.array([[1.0, 0.0, 1.0 / 64], [0.0, 1.0, -1.0 / 64],
                                                 [2.0 ** -40, 2.0 ** -41, 1.0]])),
        "proj_horizon": np.linalg.inv(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0 / (0.6 * w), 0.0, 1.0]])),
        # M = diag(2^21, 1): X = 2^26 (x - 40) passes INT_MIN for x < 8 and INT_MAX for x >= 72 (the
        # reference's clamp before cvRound, then the +-32768 clip of X >> 5); column 40 samples column 0
        "clamp": np.array([[2.0 ** -21, 0.0, 40.0], [0.0, 1.0, 0.3], [0.0, 0.0, 1.0]]),
        # every entry of the inverse is exact: W = 2 - x / 16 is exactly 0.0 at x = 32 (Wd = 0 there),
        # negative to its right, where x' = 32 (x - 16) / (x - 32), y' = h - 5 - y / |W| stay in frame
        "w_zero": np.array([[-1.0, 0.0, 16.0], [0.0, 1.0, 5.0 - h], [-1.0 / 32, 0.0, 1.0]]),
        # a homography is defined up to scale: -H samples the same points with W < 0 everywhere
        "neg_w": -np.array([[1.002, 0.013, -2.5], [-0.011, 0.995, 1.75], [2.1e-5, -1.3e-5, 1.0]]),
        # perspective in y only: M6 is exactly 0 (H10 = H20 = 0), M7 is not
        "proj_y": np.array([[1.003, 0.01, 2.25], [0.0, 0.99, -1.5], [0.0, 1.7e-5, 1.0]]),
    }[kind]


@pytest.fixture(scope="module")
def wctx(mdx):
    c = mdx.Context(0, 3840, 2160, 1)
    yield c
    c.close()


def _run(mdx, ctx, oracle, g1, g2, Hs, thresh):
    B, h, w = g1.shape
    Hb = np.ascontiguousarray(np.stack(Hs).astype(np.float64))
    ctx.set_params(thresh=thresh)
    d1, d2, dH, dM = (ctx.dev_alloc(x) for x in (g1.nbytes, g2.nbytes, Hb.nbytes, B * w * h))
    try:
        ctx.h2d(d1, g1); ctx.h2d(d2, g2); ctx.h2d(dH, Hb)
        ctx.h2d(dM, np.full(B * w * h, 0xAA, np.uint8))    # a byte the kernel never writes fails below
        ctx.warp_diff_dev(B, d1, d2, w, h, w, w * h, dH, dM)
        ctx.sync()
        out = np.empty((B, h, w), np.uint8)
        ctx.d2h(out, dM)
        codes = ctx.debug_warp_paths().reshape(B, -1)
    finally:
        ctx.set_params(thresh=190)
        for p in (d1, d2, dH, dM):
            ctx.dev_free(p)
    for i in range(B):
        warped = oracle.warp_perspective(g1[i], oracle.invert3x3(Hb[i]), nthreads=8)
        ref = np.where(np.abs(warped.astype(np.int16) - g2[i].astype(np.int16)) > thresh, 255, 0).astype(np.uint8)
        bad = np.argwhere(out[i] != ref)
        assert bad.size == 0, f"pair {i}: {len(bad)} mask pixels differ, first (y, x) {bad[:4].tolist()}"
    return codes


KINDS = ["true", "identity", "tie_translation", "tie_scale_half", "rot5", "flip_x", "zoom_in", "zoom_out",
         "far_away", "m8_not_pow2", "projective", "singular", "tie_rows", "near_tie", "near_tie_rot", "proj_xy",
         "proj_near_tie", "proj_horizon"]


# ---------------------------------------------------------------------------------------------
# Exact-value probe.  k_warp_diff never stores the warped image, only |warped - gray2| > thresh; with
# gray2 := the oracle's warped image and thresh = 0 the mask byte is 0 exactly where the kernel's
# warped byte equals the oracle's, so every pixel is an equality check of the warped VALUE.
PROBE_KINDS = KINDS + ["clamp", "w_zero", "neg_w", "proj_y"]
PROBE_SEED = 20261019
NSRC = 3                    # independent noise sources per homography
PATH_NAMES = ["general", "fixed-point", "affine FP64", "projective"]     # mdx_debug_warp_paths codes
# the row path each kind is there to reach on full-size tiles (dword-aligned rows, h >= 16)
FIXED_KINDS = ["identity", "tie_rows", "near_tie", "rot5"]               # M8 = 1: 32 / M8 a power of two
AFFINE_KINDS = ["m8_not_pow2"]
PROJ_KINDS = ["projective", "proj_xy", "proj_near_tie", "proj_y", "neg_w"]
GENERAL_KINDS = ["zoom_out", "clamp"]                                    # footprint too tall; |X| >= 2^30
MIXED_KINDS = ["proj_horizon", "w_zero"]                                 # W changes sign inside some tiles


def probe_H(mdx, kind, w, h):
    return _H(kind, w, h, mdx.synth_pair(500, w, h, 1)[2] if kind == "true" else None)


def probe_source(w, h, j):
    """Source j of the probe: uniform noise, so neighbouring 1/32-px positions give different bytes
    (the synthetic frames are blurred: most one-unit errors leave the byte unchanged)."""
    return np.random.default_rng([PROBE_SEED, w, h, j]).integers(0, 256, (h, w), dtype=np.uint8)


_PROBE_REFS = {}


def probe_ref(oracle, w, h, key, H, j):
    """The oracle's warp of source j under H, computed once per (size, key, source), read-only."""
    k = (w, h, key, j)
    if k not in _PROBE_REFS:
        r = oracle.warp_perspective(probe_source(w, h, j), oracle.invert3x3(H))
        r.setflags(write=False)
        _PROBE_REFS[k] = r
    return _PROBE_REFS[k]


def probe_gray2(ref, j, mode, thresh, seed):
    """gray2 of source j.  "sparse": ref, except ref +- 1 on the pixels whose label (one draw of
    0..15 per pixel, shared by the sources) is j: the expected mask is not constant, the sets of the
    three sources are disjoint, and every pixel is an exact-equality check in at least two of them.
    "boundary": ref + s (thresh + e), s = +-1, e in {0, 1} per pixel: every pixel sits exactly on the
    > thresh boundary.  "plain": ref.  Where ref + d would leave 0..255 the other sign is taken, and
    what still does not fit is clipped: the expectation is computed from the gray2 returned here."""
    rng = np.random.default_rng([PROBE_SEED, *seed])
    label = rng.integers(0, 16, ref.shape)
    rng = np.random.default_rng([PROBE_SEED, *seed, j + 1])
    s = rng.choice(np.array([-1, 1]), ref.shape)
    if mode == "sparse":
        d = np.where(label == j, s, 0)
    elif mode == "boundary":
        d = s * (thresh + rng.integers(0, 2, ref.shape))
    else:
        assert mode == "plain"
        d = np.zeros(ref.shape, np.int64)
    r = ref.astype(np.int64)
    g = np.where((r + d < 0) | (r + d > 255), r - d, r + d)
    return np.clip(g, 0, 255).astype(np.uint8)


def probe_expected(ref, g2, thresh):
    return np.where(np.abs(ref.astype(np.int16) - g2.astype(np.int16)) > thresh, 255, 0).astype(np.uint8)


def _probe(ctx, oracle, w, h, cases, thresh=0, mode="sparse", stride=None, frame_stride=None):
    """Run mdx_warp_diff_dev over cases [(key, H)] x NSRC sources and compare every mask byte with the
    oracle's; frames at row pitch `stride`, frame pitch `frame_stride` (padding: noise).  Returns the
    path codes, (len(cases), tiles): tile column fastest."""
    stride = stride or w
    fs = frame_stride or stride * h
    B = len(cases) * NSRC
    refs = [probe_ref(oracle, w, h, key, H, j) for key, H in cases for j in range(NSRC)]
    g1 = np.stack([probe_source(w, h, j) for _ in cases for j in range(NSRC)])
    g2 = np.stack([probe_gray2(refs[n], n % NSRC, mode, thresh, (w, h, n // NSRC)) for n in range(B)])
    exp = np.stack([probe_expected(refs[n], g2[n], thresh) for n in range(B)])
    Hb = np.ascontiguousarray(np.repeat(np.stack([H for _, H in cases]).astype(np.float64), NSRC, axis=0))
    pad = np.random.default_rng([PROBE_SEED, stride, fs])
    idx = ((np.arange(B) * fs)[:, None, None] + (np.arange(h) * stride)[None, :, None] + np.arange(w)[None, None, :])

    def lay(frames):
        buf = pad.integers(0, 256, B * fs + stride, dtype=np.uint8)
        buf[idx] = frames
        return buf
    b1, b2 = lay(g1), lay(g2)
    ctx.set_params(thresh=thresh)
    d1, d2, dH, dM = (ctx.dev_alloc(x) for x in (b1.nbytes, b2.nbytes, Hb.nbytes, B * w * h))
    try:
        ctx.h2d(d1, b1); ctx.h2d(d2, b2); ctx.h2d(dH, Hb)
        ctx.h2d(dM, np.full(B * w * h, 0xAA, np.uint8))    # a byte the kernel never writes fails below
        ctx.warp_diff_dev(B, d1, d2, w, h, stride, fs, dH, dM)
        ctx.sync()
        out = np.empty((B, h, w), np.uint8)
        ctx.d2h(out, dM)
        codes = ctx.debug_warp_paths()
    finally:
        ctx.set_params(thresh=190)
        for p in (d1, d2, dH, dM):
            ctx.dev_free(p)
    ntx = (w + 127) // 128
    assert codes.size == B * ntx * ((h + 63) // 64)
    codes = codes.reshape(len(cases), NSRC, -1)
    assert (codes == codes[:, :1]).all()        # the path depends on H and the geometry only
    codes = codes[:, 0]
    bad = np.argwhere(out != exp)
    msg = [f"{cases[n // NSRC][0]} source {n % NSRC} (y, x) = ({y}, {x}) path "
           f"{PATH_NAMES[codes[n // NSRC, (y // 64) * ntx + x // 128]]}: mask {out[n, y, x]:#x}, expected "
           f"{exp[n, y, x]:#x} (oracle warped {refs[n][y, x]}, gray2 {g2[n, y, x]})" for n, y, x in bad[:6]]
    assert not len(bad), (f"{w}x{h} pitch {stride}/{fs} thresh {thresh} {mode}: {len(bad)} mask bytes differ in pairs "
                          f"{sorted({cases[n // NSRC][0] for n in bad[:, 0]})}: " + "; ".join(msg))
    return codes


def _shares(codes):
    return " ".join(f"{PATH_NAMES[c]} {np.mean(codes == c):.3f}" for c in range(4) if (codes == c).any())


def _check_paths(kinds, codes, full, big=False):
    """Each kind's tiles ran the rows it is there for.  full: the launch allows the fast path; big: the
    frame has whole 128 x 64 tiles, whose footprints are what sends zoom_out to the general path
    (on a small frame's partial tiles it fits the staging buffer)."""
    for kind, c in zip(kinds, codes):
        got = set(c.tolist())
        if not full:
            assert got == {0}, (kind, got)
        elif kind in FIXED_KINDS:
            assert 1 in got and got <= {0, 1}, (kind, got)
        elif kind in AFFINE_KINDS:
            assert 2 in got and got <= {0, 2}, (kind, got)
        elif kind in PROJ_KINDS:
            assert 3 in got and got <= {0, 3}, (kind, got)
        elif kind in GENERAL_KINDS:
            assert 0 in got or not big, (kind, got)
        elif kind in MIXED_KINDS:       # the horizon crosses some tiles and leaves others
            assert got == {0, 3} if big else got <= {0, 3}, (kind, got)
        elif kind == "singular":
            # M = 0: Wd = 0, every corner maps to (0, 0), a 2 x 2 footprint; 32 / M8 is no power of
            # two, so it is the affine FP64 rows (X = 0 * Wd + magic) that must return src[0, 0]
            assert got == {2}, (kind, got)


PROBE_SIZES = [(132, 65), (68, 33), (388, 200), (131, 65), (130, 70), (150, 10)]


@pytest.mark.parametrize("w,h", PROBE_SIZES)
def test_warp_probe_geometries(mdx, wctx, oracle, w, h):
    """The warped value of every pixel, every kind, three noise sources, at the smallest sizes that
    keep each mechanism: (132, 65) a second tile column of one reference block and 4 columns and a
    second tile row of one row; (388, 200) 4 x 4 tiles with edge chunks on both borders; (131, 65) and
    (130, 70) w % 4 != 0 and (150, 10) h < 16 (reference blocks of 102 columns): general path only."""
    cases = [(k, probe_H(mdx, k, w, h)) for k in PROBE_KINDS]
    codes = _probe(wctx, oracle, w, h, cases)
    for k, c in zip(PROBE_KINDS, codes):
        print(f"warp paths {w}x{h} {k}: {_shares(c)}")
    _check_paths(PROBE_KINDS, codes, full=(w % 4 == 0 and h >= 16), big=(w, h) == (388, 200))


@pytest.mark.parametrize("stride,frame_stride", [(136, 136 * 65), (136, 136 * 65 + 2), (135, 135 * 65 + 1), (135, 135 * 65)])
def test_warp_probe_pitched(mdx, wctx, oracle, stride, frame_stride):
    """Row pitch != width at (132, 65): 136 with a dword-aligned frame pitch keeps the fast path;
    a frame pitch of 2 mod 4, and the unaligned row pitch 135 (frame pitch rounded up to 4, and not),
    clear vec_ok: general path only."""
    w, h = 132, 65
    cases = [(k, probe_H(mdx, k, w, h)) for k in PROBE_KINDS]
    codes = _probe(wctx, oracle, w, h, cases, stride=stride, frame_stride=frame_stride)
    _check_paths(PROBE_KINDS, codes, full=(stride % 4 == 0 and frame_stride % 4 == 0))


# one kind per row path: fixed point, affine FP64, projective, general
BOUNDARY_KINDS = ["rot5", "m8_not_pow2", "proj_xy", "zoom_out"]


@pytest.mark.parametrize("thresh", [0, 1, 10, 190, 254])
def test_warp_probe_threshold_boundary(mdx, wctx, oracle, thresh):
    """Every pixel exactly on the > thresh boundary (|warped - gray2| = thresh or thresh + 1, both
    signs): the fused comparison |s - 65536 g| >= 65536 t + 32800 at all values of the warped byte
    and gray2, on each row path."""
    w, h = 132, 65
    cases = [(k, probe_H(mdx, k, w, h)) for k in BOUNDARY_KINDS]
    codes = _probe(wctx, oracle, w, h, cases, thresh=thresh, mode="boundary")
    assert [int(c.max()) for c in codes] == [1, 2, 3, 2] and codes[3].min() == 0, codes.tolist()


@pytest.mark.parametrize("thresh", [-1, 255, 300])
def test_warp_probe_threshold_saturated(mdx, wctx, oracle, thresh):
    """thresh < 0: every byte moves; thresh >= 255: none (gray2 = the oracle's warped image)."""
    w, h = 132, 65
    cases = [(k, probe_H(mdx, k, w, h)) for k in BOUNDARY_KINDS]
    _probe(wctx, oracle, w, h, cases, thresh=thresh, mode="plain")


@pytest.mark.parametrize("w,h", [(640, 480), (1000, 300), (1984, 70), (128, 64), (132, 65), (68, 33)])
def test_warp_geometries(mdx, wctx, oracle, w, h):
    g1, g2 = [], []
    Hs = []
    for i, kind in enumerate(KINDS):
        a, b, Ht = mdx.synth_pair(500 + i, w, h, 1)
        g1.append(a); g2.append(b)
        Hs.append(_H(kind, w, h, Ht))
    _run(mdx, wctx, oracle, np.stack(g1), np.stack(g2), Hs, 190)


@pytest.mark.parametrize("thresh", [-1, 0, 10, 190, 254, 255, 300])
def test_warp_thresholds(mdx, wctx, oracle, thresh):
    w, h = 640, 480
    a, b, Ht = mdx.synth_pair(77, w, h, 1)
    a2, b2, _ = mdx.synth_pair(78, w, h, 1)
    _run(mdx, wctx, oracle, np.stack([a, a2]), np.stack([b, b2]), [Ht, _H("rot5", w, h, Ht)], thresh)


def test_warp_4k_true_h(mdx, wctx, oracle):
    """The roofline workload's geometry (bench.py --only-roofline), one pair."""
    w, h = 3840, 2160
    a, b, Ht = mdx.synth_pair(20141105, w, h, 1)
    _run(mdx, wctx, oracle, a[None], b[None], [Ht], 190)


def test_warp_4k_projective(mdx, wctx, oracle):
    """The bench's projective roofline sub-line geometry (roofline.projective): 4K with the tests'
    perspective H, and its near-tie variant, both on the projective fast path."""
    w, h = 3840, 2160
    a, b, Ht = mdx.synth_pair(20141105, w, h, 1)
    a2, b2, _ = mdx.synth_pair(20141106, w, h, 1)
    _run(mdx, wctx, oracle, np.stack([a, a2]), np.stack([b, b2]),
         [_H("projective", w, h, Ht), _H("proj_near_tie", w, h, Ht)], 190)


def test_warp_projective_random(mdx, wctx, oracle):
    """Random projective H across the projective fast path's range (round 6: one v_rcp_f64 per four
    pixels of the product of their W, one quadratic Newton step, the shift-add boundary test):
    perspective terms from 1e-7 to 4e-4 per pixel, rotations, anisotropic scales and translations
    with 1/64-px parts, every mask byte against the oracle.  The first eight stay mild (|angle| <=
    1 deg, scales 0.97-1.03, perspective <= 5e-5: W within ~10% over the frame), so nearly every
    tile's footprint fits the staging buffer and takes the projective fast path; the last four are
    strong (W varying by up to ~1.5x, a horizon in some), where tiles also fall back.  That is
    asserted: at least 90 % of each mild homography's tiles report the projective rows
    (mdx_debug_warp_paths).  The same twelve also go through the exact-value probe at (388, 200)."""
    w, h = 1920, 1080
    Hs = _random_projective()
    g1, g2 = [], []
    for i in range(12):
        a, b, _ = mdx.synth_pair(900 + i, w, h, 1)
        g1.append(a); g2.append(b)
    codes = _run(mdx, wctx, oracle, np.stack(g1), np.stack(g2), Hs, 190)
    for i, c in enumerate(codes):
        print(f"warp paths {w}x{h} random projective {i} ({'mild' if i < 8 else 'strong'}): {_shares(c)}")
    for i in range(8):
        assert np.mean(codes[i] == 3) >= 0.90, (i, _shares(codes[i]))
    pc = _probe(wctx, oracle, 388, 200, [(f"random_projective_{i}", H) for i, H in enumerate(Hs)])
    for i, c in enumerate(pc):
        print(f"warp paths 388x200 random projective {i}: {_shares(c)}")
    assert all(3 in c for c in pc[:8])


def test_warp_paths_hook(mdx, oracle):
    """mdx_debug_warp_paths: an error before the context's first warp launch; after a whole-path call
    one code per tile of that call's launch (a first-4 fit is projective: general or projective rows)."""
    w, h = 320, 240
    a, b, _ = mdx.synth_pair(20141105, w, h, 1)
    with mdx.Context(0, w, h, 1) as c:
        with pytest.raises(mdx.MdxError, match="no warp launch"):
            c.debug_warp_paths()
        res = c.flow_warp_diff(a, b)
        codes = c.debug_warp_paths()
        assert codes.size == 3 * 4 and res.num_vectors >= 4
        M = oracle.invert3x3(res.H).ravel()
        assert set(codes.tolist()) <= ({0, 3} if M[6] != 0.0 or M[7] != 0.0 else {0, 1, 2}), codes.tolist()


def _random_projective():
    """test_warp_projective_random's twelve homographies: eight mild, four strong."""
    rng = np.random.default_rng(20261018)
    Hs = []
    for i in range(12):
        mild = i < 8
        ang = math.radians(rng.uniform(-1.0, 1.0) if mild else rng.uniform(-8.0, 8.0))
        sx, sy = rng.uniform(0.97, 1.03, 2) if mild else rng.uniform(0.8, 1.25, 2)
        p6, p7 = (rng.choice([-1.0, 1.0], 2) * 10.0 ** rng.uniform(-7.0, -4.3 if mild else -3.4, 2))
        tx, ty = rng.uniform(-30, 30, 2) + rng.integers(0, 64, 2) / 64.0
        Hs.append(np.array([[sx * math.cos(ang), -sy * math.sin(ang), tx],
                            [sx * math.sin(ang), sy * math.cos(ang), ty], [p6, p7, 1.0]]))
    return Hs


def test_div32_is_ieee_division(mdx, wctx):
    """The projective fast path's 32 / W (mdx_warp.hip div32: the IEEE division sequence without its
    range-scaling steps) equals correctly rounded IEEE division bit for bit over its range
    |W| in [2^-100, 2^100]: random mantissas over every exponent, both signs, and hard mantissas
    (all ones, powers of two, near one)."""
    import ctypes as C
    rng = np.random.default_rng(11)
    n = 1 << 20
    e = rng.integers(-100, 100, n)
    m = 1.0 + rng.random(n)
    d = np.ldexp(m, e) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    hard = []
    for ex in range(-100, 100):
        for mm in (1.0, np.nextafter(2.0, 0.0), np.nextafter(1.0, 2.0), 1.5, 1.0 + 2.0 ** -26, 2.0 - 2.0 ** -26):
            hard += [np.ldexp(mm, ex), -np.ldexp(mm, ex)]
    d[:len(hard)] = hard
    d = np.ascontiguousarray(d[(np.abs(d) >= 2.0 ** -100) & (np.abs(d) <= 2.0 ** 100)])
    di, do = wctx.dev_alloc(d.nbytes), wctx.dev_alloc(d.nbytes)
    try:
        wctx.h2d(di, d)
        assert mdx.lib().mdx_debug_div32(wctx._h, C.c_void_p(di), C.c_void_p(do), len(d)) == 0
        wctx.sync()
        out = np.empty_like(d)
        wctx.d2h(out, do)
    finally:
        wctx.dev_free(di)
        wctx.dev_free(do)
    ref = 32.0 / d
    bad = np.nonzero(out.view(np.uint64) != ref.view(np.uint64))[0]
    assert bad.size == 0, f"{bad.size} of {len(d)} differ, first W {d[bad[:4]].tolist()}"


def test_copy_ceiling_probe(mdx, wctx):
    """The bench's copy-ceiling probe (mdx_probe_stream3_dev) computes the same 3 B/px result as an
    identity warp would: mask = |a - b| > t; and rejects unaligned sizes."""
    rng = np.random.default_rng(5)
    n = 1 << 20
    a = rng.integers(0, 256, n, dtype=np.uint8)
    b = rng.integers(0, 256, n, dtype=np.uint8)
    da, db, dm = (wctx.dev_alloc(n) for _ in range(3))
    try:
        wctx.h2d(da, a); wctx.h2d(db, b)
        for t in (-1, 0, 190, 255):
            wctx.probe_stream3_dev(n, da, db, dm, t)
            wctx.sync()
            out = np.empty(n, np.uint8)
            wctx.d2h(out, dm)
            ref = np.where(np.abs(a.astype(np.int16) - b.astype(np.int16)) > t, 255, 0).astype(np.uint8)
            assert np.array_equal(out, ref), t
        with pytest.raises(mdx.MdxError):
            wctx.probe_stream3_dev(n - 8, da, db, dm)
    finally:
        for p in (da, db, dm):
            wctx.dev_free(p)
