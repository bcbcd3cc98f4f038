"""k_lk_iter's two row bodies: the exact one (round the product, then add) and the fused one (one
fma per element), chosen per wave and Newton iteration by the per-point product certificate
(mdx_lk.hip: every Ix / Iy of the point's 40x40 window at that level is at most 2056 in magnitude,
so every product with |J - I| * 32 <= 8160 stays below 2^24 and the fma has the same bits).

Frames are 200x160 gray at pixel_step 10: two pyramid levels, level 1 on k_lk_iter<4, 56> and level 0
on k_lk_iter<8, 112>.  Every case is compared with the oracle bit for bit (next_pts as uint32, status,
num_vectors), once with the default and once with MDX_LK_FMA=0; a debug context's counters
(mdx_debug_copy selector 6) say which body the wave-iterations of each level took.
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, PS = 200, 160, 10
NLEV = 2                      # levels 1 and 0
CERT_MAX = 2056               # mdx_lk.hip kLkCertMax
K5 = np.array([1, 4, 6, 4, 1], np.float64) / 16


def _blur(a, times):
    for _ in range(times):
        a = sum(k * np.roll(a, s, 0) for k, s in zip(K5, range(-2, 3)))
        a = sum(k * np.roll(a, s, 1) for k, s in zip(K5, range(-2, 3)))
    return a


def _shifted(base, dx, dy):
    """base sampled at (x + dx, y + dy), 0 <= dx, dy < 1, bilinear; the margin of 8 is cut off."""
    b = base
    s = ((1 - dx) * (1 - dy) * b[:-1, :-1] + dx * (1 - dy) * b[:-1, 1:] + (1 - dx) * dy * b[1:, :-1]
         + dx * dy * b[1:, 1:])
    return np.ascontiguousarray(np.clip(np.rint(s[8:8 + H, 8:8 + W]), 0, 255).astype(np.uint8))


def _smooth_base(seed):
    """Blurred noise, 128 +- 30: neighbouring pixels differ by a few grey levels."""
    r = np.random.default_rng(seed).random((H + 17, W + 17))
    b = _blur(r, 2)
    return 128 + 60 * (b - b.min()) / (b.max() - b.min()) - 30


def _smooth_pair(seed):
    base = _smooth_base(seed)
    return _shifted(base, 0, 0), _shifted(base, 0.4, 0.3)


def _edges_pair(axis):
    """0/255 blocks of 8 px, the second frame moved by 3 px along `axis`."""
    yy, xx = np.mgrid[0:H + 3, 0:W + 3]
    board = ((((xx // 8) + (yy // 8)) & 1) * 255).astype(np.uint8)
    a = np.ascontiguousarray(board[:H, :W])
    b = np.ascontiguousarray(board[3:3 + H, :W] if axis == 0 else board[:H, 3:3 + W])
    return a, b


def _mixed_pair(seed):
    """The smooth scene with one 0/255 rectangle (a 255 block inside a 0 frame), moving with it."""
    base = _smooth_base(seed)
    base[8 + 60:8 + 100, 8 + 70:8 + 120] = 0
    base[8 + 68:8 + 92, 8 + 78:8 + 112] = 255
    return _shifted(base, 0, 0), _shifted(base, 0.4, 0.3)


def _scharr(img):
    """calcSharrDeriv in numpy (reflect-101 borders): (Ix, Iy) as int32."""
    p = np.pad(img.astype(np.int32), 1, mode="reflect")
    t0 = 3 * (p[:-2] + p[2:]) + 10 * p[1:-1]          # vertical smoothing, all padded columns
    t1 = p[2:] - p[:-2]
    ix = t0[:, 2:] - t0[:, :-2]
    iy = 3 * (t1[:, :-2] + t1[:, 2:]) + 10 * t1[:, 1:-1]
    return ix, iy


def _levels(oracle, img):
    out = [img]
    for _ in range(NLEV - 1):
        out.append(oracle.pyrdown(out[-1]))
    return out


def _max_deriv(oracle, img):
    """max(|Ix|, |Iy|) over each level of the frame's pyramid."""
    return [int(max(np.abs(d).max() for d in _scharr(l))) for l in _levels(oracle, img)]


@functools.lru_cache(maxsize=None)
def _case(name):
    if name == "smooth":
        pairs = [_smooth_pair(11), _smooth_pair(12)]
    elif name == "edges":
        pairs = [_edges_pair(1), _edges_pair(0)]
    else:
        pairs = [_mixed_pair(21), _mixed_pair(22)]
    return pairs


@functools.lru_cache(maxsize=None)
def _refs(name):
    from oracle import pyoracle
    return [pyoracle.calculate_optical_flow(a, b, pixel_step=PS, min_vector_size=1.0) for a, b in _case(name)]


def _run(mdx, pairs, slots, debug, pipelined=False):
    """The batch entry over pairs[slots[i]]; -> (next_pts, status, num_vectors, body counts or None)."""
    batch = len(slots)
    n = mdx.grid_count(W, H, PS)
    g1 = np.stack([pairs[s][0] for s in slots])
    g2 = np.stack([pairs[s][1] for s in slots])
    with mdx.Context(0, W, H, batch, pixel_step=PS, min_vector_size=1.0, call_pipelining=int(pipelined)) as c:
        d1, d2 = c.dev_alloc(g1.nbytes), c.dev_alloc(g2.nbytes)
        c.h2d(d1, g1)
        c.h2d(d2, g2)
        o = dict(np=c.dev_alloc(batch * n * 8), st=c.dev_alloc(batch * n), mask=c.dev_alloc(batch * W * H),
                 H=c.dev_alloc(batch * 72), num=c.dev_alloc(batch * 4))
        for _ in range(2 if pipelined else 1):
            c.flow_warp_diff_batch_dev(batch, d1, d2, W, H, W, W * H, 0, d_next_pts=o["np"], d_status=o["st"],
                                       d_mask=o["mask"], d_H=o["H"], d_num_vectors=o["num"])
        c.sync()
        nextp = np.empty((batch, n, 2), np.float32)
        st = np.empty((batch, n), np.uint8)
        num = np.empty(batch, np.int32)
        c.d2h(nextp, o["np"])
        c.d2h(st, o["st"])
        c.d2h(num, o["num"])
        cnt = None
        if debug:
            cnt = np.zeros((8, 2), np.uint32)          # [level][exact, fused]
            rc = mdx.lib().mdx_debug_copy(c._h, 6, cnt.ctypes.data_as(C.c_void_p), cnt.nbytes)
            assert rc == 0
        for p in list(o.values()) + [d1, d2]:
            c.dev_free(p)
    return nextp, st, num, cnt


def _check(got, refs, slots, label):
    nextp, st, num, _ = got
    for i, s in enumerate(slots):
        ref = refs[s]
        assert num[i] == ref["num_vectors"], f"{label} slot {i}"
        np.testing.assert_array_equal(st[i], ref["status"], err_msg=f"{label} slot {i}")
        bad = np.nonzero((nextp[i].view(np.uint32) != ref["next_pts"].view(np.uint32)).any(axis=1))[0]
        assert bad.size == 0, f"{label} slot {i}: {bad.size} LK points differ, first {bad[:5]}"


def _env(monkeypatch, fma, debug=True):
    if debug:
        monkeypatch.setenv("MDX_LK_DEBUG", "1")
    if fma == "0":
        monkeypatch.setenv("MDX_LK_FMA", "0")
    else:
        monkeypatch.delenv("MDX_LK_FMA", raising=False)


def _check_forced_exact(cnt):
    """MDX_LK_FMA=0: every wave-iteration takes the exact body."""
    assert (cnt[:, 1] == 0).all() and (cnt[:NLEV, 0] > 0).all(), cnt[:NLEV]


@pytest.mark.parametrize("fma", ["1", "0"])
def test_smooth_scene_runs_fused_only(mdx, oracle, monkeypatch, fma):
    """Blurred low-contrast noise moved by (0.4, 0.3) px: every Scharr value of every level is within
    the bound, so every point is certified and no wave-iteration takes the exact body."""
    pairs = _case("smooth")
    for a, _ in pairs:
        assert max(_max_deriv(oracle, a)) <= CERT_MAX
    _env(monkeypatch, fma)
    got = _run(mdx, pairs, [0, 1], debug=True)
    print("body counts [level][exact, fused]:", got[3][:NLEV].tolist())
    _check(got, _refs("smooth"), [0, 1], f"smooth fma={fma}")
    if fma == "0":
        _check_forced_exact(got[3])
    else:
        assert (got[3][:NLEV, 0] == 0).all() and (got[3][:NLEV, 1] > 0).all(), got[3][:NLEV]
    assert (got[3][NLEV:] == 0).all()


@pytest.mark.parametrize("fma", ["1", "0"])
def test_hard_edges_keep_the_exact_body(mdx, oracle, monkeypatch, fma):
    """0/255 blocks moved by 3 px: some pixel has |Ix| > 2056 together with |I2 - I1| >= 129, so
    products above 2^24 occur (a fused multiply-add would round them differently).  At level 0
    every window holds block edges: no point is certified and every wave-iteration is exact."""
    pairs = _case("edges")
    for a, b in pairs:
        ix, iy = _scharr(a)
        big = (np.maximum(np.abs(ix), np.abs(iy)) > CERT_MAX) & (np.abs(b.astype(np.int32) - a) >= 129)
        assert big.any()
    _env(monkeypatch, fma)
    got = _run(mdx, pairs, [0, 1], debug=True)
    print("body counts [level][exact, fused]:", got[3][:NLEV].tolist())
    _check(got, _refs("edges"), [0, 1], f"edges fma={fma}")
    if fma == "0":
        _check_forced_exact(got[3])
    else:
        assert got[3][0, 0] > 0 and got[3][0, 1] == 0, got[3][:NLEV]
        for lvl, m in enumerate(_max_deriv(oracle, pairs[0][0])):
            if m > CERT_MAX:
                assert got[3][lvl, 0] > 0, (lvl, got[3][:NLEV])


@pytest.mark.parametrize("fma", ["1", "0"])
def test_mixed_scene_takes_both_bodies(mdx, oracle, monkeypatch, fma):
    """The smooth scene with one 0/255 rectangle: points near it are not certified, the others are,
    and both kinds share groups and waves.  Both bodies run."""
    pairs = _case("mixed")
    assert _max_deriv(oracle, pairs[0][0])[0] > CERT_MAX
    _env(monkeypatch, fma)
    got = _run(mdx, pairs, [0, 1], debug=True)
    print("body counts [level][exact, fused]:", got[3][:NLEV].tolist())
    _check(got, _refs("mixed"), [0, 1], f"mixed fma={fma}")
    if fma == "0":
        _check_forced_exact(got[3])
    else:
        assert got[3][0, 0] > 0 and got[3][0, 1] > 0, got[3][:NLEV]


@pytest.mark.parametrize("fma", ["1", "0"])
def test_mixed_scene_batch_of_16_dataflow(mdx, oracle, monkeypatch, fma):
    """The mixed scene in a batch of 16 with call pipelining, which takes the level dataflow (the
    k_lk_iter<.., true> instantiations): the results of every slot equal the batch-1 results and the
    oracle's."""
    pairs = _case("mixed")
    slots = [i % 2 for i in range(16)]
    assert mdx.grid_count(W, H, PS) % 16 == 0                    # the dataflow's condition
    _env(monkeypatch, fma, debug=False)
    one = [_run(mdx, pairs, [s], debug=False) for s in (0, 1)]
    got = _run(mdx, pairs, slots, debug=False, pipelined=True)
    _check(got, _refs("mixed"), slots, f"mixed x16 fma={fma}")
    for i, s in enumerate(slots):
        assert np.array_equal(got[0][i].view(np.uint32), one[s][0][0].view(np.uint32)), f"slot {i}"
        assert np.array_equal(got[1][i], one[s][1][0]) and got[2][i] == one[s][2][0], f"slot {i}"
