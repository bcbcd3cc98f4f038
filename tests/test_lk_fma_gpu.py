"""k_lk_iter's two row bodies: the exact one (round the product, then add) and the fused one (one
fma per element), chosen per wave and Newton iteration by the per-point product certificate
(mdx_lk.hip: every Ix / Iy of the point's 40x40 window at that level is at most 2056 in magnitude,
so every product with |J - I| * 32 <= 8160 stays below 2^24 and the fma has the same bits).

Frames are 200x160 gray at pixel_step 10: two pyramid levels, level 1 on k_lk_iter<4, 56> and level 0
on k_lk_iter<8, 112>.  Every case is compared with the oracle bit for bit (next_pts as uint32, status,
num_vectors, H as uint64 and the mask), once with the default and once with MDX_LK_FMA=0; a debug
context's counters (mdx_debug_copy selector 6) say which body the wave-iterations of each level took.
"""
import functools

import numpy as np
import pytest

from lk_scenes import PS, H, W, edges_pair, mixed_pair, smooth_pair
from oracle_check import assert_batch_equals_oracle, lk_env, run_batch, without

pytestmark = pytest.mark.gpu

NLEV = 2                      # levels 1 and 0
CERT_MAX = 2056               # mdx_lk.hip kLkCertMax


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
        pairs = [smooth_pair(11), smooth_pair(12)]
    elif name == "edges":
        pairs = [edges_pair(1), edges_pair(0)]
    else:
        pairs = [mixed_pair(21), mixed_pair(22)]
    return pairs


@functools.lru_cache(maxsize=None)
def _refs(name):
    from oracle import pyoracle
    return [pyoracle.calculate_optical_flow(a, b, pixel_step=PS, min_vector_size=1.0) for a, b in _case(name)]


def _run(mdx, pairs, slots, debug, pipelined=False):
    """The batch entry over pairs[slots[i]] (no Vec4d buffer; pipelined: two calls back to back)."""
    g1 = np.stack([pairs[s][0] for s in slots])
    g2 = np.stack([pairs[s][1] for s in slots])
    return run_batch(mdx, g1, g2, create=dict(pixel_step=PS, min_vector_size=1.0, call_pipelining=int(pipelined)),
                     vectors=False, calls=2 if pipelined else 1, back_to_back=True, body_counts=debug)


def _check(got, refs, slots, label):
    assert_batch_equals_oracle(got, [refs[s] for s in slots], label, fields=without("vectors"))


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
    lk_env(monkeypatch, fma=fma, debug=True)
    got = _run(mdx, pairs, [0, 1], debug=True)
    cnt = got["body_counts"]
    print("body counts [level][exact, fused]:", cnt[:NLEV].tolist())
    _check(got, _refs("smooth"), [0, 1], f"smooth fma={fma}")
    if fma == "0":
        _check_forced_exact(cnt)
    else:
        assert (cnt[:NLEV, 0] == 0).all() and (cnt[:NLEV, 1] > 0).all(), cnt[:NLEV]
    assert (cnt[NLEV:] == 0).all()


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
    lk_env(monkeypatch, fma=fma, debug=True)
    got = _run(mdx, pairs, [0, 1], debug=True)
    cnt = got["body_counts"]
    print("body counts [level][exact, fused]:", cnt[:NLEV].tolist())
    _check(got, _refs("edges"), [0, 1], f"edges fma={fma}")
    if fma == "0":
        _check_forced_exact(cnt)
    else:
        assert cnt[0, 0] > 0 and cnt[0, 1] == 0, cnt[:NLEV]
        for lvl, m in enumerate(_max_deriv(oracle, pairs[0][0])):
            if m > CERT_MAX:
                assert cnt[lvl, 0] > 0, (lvl, cnt[:NLEV])


@pytest.mark.parametrize("fma", ["1", "0"])
def test_mixed_scene_takes_both_bodies(mdx, oracle, monkeypatch, fma):
    """The smooth scene with one 0/255 rectangle: points near it are not certified, the others are,
    and both kinds share groups and waves.  Both bodies run."""
    pairs = _case("mixed")
    assert _max_deriv(oracle, pairs[0][0])[0] > CERT_MAX
    lk_env(monkeypatch, fma=fma, debug=True)
    got = _run(mdx, pairs, [0, 1], debug=True)
    cnt = got["body_counts"]
    print("body counts [level][exact, fused]:", cnt[:NLEV].tolist())
    _check(got, _refs("mixed"), [0, 1], f"mixed fma={fma}")
    if fma == "0":
        _check_forced_exact(cnt)
    else:
        assert cnt[0, 0] > 0 and cnt[0, 1] > 0, cnt[:NLEV]


@pytest.mark.parametrize("fma", ["1", "0"])
def test_mixed_scene_batch_of_16_dataflow(mdx, oracle, monkeypatch, fma):
    """The mixed scene in a batch of 16 with call pipelining, which takes the level dataflow (the
    k_lk_iter<.., true> instantiations): the results of every slot equal the batch-1 results and the
    oracle's."""
    pairs = _case("mixed")
    slots = [i % 2 for i in range(16)]
    assert mdx.grid_count(W, H, PS) % 16 == 0                    # the dataflow's condition
    lk_env(monkeypatch, fma=fma)
    one = [_run(mdx, pairs, [s], debug=False) for s in (0, 1)]
    got = _run(mdx, pairs, slots, debug=False, pipelined=True)
    _check(got, _refs("mixed"), slots, f"mixed x16 fma={fma}")
    for i, s in enumerate(slots):
        for k in ("next_pts", "status", "mask", "H", "num_vectors"):
            assert got[k][i].tobytes() == one[s][k][0].tobytes(), f"slot {i} {k}"
