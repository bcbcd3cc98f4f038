"""OutlierDetector::findOutliers / getOutlierVectors on the device (mdx_find_outliers).

Reference: findOutliers, getOutlierVectors, createAngleMatrix, createMagnitudeMatrix, getMedian and
createMask (common/src/outlier_detector.cpp:37-186).  Restated from the source; unpinned against a
real build.

The checker below is the reference's literal loop: gather the selected values, np.sort, the two-case
median, np.abs, 0.6745 * diff / mad > 3.5.  The magnitude is np.sqrt(dy*dy + dx*dx) (numpy does not
fuse); the angle is math.atan2 per element, the libm function the library's host code calls, so every
device output must equal the checker bit for bit, with no margin.  The checker shares nothing with
the device's key mapping or radix selection.  std::sort leaves the order of -0.0 and +0.0 open, so a
median that is zero is compared as a value; every other double is compared as bits.
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

STAT_INTS = ("selected", "flagged_angle", "flagged_magnitude", "outliers")
STAT_DOUBLES = ("median_angle", "mad_angle", "median_magnitude", "mad_magnitude")


def median_of_sorted(v):
    """getMedian (:97-119) after its sort."""
    m = len(v)
    if m % 2 == 0:
        return (v[m // 2 - 1] + v[m // 2]) / 2.0
    return v[(m - 1) // 2]


def channels(vec):
    dx, dy = vec[:, 2], vec[:, 3]
    ang = np.array([math.atan2(y, x) for x, y in zip(dx.tolist(), dy.tolist())], np.float64).reshape(-1)
    mag = np.sqrt(dy * dy + dx * dx)
    return ang, mag


def outliers_reference(vectors, include_zeros=False):
    vec = np.ascontiguousarray(vectors, np.float64).reshape(-1, 4)
    n = len(vec)
    sel = np.ones(n, bool) if include_zeros else (np.abs(vec[:, 2]) > 0) | (np.abs(vec[:, 3]) > 0)
    idx = np.nonzero(sel)[0]
    flags = np.zeros(n, np.uint8)
    stats = dict.fromkeys(STAT_INTS, 0)
    stats.update(dict.fromkeys(STAT_DOUBLES, 0.0))
    stats["selected"] = len(idx)
    for bit, name, values in zip((1, 2), ("angle", "magnitude"), channels(vec)):
        vals = values[idx]
        if len(vals) == 0:                                   # :140-143
            continue
        median = median_of_sorted(np.sort(vals))
        diff = np.abs(vals - median)
        mad = median_of_sorted(np.sort(diff))
        with np.errstate(all="ignore"):
            z = 0.6745 * diff / mad
            hit = np.abs(z) > 3.5
        flags[idx[hit]] |= bit
        stats["median_" + name], stats["mad_" + name] = float(median), float(mad)
        stats["flagged_" + name] = int(hit.sum())
    stats["outliers"] = int(np.count_nonzero(flags))
    out = np.where((flags != 0)[:, None], vec, 0.0)          # getOutlierVectors (:55-71)
    return dict(flags=flags, outlier_vectors=out, stats=stats)


def vecs(rows):
    return np.array(rows, np.float64).reshape(-1, 4)


def field(dx, dy, seed=1):
    """(n, 4) vectors with the given flow at seeded positions."""
    dx, dy = np.asarray(dx, np.float64).reshape(-1), np.asarray(dy, np.float64).reshape(-1)
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(0, 640, (len(dx), 2)), dx[:, None], dy[:, None]], 1)


# ---------------------------------------------------------------- inputs of the GPU cases

SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]


@functools.lru_cache(maxsize=None)
def coherent_input(n):
    """(a) a coherent translation plus 3 % vectors pointing anywhere."""
    rng = np.random.default_rng(21000 + n)
    dx = 3.0 + rng.normal(0, 0.05, n)
    dy = -1.5 + rng.normal(0, 0.05, n)
    wild = rng.random(n) < 0.03
    if n >= 63:
        wild[rng.choice(n, 2, replace=False)] = True
    ang, mag = rng.uniform(-np.pi, np.pi, n), rng.uniform(0, 12, n)
    dx[wild], dy[wild] = (mag * np.cos(ang))[wild], (mag * np.sin(ang))[wild]
    return field(dx, dy, n)


@functools.lru_cache(maxsize=None)
def uniform_input(n):
    """(b) uniform random."""
    rng = np.random.default_rng(23000 + n)
    return field(rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), n)


@functools.lru_cache(maxsize=None)
def holes_input(n):
    """(c) uniform_input(n) with inactive (x, y, 0, 0) and (-1, -1, 0, 0) entries interleaved: m != n
    without include_zeros, and m takes both parities over the sizes."""
    rng = np.random.default_rng(25000 + n)
    total = n + n // 2 + 3
    where = np.sort(rng.choice(total, n, replace=False))
    out = np.zeros((total, 4))
    out[:, :2] = rng.uniform(0, 640, (total, 2))
    out[::3, :2] = -1.0
    out[where] = uniform_input(n)
    return out


FAMILIES = {"coherent": coherent_input, "uniform": uniform_input, "holes": holes_input}


@functools.lru_cache(maxsize=None)
def family_reference(family, n, include_zeros):
    return outliers_reference(FAMILIES[family](n), include_zeros)


def identical_field():
    return field(np.full(500, 2.0), np.full(500, 1.0))


def ties_field():
    """4 distinct vectors in 2000; both channels' medians lie inside a run of equal keys."""
    rng = np.random.default_rng(5)
    rows = [(1.0, 0.0)] * 600 + [(0.0, 2.0)] * 800 + [(-3.0, 0.0)] * 500 + [(0.0, -40.0)] * 100
    d = np.array(rows)[rng.permutation(2000)]
    return field(d[:, 0], d[:, 1])


def split_angles_field(m=1000, a=0.7):
    """Angles -a and +a, m / 2 each: the two middle elements lie on either side of the sign."""
    rng = np.random.default_rng(6)
    s = np.where(rng.permutation(m) < m // 2, -1.0, 1.0)
    mag = rng.uniform(1, 2, m)
    return field(mag * np.cos(a), s * (mag * np.sin(a)))


def signed_zero_angles_field():
    rng = np.random.default_rng(7)
    dx = rng.uniform(1, 3, 301)
    dx[17] = 80.0
    dy = np.where(rng.random(301) < 0.5, -0.0, 0.0)
    return field(dx, dy)


def denormal_field():
    k = np.tile([1.0, 2.0, 3.0, 4.0, 5.0], 60)
    k[[7, 120]] = 100.0
    return field(k * 1e-160, np.zeros(300))


def huge_field():
    rng = np.random.default_rng(8)
    dx = rng.uniform(1, 2, 257) * 1e149
    dy = rng.uniform(-1, 1, 257) * 1e148
    dx[[3, 200]] = 9e149
    dy[200] = -9e149
    return field(dx, dy)


def last_bit_field():
    two = float(np.nextafter(2.0, 3.0))
    return field([1.0] * 4 + [2.0, two] + [3.0] * 4, np.zeros(10))


def single_active_field():
    v = np.zeros((40, 4))
    v[:, :2] = -1.0
    v[23] = (50, 60, 1.5, -2.5)
    return v


def no_active_field():
    v = np.zeros((70, 4))
    v[:, 0] = np.arange(70)
    return v


HAND_MADE = {"identical": identical_field, "ties": ties_field, "split_angles": split_angles_field,
             "split_angles_odd": lambda: split_angles_field(1001), "signed_zero_angles": signed_zero_angles_field,
             "denormal": denormal_field, "huge": huge_field, "last_bit": last_bit_field,
             "single_active": single_active_field, "no_active": no_active_field}
BOTH_OUTCOMES = {"ties", "signed_zero_angles", "denormal", "huge"}      # cases meant to flag some and not others


def passes(diff, mad):
    with np.errstate(all="ignore"):
        return bool(np.abs(0.6745 * np.float64(diff) / np.float64(mad)) > 3.5)


def threshold_field():
    """Magnitudes with median 100 and MAD 2 exactly (98 x 50, 100 x 21, 102 x 50), and four more at
    the smallest double above 100 whose z-score passes, the double just below it, and their mirror
    images below 100: two are flagged, two are not, one ulp apart."""
    hi = 100.0 + 3.5 * 2.0 / 0.6745
    while passes(abs(np.nextafter(hi, 0.0) - 100.0), 2.0):
        hi = float(np.nextafter(hi, 0.0))
    while not passes(abs(hi - 100.0), 2.0):
        hi = float(np.nextafter(hi, np.inf))
    lo = 100.0 - 3.5 * 2.0 / 0.6745
    while passes(abs(np.nextafter(lo, np.inf) - 100.0), 2.0):
        lo = float(np.nextafter(lo, np.inf))
    while not passes(abs(lo - 100.0), 2.0):
        lo = float(np.nextafter(lo, 0.0))
    edge = [hi, float(np.nextafter(hi, 0.0)), lo, float(np.nextafter(lo, np.inf))]
    return field([98.0] * 50 + [100.0] * 21 + [102.0] * 50 + edge, np.zeros(125)), edge


# ---------------------------------------------------------------- CPU: the checker itself

def magnitudes(values):
    return field(values, np.zeros(len(values)))


def test_checker_known_answer():
    r = outliers_reference(magnitudes([1, 2, 3, 4, 100]))
    assert (r["stats"]["median_magnitude"], r["stats"]["mad_magnitude"]) == (3.0, 1.0)
    assert list(r["flags"]) == [0, 0, 0, 0, 2]
    assert r["stats"]["mad_angle"] == 0.0 and r["stats"]["flagged_angle"] == 0
    assert np.array_equal(r["outlier_vectors"][:4], np.zeros((4, 4)))
    assert np.array_equal(r["outlier_vectors"][4], magnitudes([1, 2, 3, 4, 100])[4])


def test_checker_even_median():
    r = outliers_reference(magnitudes([1, 2, 4, 8]))
    assert r["stats"]["median_magnitude"] == 3.0             # (2 + 4) / 2
    assert r["stats"]["mad_magnitude"] == 1.5                # diffs 2, 1, 1, 5 -> (1 + 2) / 2
    r = outliers_reference(magnitudes([5, 1, 1, 5, 1, 5]))
    assert r["stats"]["median_magnitude"] == 3.0 and r["stats"]["mad_magnitude"] == 2.0


def test_checker_mad_zero():
    r = outliers_reference(magnitudes([7.0] * 9))
    assert r["stats"]["mad_magnitude"] == 0.0 and not r["flags"].any()       # 0 / 0 = NaN: not flagged
    r = outliers_reference(magnitudes([7.0] * 5 + [7.5] + [7.0] * 3))
    assert r["stats"]["mad_magnitude"] == 0.0 and list(np.nonzero(r["flags"])[0]) == [5]     # +inf: flagged
    assert r["flags"][5] == 2


def test_checker_include_zeros_changes_the_median():
    v = magnitudes([4.0, 0.0] * 10)
    a, b = outliers_reference(v), outliers_reference(v, True)
    assert (a["stats"]["selected"], b["stats"]["selected"]) == (10, 20)
    assert a["stats"]["median_magnitude"] == 4.0 and b["stats"]["median_magnitude"] == 2.0
    v = magnitudes([1, 2, 3, 4, 100] + [0.0] * 200)
    a, b = outliers_reference(v), outliers_reference(v, True)
    assert list(np.nonzero(a["flags"])[0]) == [4]
    assert list(np.nonzero(b["flags"])[0]) == [0, 1, 2, 3, 4]                # MAD 0 over the zeros: +inf
    assert not a["flags"][5:].any() and not b["flags"][5:].any()


def test_checker_angles_are_not_wrapped():
    """Directions 0.08 rad apart on either side of pi are 6.2 apart as angles: flagged."""
    ang = [3.1] * 20 + [-3.1]
    v = field(np.cos(ang) * 2.0, np.sin(ang) * 2.0)
    r = outliers_reference(v)
    assert list(np.nonzero(r["flags"] & 1)[0]) == [20]
    near = [3.1] * 20 + [3.1 - 0.08]
    r = outliers_reference(field(np.cos(near) * 2.0, np.sin(near) * 2.0))
    assert r["stats"]["mad_angle"] == 0.0 and list(np.nonzero(r["flags"] & 1)[0]) == [20]    # through +inf alone


def test_checker_channels_are_kept_apart():
    ang = np.array([0.3] * 30 + [2.0] + [0.3])
    mag = np.array([2.0] * 31 + [50.0])
    r = outliers_reference(field(mag * np.cos(ang), mag * np.sin(ang)))
    assert r["flags"][30] & 1 and r["flags"][31] & 2 and r["stats"]["outliers"] == np.count_nonzero(r["flags"])


def test_gpu_inputs_hold_both_outcomes():
    for n in SIZES:
        if n < 63:
            continue
        for iz in (False, True):
            f = family_reference("coherent", n, iz)["flags"]
            assert (f & 1).any() and (f & 2).any() and (f == 0).any(), (n, iz)
    for n in SIZES:                                          # m != n, and both parities of m
        assert family_reference("holes", n, False)["stats"]["selected"] == n < len(holes_input(n))
    assert {n % 2 for n in SIZES} == {0, 1}
    for name in BOTH_OUTCOMES:
        f = outliers_reference(HAND_MADE[name]())["flags"]
        assert f.any() and (f == 0).any(), name
    assert not outliers_reference(identical_field())["flags"].any()
    r = outliers_reference(ties_field())
    assert r["stats"]["flagged_magnitude"] == 100 and r["stats"]["median_magnitude"] == 2.0
    r = outliers_reference(split_angles_field())
    assert r["stats"]["median_angle"] == 0.0 and r["stats"]["mad_angle"] > 0.69
    ang = channels(split_angles_field())[0]
    assert np.count_nonzero(ang < 0) == 500 == np.count_nonzero(ang > 0)
    ang = channels(signed_zero_angles_field())[0]
    assert np.all(ang == 0) and 100 < np.count_nonzero(np.signbit(ang)) < 200
    v = denormal_field()
    assert 0 < v[0, 2] * v[0, 2] < np.finfo(np.float64).tiny
    assert outliers_reference(v)["stats"]["flagged_magnitude"] == 2
    mag = np.sort(channels(last_bit_field())[1])
    assert mag[4] == 2.0 and mag[5] == np.nextafter(2.0, 3.0)
    r = outliers_reference(single_active_field())
    assert r["stats"]["selected"] == 1 and not r["flags"].any() and r["stats"]["mad_magnitude"] == 0.0
    r = outliers_reference(no_active_field())
    assert r["stats"]["selected"] == 0 and not r["flags"].any()
    assert outliers_reference(no_active_field(), True)["stats"]["selected"] == 70


def test_batch_fields_differ():
    v = batch_fields(32)
    m = [int(np.count_nonzero((v[b, :, 2] != 0) | (v[b, :, 3] != 0))) for b in range(32)]
    assert len(set(m)) > 16 and {k % 2 for k in m} == {0, 1}         # different m in one call, both parities
    assert all(outliers_reference(v[b])["flags"].any() for b in range(1, 32, 2))


def test_threshold_field_is_exact_to_the_ulp():
    v, edge = threshold_field()
    r = outliers_reference(v)
    assert (r["stats"]["median_magnitude"], r["stats"]["mad_magnitude"]) == (100.0, 2.0)
    assert list(r["flags"][-4:]) == [2, 0, 2, 0] and not r["flags"][:-4].any()
    assert edge[0] == np.nextafter(edge[1], np.inf) and edge[2] == np.nextafter(edge[3], 0.0)
    assert np.array_equal(channels(v)[1][-4:], edge)         # sqrt(x * x) == x: the magnitudes are the edges


def test_abi_struct_and_version(mdx):
    from motion_detection_amd import _lib
    assert C.sizeof(_lib.MdxOutlierStats) == 48 and _lib.ABI_VERSION >= 9
    assert _lib.OUTLIERS_INCLUDE_ZEROS == 1 and _lib.OUTLIERS_MAX_POINTS == 131072
    assert np.dtype(_lib.MdxOutlierStats).itemsize == 48


def test_null_context_is_einval(mdx):
    v = uniform_input(64)
    rc = mdx.lib().mdx_find_outliers(None, v.ctypes.data_as(C.c_void_p), 1, 64, 0, None, None, None)
    assert rc == mdx._lib.MDX_EINVAL


def test_get_outlier_vectors_is_a_gather(mdx):
    """getOutlierVectors reads the probabilities at the grid only, and > 0.5 (:63)."""
    rng = np.random.default_rng(3)
    img = rng.normal(size=(30, 40, 4))
    prob = rng.random((30, 40))
    od = mdx.OutlierDetector.__new__(mdx.OutlierDetector)
    out = od.getOutlierVectors(img, prob, 10)
    exp = np.zeros_like(img)
    for i in range(0, 30, 10):
        for j in range(0, 40, 10):
            if prob[i, j] > 0.5:
                exp[i, j] = img[i, j]
    assert np.array_equal(out, exp) and exp.any()
    with pytest.raises(ValueError):
        od.getOutlierVectors(img, prob[:20], 10)


def test_node_stage_is_off_by_default():
    import inspect

    from motion_detection_amd.node import MotionDetectionNode
    src = inspect.getsource(MotionDetectionNode.__init__)
    assert '"detect_outliers": False' in src and '"include_zeros": False' in src


# ---------------------------------------------------------------- GPU: the device against the checker

AA64 = np.frombuffer(b"\xaa" * 8, np.float64)[0]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def run(ctx, vectors, include_zeros=False):
    """mdx_find_outliers with every output prefilled with 0xAA; what it wrote.  vectors: (n, 4) or
    (batch, n, 4)."""
    from motion_detection_amd._lib import OUTLIERS_INCLUDE_ZEROS, MdxOutlierStats, lib
    vec = np.ascontiguousarray(vectors, np.float64)
    batch, n = (1, vec.shape[0]) if vec.ndim == 2 else vec.shape[:2]
    total = batch * n
    flags = np.full(total + 8, 0xAA, np.uint8)
    out = np.full((total + 1, 4), AA64, np.float64)
    stats = np.frombuffer(bytearray(b"\xaa" * 48 * (batch + 1)), np.dtype(MdxOutlierStats))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = lib().mdx_find_outliers(ctx._h, vp(vec) if total else None, batch, n, OUTLIERS_INCLUDE_ZEROS if include_zeros else 0,
                                 vp(flags), vp(out), vp(stats))
    assert rc == 0, lib().mdx_last_error(ctx._h)
    # nothing is written past the arrays' ends
    assert np.all(flags[total:] == 0xAA) and np.all(bits(out[total:]) == bits(AA64))
    assert stats[batch:].tobytes() == b"\xaa" * 48
    return dict(flags=flags[:total].reshape(batch, n), outlier_vectors=out[:total].reshape(batch, n, 4), stats=stats[:batch])


def same_field(flags, out, st, ref):
    assert np.array_equal(flags, ref["flags"])
    assert np.array_equal(bits(out), bits(ref["outlier_vectors"]))
    for k in STAT_INTS:
        assert int(st[k]) == ref["stats"][k], k
    for k in STAT_DOUBLES:
        got, exp = float(st[k]), ref["stats"][k]
        if k.startswith("median_") and exp == 0.0:
            assert got == 0.0, k                             # a zero median: a value, not a sign
        else:
            assert bits(got) == bits(exp), (k, got, exp)


def same(res, ref, b=0):
    same_field(res["flags"][b], res["outlier_vectors"][b], res["stats"][b], ref)


@pytest.fixture(scope="module", params=["registers", "reread"])
def octx(request, mdx):
    """A context of each kernel variant: fields of up to 4,096 and 24,576 vectors keep their values in
    registers, larger ones re-read them on every pass; MDX_OL_REG=0 (read at mdx_create) makes every
    size re-read."""
    old = os.environ.pop("MDX_OL_REG", None)
    if request.param == "reread":
        os.environ["MDX_OL_REG"] = "0"
    try:
        c = mdx.Context(0, 64, 64, 1)
    finally:
        os.environ.pop("MDX_OL_REG", None)
        if old is not None:
            os.environ["MDX_OL_REG"] = old
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("include_zeros", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_sizes(octx, family, n, include_zeros):
    same(run(octx, FAMILIES[family](n), include_zeros), family_reference(family, n, include_zeros))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4095, 4096, 4097, 24575, 24576, 24577])
def test_variant_edges(octx, n):
    """The sizes at which the launch changes kernel variant (4 values per thread, 24, re-read)."""
    same(run(octx, holes_input(n)[:n], n % 2 == 0), outliers_reference(holes_input(n)[:n], n % 2 == 0))


@pytest.mark.gpu
@pytest.mark.parametrize("include_zeros", [False, True])
def test_1080p_grid(octx, include_zeros):
    ref = family_reference("coherent", 20736, include_zeros)
    assert ref["stats"]["flagged_angle"] > 100 and ref["stats"]["flagged_magnitude"] > 100
    same(run(octx, coherent_input(20736), include_zeros), ref)


@pytest.mark.gpu
def test_max_points(ctx, mdx):
    n = mdx._lib.OUTLIERS_MAX_POINTS
    rng = np.random.default_rng(29000)
    v = field(rng.uniform(-5, 5, n), rng.uniform(-5, 5, n))
    v[::7, 2:] *= 4.0
    v[rng.random(n) < 0.3, 2:] = 0.0
    ref = outliers_reference(v)
    assert 0 < ref["stats"]["outliers"] < ref["stats"]["selected"] < n
    same(run(ctx, v), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("include_zeros", [False, True])
@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_hand_made(octx, name, include_zeros):
    v = HAND_MADE[name]()
    same(run(octx, v, include_zeros), outliers_reference(v, include_zeros))


@pytest.mark.gpu
def test_threshold_to_the_ulp(octx):
    v, _ = threshold_field()
    ref = outliers_reference(v)
    res = run(octx, v)
    same(res, ref)
    assert list(res["flags"][0][-4:]) == [2, 0, 2, 0]         # both outcomes, one ulp apart


def batch_fields(batch, n=2049):
    """Fields of n vectors with different contents and different numbers of active vectors."""
    out = np.zeros((batch, n, 4))
    for b in range(batch):
        rng = np.random.default_rng(27000 + b)
        v = coherent_input(n).copy() if b % 2 else uniform_input(n).copy()
        v[:, 2:] *= 1.0 + 0.25 * b
        v[rng.random(n) < 0.02 * b, 2:] = 0.0
        out[b] = v[rng.permutation(n)]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("include_zeros", [False, True])
@pytest.mark.parametrize("batch", [1, 2, 32])
def test_batch(octx, batch, include_zeros):
    v = batch_fields(batch)
    res = run(octx, v, include_zeros)
    for b in range(batch):
        ref = outliers_reference(v[b], include_zeros)
        same(res, ref, b)
        one = run(octx, v[b], include_zeros)                  # the single-field call
        assert np.array_equal(one["flags"][0], res["flags"][b])
        assert np.array_equal(bits(one["outlier_vectors"][0]), bits(res["outlier_vectors"][b]))
        assert one["stats"][0].tobytes() == res["stats"][b].tobytes()


@pytest.mark.gpu
def test_no_stale_scratch(octx):
    big = np.stack([coherent_input(20736), uniform_input(20736)])
    a = run(octx, big)
    b = run(octx, coherent_input(65), True)
    c = run(octx, holes_input(257))
    d = run(octx, big)
    for r in (a, d):
        same(r, family_reference("coherent", 20736, False), 0)
        same(r, family_reference("uniform", 20736, False), 1)
    same(b, family_reference("coherent", 65, True))
    same(c, family_reference("holes", 257, False))


@pytest.mark.gpu
def test_optional_outputs(ctx):
    """Every output may be NULL; the vectors alone come back right."""
    from motion_detection_amd._lib import lib
    v = coherent_input(257)
    ref = family_reference("coherent", 257, False)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert lib().mdx_find_outliers(ctx._h, vp(v), 1, 257, 0, None, None, None) == 0
    out = np.full((257, 4), AA64)
    assert lib().mdx_find_outliers(ctx._h, vp(v), 1, 257, 0, None, vp(out), None) == 0
    assert np.array_equal(bits(out), bits(ref["outlier_vectors"]))


@pytest.mark.gpu
def test_bad_arguments(ctx, mdx):
    from motion_detection_amd._lib import lib
    E = mdx._lib.MDX_EINVAL
    v = uniform_input(65).copy()
    flags = np.full(65, 0xAA, np.uint8)

    def call(p, batch, n, fl=0, h=ctx._h):
        return lib().mdx_find_outliers(h, None if p is None else p.ctypes.data_as(C.c_void_p), batch, n, fl,
                                       flags.ctypes.data_as(C.c_void_p), None, None)
    assert call(v, 1, 65, h=None) == E
    assert call(v, -1, 65) == E and call(v, 1, -1) == E
    assert call(v, 1, mdx._lib.OUTLIERS_MAX_POINTS + 1) == E
    assert call(v, 1, 65, fl=2) == E and call(v, 1, 65, fl=3) == E and call(v, 1, 65, fl=-1) == E
    assert call(None, 1, 3) == E
    assert call(None, 0, 3) == 0 and call(None, 1, 0) == 0 and call(None, 0, 0) == 0
    for col in range(4):
        for bad in (np.nan, np.inf, -np.inf):
            q = v.copy()
            q[40, col] = bad
            assert call(q, 1, 65) == E
    for col in (2, 3):
        for bad in (1e150, -1e150, 1.7e308):
            q = v.copy()
            q[64, col] = bad
            assert call(q, 1, 65) == E
    assert np.all(flags == 0xAA)                             # a rejected call writes nothing
    q = v.copy()
    q[64, :2] = 1e300                                        # positions are not squared
    q[64, 2] = 9.99e149
    assert call(q, 1, 65) == 0 and call(v, 1, 65, fl=1) == 0
    assert call(v[:64], 2, 32) == 0


@pytest.mark.gpu
def test_context_method(ctx):
    v = coherent_input(257)
    ref = family_reference("coherent", 257, False)
    r = ctx.find_outliers(v)
    assert r.flags.shape == (257,) and r.outlier_vectors.shape == (257, 4) and r.stats.shape == (1,)
    same_field(r.flags, r.outlier_vectors, r.stats[0], ref)
    assert np.array_equal(r.is_outlier, ref["flags"] != 0)
    vb = batch_fields(3, 300)
    r = ctx.find_outliers(vb, include_zeros=True)
    assert r.flags.shape == (3, 300) and r.outlier_vectors.shape == (3, 300, 4) and r.stats.shape == (3,)
    for b in range(3):
        same_field(r.flags[b], r.outlier_vectors[b], r.stats[b], outliers_reference(vb[b], True))
    with pytest.raises(ValueError):
        ctx.find_outliers(np.zeros((5, 3)))


@pytest.mark.gpu
@pytest.mark.parametrize("include_zeros", [False, True])
def test_outlier_detector_mirror(ctx, mdx, include_zeros):
    """findOutliers / getOutlierVectors on a 160 x 120 Vec4d image at pixel_step 10."""
    from motion_detection_amd.flow_clusterer import grid_vectors
    rng = np.random.default_rng(9)
    img = rng.normal(size=(120, 160, 4)) * 50                # off-grid pixels hold junk that must not be read
    for yy in range(0, 120, 10):
        for xx in range(0, 160, 10):
            r = rng.random()
            if r < 0.15:
                img[yy, xx] = (xx, yy, 0, 0)
            elif r < 0.25:
                img[yy, xx] = (xx, yy, rng.uniform(-9, 9), rng.uniform(-9, 9))
            else:
                img[yy, xx] = (xx, yy, 2.0 + rng.normal(0, 0.05), 1.0 + rng.normal(0, 0.05))
    ref = outliers_reference(grid_vectors(img, 10), include_zeros)
    assert 3 < ref["stats"]["outliers"] < 100
    od = mdx.OutlierDetector(context=ctx)
    prob = od.findOutliers(img, include_zeros, 10)
    assert prob.shape == (120, 160) and prob.dtype == np.float64
    exp = np.zeros((120, 160))
    exp[::10, ::10] = (ref["flags"] != 0).reshape(12, 16)
    assert np.array_equal(prob, exp)                         # 1.0 at flagged grid points, off-grid pixels zero
    ov = od.getOutlierVectors(img, prob, 10)
    expv = np.zeros((120, 160, 4))
    expv[::10, ::10] = ref["outlier_vectors"].reshape(12, 16, 4)
    assert ov.shape == (120, 160, 4) and np.array_equal(bits(ov), bits(expv))
    same_field(od.last_outliers.flags, od.last_outliers.outlier_vectors, od.last_outliers.stats[0], ref)
    od.close()
    assert ctx.find_outliers(vecs([(1, 2, 3, 4)])).stats["selected"][0] == 1     # the shared context stays open
