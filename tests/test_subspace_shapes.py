"""fitSubspace at every legal shape, the mean ladder and the slice counts (mdx_subspace.hip,
mdx_fit_subspace; test_subspace.py runs n - d = 2 only).

n = 2 T rows, d = 4 num_motions sample columns, m = n - d complement columns.  Legal: d <= n <= 32,
m != 10 (the reference's chi_square_table.at(10) throws).  SHAPES = every (T, num_motions) with
2 <= T <= 16, d < n, m != 10: 51 shapes, m = 2 ... 28, which index every entry 1 ... 9 of the
chi-square table and the 0.2 fallback (m > 10).

CPU tests
  * the oracle, both precisions, against a float64 SVD projection (P = I - U_d U_d', res = x'Px)
    within 8 n^2 eps |x|^2 (the bound of test_float_mode_is_float_arithmetic; eps of the mode's
    arithmetic), the winner's inlier count and the outlier flags recomputed from that reference with
    this file's chi-square numbers (P99 of test_subspace.py) away from the thresholds.  Worst
    observed |res - ref| / bound over the 51 shapes: 0.12 (F64), 0.066 (F32);
  * the spike series the mean ladder uses really encodes the order of the float sum.
GPU tests (-m gpu): columns, flags, residual bits, outlier points and the generator's advance
(_gpu_vs_oracle), the per-hypothesis inlier counts (mdx_debug_copy selector 8) and the centred data
with its two means (selector 7), all bit for bit against the oracle.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_subspace import P99, _gpu_vs_oracle, np_mean_subtract, scene_trajectories

SIGMA = 0.5
SHAPES = [(T, nm) for T in range(2, 17) for nm in range(1, 9) if 4 * nm < 2 * T and 2 * T - 4 * nm != 10]
FULL = [(2 * nm, nm) for nm in range(1, 9)]              # n == d: no complement, nothing can be an inlier
# the srand seed per shape at which both modes' winners are d distinct, well-conditioned columns
# (asserted in test_oracle_matches_svd_projection); 1 unless listed
SEEDS = {}
MODES = [0, 1]                                           # MDX_SUBSPACE_F64 / _F32 = the oracle's precision 0 / 1


def test_shape_list():
    assert len(SHAPES) == 51 and len(set(SHAPES)) == 51
    ms = {2 * T - 4 * nm for T, nm in SHAPES}
    assert set(range(2, 10, 2)) <= ms and 10 not in ms and max(ms) == 28 and min(ms) == 2
    assert max(4 * nm for _, nm in SHAPES) == 28 and max(2 * T for T, _ in SHAPES) == 32


@functools.lru_cache(maxsize=None)
def shape_scene(T):
    """3000 trajectories of T points: camera, one object, 40 erratic ones.  Noise 0.2 px keeps the
    d-column samples' condition numbers near 1e4 ... 1e5 up to d = 28 (the scene is two rigid
    motions: rank 6 plus noise)."""
    traj, _ = scene_trajectories(n_bg=2600, n_fg=360, T=T, seed=T, n_bad=40, noise=0.2)
    traj.setflags(write=False)
    return traj


@functools.lru_cache(maxsize=None)
def shape_oracle(T, nm, precision):
    from oracle import pyoracle
    return pyoracle.fit_subspace_counts(shape_scene(T), nm, SIGMA, pyoracle.rand_state(SEEDS.get((T, nm), 1)), precision)


def out_threshold(n, d, sigma):
    """outlier_detector.cpp:311-315 with this file's own copy of the table."""
    return sigma * sigma * P99[n - d] if 0 < n - d < 10 else 0.2


# ------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("T,nm", SHAPES)
def test_oracle_matches_svd_projection(oracle, T, nm, precision):
    n, d = 2 * T, 4 * nm
    traj = shape_scene(T)
    seed = SEEDS.get((T, nm), 1)
    r = shape_oracle(T, nm, precision)
    cols = [int(c) for c in r["columns"]]
    data = np_mean_subtract(traj).astype(np.float64)      # N x n
    # the condition under which the SVD reference is defined: a full-rank, well-conditioned winner
    assert min(cols) >= 0 and len(set(cols)) == d, (T, nm, precision, cols)
    U, s, _ = np.linalg.svd(data[cols].T, full_matrices=True)
    assert s[0] / s[d - 1] < 1e6, (T, nm, precision, s[0] / s[d - 1])
    # the winner is the first hypothesis with the most inliers, and its columns are that draw's
    counts = r["counts"]
    win = int(np.argmax(counts))
    st = oracle.rand_state(seed)
    draws = [oracle.rand(st) for _ in range(50 * d)]
    assert cols == [v % len(traj) for v in draws[win * d:(win + 1) * d]]
    P = np.eye(n) - U[:, :d] @ U[:, :d].T
    ref = np.einsum("ij,jk,ik->i", data, P, data)
    eps = np.finfo(np.float64 if precision == 0 else np.float32).eps
    tol = 8 * n * n * eps * (data ** 2).sum(axis=1)
    err = np.abs(r["residuals"] - ref)
    print(f"T={T} nm={nm} precision={precision}: worst |res - ref| / tol = {float((err / tol).max()):.4g}")
    assert np.all(err <= tol), float((err / tol).max())
    # inliers of the winner: the count is the number of returned residuals under the threshold,
    # and those decisions are the reference's wherever the reference is clear of the threshold
    in_thr = (n - d) * SIGMA * SIGMA
    assert int(counts[win]) == int((r["residuals"] < in_thr).sum())
    clear = np.abs(ref - in_thr) > tol
    np.testing.assert_array_equal((r["residuals"] < in_thr)[clear], (ref < in_thr)[clear])
    lo = int((ref < in_thr)[clear].sum())
    assert lo <= int(counts[win]) <= lo + int((~clear).sum())
    # outlier flags against the table entry n - d (or 0.2)
    thr = out_threshold(n, d, SIGMA)
    clear = np.abs(ref - thr) > tol
    np.testing.assert_array_equal(r["is_outlier"][clear], (ref > thr)[clear].astype(np.uint8))
    assert r["n_outliers"] == int(r["is_outlier"].sum())
    if precision == 0:            # double: the bound is far below the thresholds, every decision is checked
        assert clear.sum() >= len(traj) - 5 and 0 < int(r["is_outlier"].sum()) < len(traj)


def test_counts_variant_changes_no_result(oracle):
    traj = shape_scene(5)
    for precision in MODES:
        a = oracle.fit_subspace(traj, 2, SIGMA, oracle.rand_state(3), precision)
        sb = oracle.rand_state(3)
        b = oracle.fit_subspace_counts(traj, 2, SIGMA, sb, precision)
        for k in ("columns", "is_outlier"):
            np.testing.assert_array_equal(a[k], b[k])
        np.testing.assert_array_equal(a["residuals"].view(np.uint64), b["residuals"].view(np.uint64))
        assert a["n_outliers"] == b["n_outliers"] and b["counts"].min() >= 0 and b["counts"].max() <= len(traj)
        sa = oracle.rand_state(3)
        oracle.fit_subspace(traj, 2, SIGMA, sa, precision)
        assert bytes(sa) == bytes(sb)


# --- the mean ladder's inputs
LADDER_GROUPS = {
    "1-100": list(range(1, 101)),
    "101-200": list(range(101, 201)),
    "4090-4145": list(range(4090, 4146)),
    "4146-4200": list(range(4146, 4201)),
    "8185-8222": list(range(8185, 8223)),
    "8223-8260": list(range(8223, 8261)),
    "chunks": [12288, 12289, 12335, 16431],
}
LADDER_NS = [N for g in LADDER_GROUPS.values() for N in g]
SPIKE = np.float32(2.0 ** 25)


def spike_positions(N):
    return sorted({p for p in (N // 3, N - 17, N - 1) if p >= 0})


def spike_series(N, pos):
    """T = 3 trajectories whose first points make the sequential float32 sums depend on the order:
    x: 1.5 everywhere, 2^25 at pos.  Before the spike the sum is exact (1.5 k); from the spike on the
    spacing is 4 and every further 1.5 is absorbed, so the sum is 2^25 + 1.5 * (elements before the
    spike), rounded to a multiple of 4.  y: 2.5 and the same spike: every later 2.5 rounds up to 4,
    so the y sum also counts the elements after the spike.  The other points are ordinary."""
    rng = np.random.default_rng(N)
    traj = rng.uniform(0, 64, (N, 3, 2)).astype(np.float32)
    traj[:, 0, 0] = 1.5
    traj[:, 0, 1] = 2.5
    traj[pos, 0] = SPIKE
    return traj


def ladder_scene(N):
    traj, _ = scene_trajectories(n_bg=N, n_fg=0, T=3, seed=N % 97)
    return traj


def ladder_inputs(N):
    return [spike_series(N, p) for p in spike_positions(N)] + [ladder_scene(N)]


def seq_means(traj):
    """np_mean_subtract's two means (sequential float32 sums of the first points, the division in
    double), with the sums taken by numpy's accumulate, which adds in index order."""
    N = len(traj)
    xs = np.add.accumulate(traj[:, 0, 0], dtype=np.float32)[-1]
    ys = np.add.accumulate(traj[:, 0, 1], dtype=np.float32)[-1]
    return np.array([np.float32(float(xs) / N), np.float32(float(ys) / N)], np.float32)


def seq_sum(v):
    return np.add.accumulate(np.asarray(v, np.float32), dtype=np.float32)[-1]


def test_ladder_ns():
    assert set(range(1, 201)) | set(range(4090, 4201)) | set(range(8185, 8261)) | {12288, 12289, 12335, 16431} \
        == set(LADDER_NS) and len(LADDER_NS) == len(set(LADDER_NS))


def test_spike_series_is_order_sensitive():
    """Meta-check: moving the spike by 16 places (one block of the device's pipelined sum) changes
    both sequential sums, for every N of the ladder that has 16 places to move by; and a spike
    series' sum differs from the sum without the spike's predecessors counted."""
    for N in LADDER_NS:
        if N < 17:
            continue
        assert N - 1 in spike_positions(N)             # which always has 16 places below it
        for p in spike_positions(N):
            q = p - 16 if p >= 16 else p + 16
            if q >= N:
                continue
            a, b = spike_series(N, p), spike_series(N, q)
            assert seq_sum(a[:, 0, 0]) != seq_sum(b[:, 0, 0]), (N, p, q)
            assert seq_sum(a[:, 0, 1]) != seq_sum(b[:, 0, 1]), (N, p, q)


@pytest.mark.parametrize("group", list(LADDER_GROUPS))
def test_ladder_references_agree(oracle, group):
    """seq_means (what the GPU's means are compared with) are np_mean_subtract's means, and the
    oracle's centred data is np_mean_subtract's, byte for byte, on every input of the ladder."""
    for N in LADDER_GROUPS[group]:
        for traj in ladder_inputs(N):
            ref = np_mean_subtract(traj)
            np.testing.assert_array_equal(oracle.subspace_data(traj).view(np.uint32), ref.view(np.uint32))
            xc, yc = seq_means(traj)
            d = traj.reshape(N, 6).copy()
            d[:, 0::2] = d[:, 0::2] - xc
            d[:, 1::2] = yc - d[:, 1::2]
            np.testing.assert_array_equal(d.view(np.uint32), ref.view(np.uint32))


# (T, num_motions, ntraj): n - d == 10 three times, d > n twice, n > 32, no trajectory, no motion
REJECTED = [(7, 1, 50), (9, 2, 50), (13, 4, 50), (5, 3, 50), (2, 2, 50), (17, 2, 50), (5, 2, 0), (5, 0, 50)]


def test_rejected_arguments_oracle(oracle):
    for T, nm, N in REJECTED:
        traj = np.ones((N, T, 2), np.float32)
        for precision in MODES:
            st = oracle.rand_state(9)
            before = bytes(st)
            r = oracle.fit_subspace_counts(traj, nm, SIGMA, st, precision)
            assert r["n_outliers"] == -1 and bytes(st) == before, (T, nm, N)
            assert np.all(r["counts"] == -1) and np.all(r["columns"] == -1)


# ------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctxs(mdx):
    cs = {0: mdx.Context(0, 64, 64, 1, subspace_precision=mdx.SUBSPACE_F64),
          1: mdx.Context(0, 64, 64, 1, subspace_precision=mdx.SUBSPACE_F32)}
    yield cs
    for c in cs.values():
        c.close()


def gpu_counts(mdx, c):
    cnt = np.full(50, -7, np.int32)
    assert mdx.lib().mdx_debug_copy(c._h, 8, cnt.ctypes.data_as(C.c_void_p), cnt.nbytes) == 0
    return cnt


def gpu_data(mdx, c, N, n):
    """selector 7: the centred data (N, n) and the two means."""
    buf = np.full(N * n + 2, np.nan, np.float32)
    assert mdx.lib().mdx_debug_copy(c._h, 7, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 0
    return buf[:N * n].reshape(N, n), buf[N * n:]


@pytest.mark.gpu
def test_gpu_selectors_need_a_fit(mdx):
    """Selectors 7 and 8 before any mdx_fit_subspace on the context: an error, nothing copied; after
    one: at most the buffer's bytes, however many are asked for."""
    with mdx.Context(0, 64, 64, 1) as c:
        buf = np.full(64, 7, np.int32)
        for which in (7, 8):
            assert mdx.lib().mdx_debug_copy(c._h, which, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == mdx._lib.MDX_EINVAL
            assert b"unavailable" in mdx.lib().mdx_last_error(c._h) and np.all(buf == 7)
        ps = mdx._lib.MdxRandState()
        mdx.lib().mdx_srand(C.byref(ps), 1)
        c.fit_subspace(shape_scene(3)[:40], 1, SIGMA, ps)
        assert mdx.lib().mdx_debug_copy(c._h, 8, buf.ctypes.data_as(C.c_void_p), buf.nbytes) == 0
        assert np.all(buf[:50] >= 0) and np.all(buf[:50] <= 40) and np.all(buf[50:] == 7)


def gpu_vs_oracle_counts(mdx, c, oracle, traj, nm, sigma, seed, precision, ref=None):
    g = _gpu_vs_oracle(mdx, c, oracle, traj, nm, sigma, seed, precision)
    if ref is None:
        ref = oracle.fit_subspace_counts(traj, nm, sigma, oracle.rand_state(seed), precision)
    np.testing.assert_array_equal(gpu_counts(mdx, c), ref["counts"])
    return g, ref


@pytest.mark.gpu
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("T,nm", SHAPES)
def test_gpu_every_shape(mdx, ctxs, oracle, T, nm, precision):
    g, r = gpu_vs_oracle_counts(mdx, ctxs[precision], oracle, shape_scene(T), nm, SIGMA, SEEDS.get((T, nm), 1),
                                precision, ref=shape_oracle(T, nm, precision))
    assert r["counts"].max() > 0 and g.columns.min() >= 0


@pytest.mark.gpu
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("T,nm", FULL)
def test_gpu_full_dimension_has_no_inliers(mdx, ctxs, oracle, T, nm, precision):
    """n == d: the inlier bound (n - d) sigma^2 is 0 and residual < 0 never holds."""
    traj = shape_scene(T)[:700]
    g, r = gpu_vs_oracle_counts(mdx, ctxs[precision], oracle, traj, nm, SIGMA, 2, precision)
    assert np.all(g.columns == -1) and np.all(g.residuals == 0.0) and not g.is_outlier.any()
    assert len(g.outlier_points) == 0 and np.all(gpu_counts(mdx, ctxs[precision]) == 0)
    # _gpu_vs_oracle has checked that the generator advanced by 50 * d draws


@pytest.mark.gpu
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("T,nm,N", REJECTED)
def test_gpu_rejected_arguments(mdx, ctxs, oracle, T, nm, N, precision):
    c = ctxs[precision]
    traj = np.ones((max(N, 1), T, 2), np.float32)
    ps = mdx._lib.MdxRandState()
    mdx.lib().mdx_srand(C.byref(ps), 9)
    before = bytes(ps)
    d = max(4 * nm, 1)
    cols, out, res = np.zeros(d, np.int32), np.zeros(max(N, 1), np.uint8), np.zeros(max(N, 1), np.float64)
    pts, nout = np.zeros((max(N, 1), 2), np.float32), C.c_int(0)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = mdx.lib().mdx_fit_subspace(c._h, vp(traj), N, T, nm, SIGMA, C.byref(ps), vp(cols), vp(out), vp(res), vp(pts),
                                    C.byref(nout))
    assert rc == mdx._lib.MDX_EINVAL
    assert b"mdx_fit_subspace" in mdx.lib().mdx_last_error(c._h)
    assert bytes(ps) == before
    st = oracle.rand_state(9)
    ob = bytes(st)
    assert oracle.fit_subspace(traj[:N], nm, SIGMA, st, precision)["n_outliers"] == -1 and bytes(st) == ob


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(LADDER_GROUPS))
def test_gpu_mean_ladder(mdx, ctxs, oracle, group):
    """k_subspace_prep's pipelined sum at every drain branch, pre-alignment length and chunk count:
    the centred data and the two means, byte for byte."""
    c = ctxs[0]
    for N in LADDER_GROUPS[group]:
        for traj in ladder_inputs(N):
            ps = mdx._lib.MdxRandState()
            mdx.lib().mdx_srand(C.byref(ps), 1)
            c.fit_subspace(traj, 1, SIGMA, ps)
            data, mean = gpu_data(mdx, c, N, 6)
            np.testing.assert_array_equal(mean.view(np.uint32), seq_means(traj).view(np.uint32), err_msg=f"N={N}")
            np.testing.assert_array_equal(data.view(np.uint32), oracle.subspace_data(traj).view(np.uint32),
                                          err_msg=f"N={N}")


@pytest.mark.gpu
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("N", [1023, 1024, 2047, 2048, 2049, 3071, 3073, 16383, 16384, 16385, 40001])
def test_gpu_slice_edges(mdx, ctxs, oracle, N, precision):
    """S = min(16, N / 1024) slices [N y / S, N (y + 1) / S): every trajectory counted once."""
    n_fg, n_bad = N // 8, N // 50
    traj, _ = scene_trajectories(n_bg=N - n_fg - n_bad, n_fg=n_fg, T=5, seed=N % 89, n_bad=n_bad)
    assert len(traj) == N
    _, r = gpu_vs_oracle_counts(mdx, ctxs[precision], oracle, traj, 2, SIGMA, 3, precision)
    assert r["counts"].max() > N // 2        # most trajectories are inliers: an edge one is, too


@pytest.mark.gpu
def test_gpu_modes_alternate_on_one_context(mdx, oracle):
    """One context, subspace_precision switched between calls: the basis scratch is sized per call
    from the mode's own layout.  Per hypothesis (T = 5, nm = 2) needs 160 B in F64 and 400 B in F32,
    (T = 16, nm = 1) 7168 B and 4096 B; each mode's larger need follows its smaller one, and the
    first three calls each outgrow the buffer the call before left."""
    with mdx.Context(0, 64, 64, 1) as c:
        for precision, (T, nm) in [(0, (5, 2)), (1, (5, 2)), (0, (16, 1)), (1, (16, 1))]:
            c.set_params(subspace_precision=precision)
            _, r = gpu_vs_oracle_counts(mdx, c, oracle, shape_scene(T)[:300], nm, SIGMA, 1, precision)
            assert r["counts"].max() > 0 and r["columns"].min() >= 0      # a winner's basis was read back


# --- float edges
@pytest.mark.gpu
def test_gpu_float_mode_subnormal_residuals(mdx, ctxs, oracle):
    """F32 mode on a scene scaled by 1e-19: every winner residual is a nonzero float subnormal on
    the host; a device that flushed them would return zeros."""
    traj, _ = scene_trajectories(seed=5)
    traj = (traj.astype(np.float64) * 1e-19).astype(np.float32)
    g, r = gpu_vs_oracle_counts(mdx, ctxs[1], oracle, traj, 2, 0.5e-19, 4, 1)
    res = r["residuals"]
    tiny = float(np.finfo(np.float32).tiny)
    assert r["columns"].min() >= 0 and np.all(res > 0) and np.all(res < tiny), (res.min(), res.max())


def nan_aware_vs_oracle(mdx, c, oracle, traj, nm, sigma, seed, precision):
    """_gpu_vs_oracle with NaN residuals compared as "both NaN" (payloads may differ between host
    and device), everything else by bits."""
    ps = mdx._lib.MdxRandState()
    mdx.lib().mdx_srand(C.byref(ps), seed)
    g = c.fit_subspace(traj, nm, sigma, ps)
    st = oracle.rand_state(seed)
    r = oracle.fit_subspace_counts(traj, nm, sigma, st, precision)
    np.testing.assert_array_equal(g.columns, r["columns"])
    np.testing.assert_array_equal(g.is_outlier, r["is_outlier"])
    gn, rn = np.isnan(g.residuals), np.isnan(r["residuals"])
    np.testing.assert_array_equal(gn, rn)
    np.testing.assert_array_equal(g.residuals[~gn].view(np.uint64), r["residuals"][~rn].view(np.uint64))
    np.testing.assert_array_equal(g.outlier_points, traj[r["is_outlier"].astype(bool), traj.shape[1] - 2])
    np.testing.assert_array_equal(gpu_counts(mdx, c), r["counts"])
    assert mdx.lib().mdx_rand(C.byref(ps)) == oracle.rand(st)
    return g, r


@pytest.mark.gpu
@pytest.mark.parametrize("precision", MODES)
def test_gpu_nan_in_one_trajectory(mdx, ctxs, oracle, precision):
    """A NaN in a middle point: that trajectory's residual is NaN (neither inlier nor outlier), a
    hypothesis that sampled it has no inlier, the rest is untouched."""
    traj, _ = scene_trajectories(n_bg=180, n_fg=20, seed=6)
    traj = traj.copy()
    traj[77, 2, 1] = np.nan
    g, r = nan_aware_vs_oracle(mdx, ctxs[precision], oracle, traj, 2, SIGMA, 5, precision)
    st = oracle.rand_state(5)
    hit = [77 in [oracle.rand(st) % 200 for _ in range(8)] for _ in range(50)]
    assert any(hit) and not all(hit)                       # both kinds of hypothesis ran
    assert np.all(r["counts"][np.array(hit)] == 0) and r["counts"].max() > 0
    assert np.isnan(g.residuals[77]) and np.isnan(g.residuals).sum() == 1 and not g.is_outlier[77]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", MODES)
def test_gpu_nan_mean(mdx, ctxs, oracle, precision):
    """A NaN in trajectory 0's first point: NaN mean, every residual NaN, no fit."""
    traj, _ = scene_trajectories(n_bg=180, n_fg=20, seed=6)
    traj = traj.copy()
    traj[0, 0, 0] = np.nan
    g, _ = gpu_vs_oracle_counts(mdx, ctxs[precision], oracle, traj, 2, SIGMA, 5, precision)
    assert np.all(g.columns == -1) and np.all(g.residuals == 0.0) and not g.is_outlier.any()
    assert np.all(gpu_counts(mdx, ctxs[precision]) == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", MODES)
def test_gpu_static_trajectories(mdx, ctxs, oracle, precision):
    """Every trajectory stands still: the centred data has rank 2, the later reflectors work on
    rounding residue or exact zeros (beta == 0 skips one)."""
    rng = np.random.default_rng(8)
    p = rng.uniform(10, 600, (300, 1, 2)).astype(np.float32)
    gpu_vs_oracle_counts(mdx, ctxs[precision], oracle, np.repeat(p, 5, axis=1), 2, SIGMA, 6, precision)
    # whole-pixel positions: the sums, the mean's quotient aside, are exact
    gpu_vs_oracle_counts(mdx, ctxs[precision], oracle, np.repeat(np.rint(p), 5, axis=1), 2, SIGMA, 6, precision)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", MODES)
def test_gpu_identical_trajectories(mdx, ctxs, oracle, precision):
    """100 copies of one trajectory.  Of a moving one: a rank-1 sample.  Of the constant (3, 3): the
    mean is exact, the centred data is all zero, every beta is 0 and every reflector is skipped --
    the residuals are exact zeros and every hypothesis counts all 100 (0 / 0 otherwise: none)."""
    rng = np.random.default_rng(9)
    one = rng.uniform(10, 600, (1, 5, 2)).astype(np.float32)
    gpu_vs_oracle_counts(mdx, ctxs[precision], oracle, np.repeat(one, 100, axis=0), 2, SIGMA, 7, precision)
    zero = np.full((100, 5, 2), 3.0, np.float32)
    g, r = gpu_vs_oracle_counts(mdx, ctxs[precision], oracle, zero, 2, SIGMA, 7, precision)
    assert np.all(r["counts"] == 100) and np.all(g.residuals == 0.0) and not g.is_outlier.any()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", MODES)
@pytest.mark.parametrize("N", [1, 2, 3, 9])
def test_gpu_fewer_trajectories_than_columns(mdx, ctxs, oracle, N, precision):
    """N < d = 16: every sample repeats columns."""
    traj, _ = scene_trajectories(n_bg=N, n_fg=0, T=9, seed=N)
    gpu_vs_oracle_counts(mdx, ctxs[precision], oracle, traj, 4, SIGMA, 8, precision)
