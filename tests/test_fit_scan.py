"""The classify+fit stage where no other test reaches it (mdx_fit.hip).

a) The scan over the 256-point block summaries works in chunks of 64 blocks.  The large parity cases
   (1080p and up, 81 blocks and more) find all four first accepted points in the first blocks of the
   first chunk, the small ones have no second chunk.  Here the first accepted points lie across and
   beyond the chunk boundary (point 16,384 of 19,200), for the first-4 fit, the RANSAC compaction
   (whose block offsets cross the same boundary) and the row bands' records.
b) k_band_fit's merge and its no-fit record on hand-written band records.

The expected values are the CPU oracle's (a) and the contract of include/mdx.h (b).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, PS = 320, 240, 2
NPTS, CHUNK = 19200, 64 * 256           # 160 x 120 grid points, 75 blocks; the second chunk's first point


def _texture():
    t = np.random.default_rng(11).integers(0, 256, (256, 336)).astype(np.float32)
    for _ in range(3):   # 5-point box average
        t = (t + np.roll(t, 1, 0) + np.roll(t, -1, 0) + np.roll(t, 1, 1) + np.roll(t, -1, 1)) / 5
    return np.clip((t - t.mean()) * 6 + 128, 0, 255).astype(np.uint8)


def _scene(py):
    """Flat frames but for one 24 x 40 textured patch at the right edge, moved by (+3, +2): the only
    accepted points are the grid points around it, the first of them near point 16,384."""
    tex = _texture()
    px, pw, ph = 292, 24, 40
    patch = tex[py + 8:py + 8 + ph, px + 8:px + 8 + pw]
    a = np.full((H, W), 128, np.uint8)
    b = a.copy()
    a[py:py + ph, px:px + pw] = patch
    b[py + 2:py + 2 + ph, px + 3:px + 3 + pw] = patch
    return a, b


_refs = {}


def _ref(oracle, py, mode):
    """The oracle's result of a scene, computed once and shared; with the scene's placement checked on
    the oracle's own vectors, so that a scene that drifts fails here instead of testing nothing."""
    if (py, mode) not in _refs:
        a, b = _scene(py)
        kw = dict(fit_mode=2, ransac_iters=32) if mode == "ransac" else {}
        ref = oracle.calculate_optical_flow(a, b, nthreads=8, pixel_step=PS, min_vector_size=1.0, **kw)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _refs[(py, mode)] = (a, b, ref)
    a, b, ref = _refs[(py, mode)]
    acc = np.nonzero((ref["vectors"][:, 2] != 0) | (ref["vectors"][:, 3] != 0))[0]
    assert ref["vectors"].shape[0] == NPTS and acc.size == ref["num_vectors"] >= 4 and ref["fit_status"] == 0
    assert acc[0] >= CHUNK - 3, acc[:4]
    if py == 141:   # two of the first four in block 63, two in block 64
        assert 1 <= np.count_nonzero((acc >= CHUNK - 256) & (acc < CHUNK)) <= 3, acc[:4]
    else:
        assert acc[0] >= CHUNK, acc[:4]
    return a, b, ref


def _same(ref, num, status, next_pts, vectors, Hm, mask, label):
    assert num == ref["num_vectors"], label
    np.testing.assert_array_equal(status, ref["status"], err_msg=label)
    np.testing.assert_array_equal(next_pts.view(np.uint32), ref["next_pts"].view(np.uint32), err_msg=label)
    np.testing.assert_array_equal(vectors.view(np.uint64), ref["vectors"].view(np.uint64), err_msg=label)
    np.testing.assert_array_equal(Hm.view(np.uint64), ref["H"].view(np.uint64), err_msg=label)
    assert int((mask != ref["mask"]).sum()) == 0, label


@pytest.mark.parametrize("mode", ["first4", "ransac"])
@pytest.mark.parametrize("py", [141, 147])
def test_first_four_across_scan_chunks(mdx, oracle, py, mode):
    """First-4 and RANSAC through flow_warp_diff: every output equals the oracle's bit for bit."""
    a, b, ref = _ref(oracle, py, mode)
    kw = dict(fit_mode=mdx.FIT_RANSAC, ransac_iters=32) if mode == "ransac" else dict(fit_mode=mdx.FIT_FIRST4)
    with mdx.Context(0, W, H, 1, pixel_step=PS, min_vector_size=1.0, **kw) as c:
        res = c.flow_warp_diff(a, b)
    assert res.code == mdx.MDX_OK
    _same(ref, res.num_vectors, res.status, res.next_pts, res.vectors, res.H, res.mask, f"py {py} {mode}")


@pytest.mark.parametrize("py", [141, 147])
def test_first_four_across_scan_chunks_row_bands(mdx, oracle, py):
    """Two row bands: the merged records' fit, count, points and mask equal the full path's (the
    oracle's first-4 result)."""
    from motion_detection_amd import rowtile
    a, b, ref = _ref(oracle, py, "first4")
    nb = 2
    with mdx.Context(0, W, H, 1, pixel_step=PS, min_vector_size=1.0) as c:
        d = {k: c.dev_alloc(sz) for k, sz in dict(i1=a.nbytes, i2=b.nbytes, np=NPTS * 8, st=NPTS, vec=NPTS * 32,
                                                   cand=nb * 96, mask=W * H, H=72, num=4).items()}
        try:
            c.h2d(d["i1"], a); c.h2d(d["i2"], b)
            c.h2d(d["vec"], np.zeros(NPTS * 32, np.uint8))
            for r in range(nb):
                y0, y1 = rowtile.band_rows(H, nb, r)
                c.band_flow_dev(d["i1"], d["i2"], W, H, W, mdx.FMT_GRAY8, y0, y1, d["np"], d["st"], d["cand"] + 96 * r,
                                d["vec"])
            for r in range(nb):
                y0, y1 = rowtile.band_rows(H, nb, r)
                c.band_fit_warp_dev(nb, d["cand"], y0, y1, d["mask"] + y0 * W, d["H"], d["num"])
            c.sync()
            out = dict(np=np.empty((NPTS, 2), np.float32), st=np.empty(NPTS, np.uint8), vec=np.empty((NPTS, 4)),
                       mask=np.empty((H, W), np.uint8), H=np.empty((3, 3)), num=np.empty(1, np.int32),
                       cand=np.empty(nb, rowtile.BAND_CAND_DTYPE))
            for k, arr in out.items():
                c.d2h(arr, d[k])
        finally:
            for p in d.values():
                c.dev_free(p)
    assert int(out["cand"]["count"].sum()) == ref["num_vectors"]
    _same(ref, int(out["num"][0]), out["st"], out["np"], out["vec"], out["H"], out["mask"], f"py {py} bands")


def _band_fit(mdx, record_sets):
    """k_band_fit on each set of hand-written records, in one context after a band_flow_dev call:
    per set (H, num_vectors, the band's mask rows, which held 0xFF before the call)."""
    from motion_detection_amd import rowtile
    w, h, ps = 320, 240, 10
    a, b, _ = mdx.synth_pair(9, w, h, 1)
    npts = mdx.grid_count(w, h, ps)
    nrec = max(len(r) for r in record_sets)
    outs = []
    with mdx.Context(0, w, h, 1, pixel_step=ps, min_vector_size=1.0) as c:
        d = {k: c.dev_alloc(sz) for k, sz in dict(i1=a.nbytes, i2=b.nbytes, np=npts * 8, st=npts, cand=96,
                                                   cands=nrec * 96, mask=w * h, H=72, num=4).items()}
        try:
            c.h2d(d["i1"], a); c.h2d(d["i2"], b)
            c.band_flow_dev(d["i1"], d["i2"], w, h, w, mdx.FMT_GRAY8, 0, h, d["np"], d["st"], d["cand"])
            for recs in record_sets:
                assert recs.dtype == rowtile.BAND_CAND_DTYPE
                c.h2d(d["cands"], recs)
                c.h2d(d["mask"], np.full(w * h, 0xFF, np.uint8))
                c.h2d(d["H"], np.full(9, np.nan))
                c.h2d(d["num"], np.full(1, -1, np.int32))
                c.band_fit_warp_dev(len(recs), d["cands"], 0, h, d["mask"], d["H"], d["num"])
                c.sync()
                Hm, num, mask = np.empty(9), np.empty(1, np.int32), np.empty((h, w), np.uint8)
                c.d2h(Hm, d["H"]); c.d2h(num, d["num"]); c.d2h(mask, d["mask"])
                outs.append((Hm, int(num[0]), mask))
        finally:
            for p in d.values():
                c.dev_free(p)
    return outs


def _records(rows):
    """Band records from (count, [(idx, src, dst), ...]) rows; unused slots as k_band_record leaves them."""
    from motion_detection_amd import rowtile
    recs = np.zeros(len(rows), rowtile.BAND_CAND_DTYPE)
    recs["idx"] = -1
    for r, (count, pts) in enumerate(rows):
        recs[r]["count"] = count
        recs[r]["n"] = len(pts)
        for q, (i, s, t) in enumerate(pts):
            recs[r]["idx"][q] = i
            recs[r]["src"][2 * q:2 * q + 2] = s
            recs[r]["dst"][2 * q:2 * q + 2] = t
    return recs


def _pt(i):
    """Grid point i of the 320 x 240, pixel_step 10 grid (x-major) and a destination of its own."""
    s = np.array([(i // 24) * 10, (i % 24) * 10], np.float32)
    return i, s, (s + np.float32([1.5 + 0.25 * (i % 7), -2.0 + 0.125 * (i % 5)])).astype(np.float32)


def test_band_fit_merges_records_out_of_order(mdx, oracle):
    """Three records given out of order, the four smallest indices (2, 5, 7, 9) from different records:
    H is getPerspectiveTransform of exactly those points, num_vectors the sum of the counts."""
    recs = _records([(37, [_pt(5), _pt(9), _pt(40), _pt(41)]), (0, []), (2, [_pt(2), _pt(7)])])
    (Hm, num, _), = _band_fit(mdx, [recs])
    first = [_pt(i) for i in (2, 5, 7, 9)]
    ref = oracle.get_perspective_transform(np.array([p[1] for p in first]), np.array([p[2] for p in first]))
    np.testing.assert_array_equal(Hm.view(np.uint64), ref.ravel().view(np.uint64))
    assert num == 39


def test_band_fit_fewer_than_four_vectors(mdx):
    """Totals 0, 1, 2 and 3 over the records (include/mdx.h, the oracle's fit status 1 / 2): H all
    zero, num_vectors the total, every mask row of the band zero."""
    sets = [_records([(0, []), (0, [])]),
            _records([(0, []), (1, [_pt(30)])]),
            _records([(1, [_pt(8)]), (1, [_pt(3)])]),
            _records([(2, [_pt(50), _pt(51)]), (0, []), (1, [_pt(4)])])]
    for total, (Hm, num, mask) in enumerate(_band_fit(mdx, sets)):
        assert np.array_equal(Hm.view(np.uint64), np.zeros(9, np.uint64)), total
        assert num == total
        assert mask.max() == 0, total
