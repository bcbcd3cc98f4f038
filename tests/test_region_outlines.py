"""The outer border polyline of each mask region on the device (mdx_region_outlines_dev /
mdx_mask_region_outlines): what getMotionContours' findContours(CV_RETR_EXTERNAL,
CV_CHAIN_APPROX_NONE) returns for a blob (common/src/background_subtractor.cpp:31-35).  Restated from the
border-following algorithm; unpinned against a real build like the rest of the recipe.

Two checkers, written from include/mdx.h; neither shares anything with the kernels, which never walk:
  Walker.trace   the sequential tracer, literally "The tracing rule": look around from b+1, step, repeat
                 until the start state returns.
  Walker.crack   crack following: walk the pixel edges with the blob on the left, turn right whenever the
                 ahead-right pixel is a member, else straight on if the ahead-left one is, else left; the
                 pixel to the left of each crack, consecutive repeats dropped.
Everything is integer and exact: every output buffer is prefilled with 0xAA words and every word is compared.
"""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_region_parents import NO_PARENT, nested_outlines, parents_by_rule, u8
from test_regions import AA, OPEN3, ROOT, SIZES, big_random, patterns, regions_reference

D = [(1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1)]   # E NE N NW W SW S SE


# ---------------------------------------------------------------- the checkers

class Walker:
    """A label image with one ring of -1 around it, as a flat list: everything that is not a member of a
    record with id >= 0 -- other regions, background, the outside of the frame -- compares unequal."""

    def __init__(self, labels):
        labels = np.asarray(labels)
        self.h, self.w = labels.shape
        self.W2 = self.w + 2
        self.L = np.pad(labels, 1, constant_values=-1).ravel().tolist()
        self.off = [dy * self.W2 + dx for dx, dy in D]

    def _ok(self, sx, sy, cid):
        return 0 <= sx < self.w and 0 <= sy < self.h and cid >= 0 and self.L[(sy + 1) * self.W2 + sx + 1] == cid

    def _xy(self, cells):
        return [(p % self.W2 - 1, p // self.W2 - 1) for p in cells]

    def trace(self, rec):
        sx, sy, cid = int(rec[5]), int(rec[6]), int(rec[7])
        if not self._ok(sx, sy, cid):
            return []
        L, off = self.L, self.off
        p0 = (sy + 1) * self.W2 + sx + 1
        b0 = next((d for d in (3, 2, 1, 0, 7, 6, 5, 4) if L[p0 + off[d]] == cid), None)
        if b0 is None:
            return [(sx, sy)]
        out, p, b = [], p0, b0
        while True:
            out.append(p)
            for i in range(1, 9):
                t = (b + i) & 7
                if L[p + off[t]] == cid:
                    break
            p, b = p + off[t], t ^ 4
            if p == p0 and b == b0:
                return self._xy(out)

    def crack(self, rec):
        """Only for a seed that is the component's first pixel: its left edge is then a crack of the outer border."""
        sx, sy, cid = int(rec[5]), int(rec[6]), int(rec[7])
        if not self._ok(sx, sy, cid):
            return []
        L, W2 = self.L, self.W2

        def px(cx, cy, ax, ay):          # the pixel whose centre is corner + (ax, ay) / 2, as a padded index
            return (cy + (ay - 1) // 2 + 1) * W2 + cx + (ax - 1) // 2 + 1
        cx, cy, vx, vy = sx, sy, 0, 1    # at the seed's top left corner, heading south: the blob lies to the left
        owners = []
        while True:
            lx, ly = vy, -vx
            owners.append(px(cx, cy, vx + lx, vy + ly))
            cx, cy = cx + vx, cy + vy
            if L[px(cx, cy, vx - lx, vy - ly)] == cid:       # ahead right
                vx, vy = -lx, -ly
            elif L[px(cx, cy, vx + lx, vy + ly)] != cid:     # not ahead left either
                vx, vy = lx, ly
            if (cx, cy, vx, vy) == (sx, sy, 0, 1):
                break
        out = [owners[0]]
        for p in owners[1:]:
            if p != out[-1]:
                out.append(p)
        while len(out) > 1 and out[-1] == out[0]:
            out.pop()
        return self._xy(out)


def outlines_of(labels, recs, how="trace"):
    wk = Walker(labels)
    return [getattr(wk, how)(r) for r in np.asarray(recs).reshape(-1, 8)]


def case(mask, open3=False, min_area=1):
    ref = regions_reference(mask, open3=open3, min_area=min_area)
    ref["outlines"] = outlines_of(ref["labels"], ref["kept"])
    return ref


def first(mask):
    """The outline of a mask's first component, as a list of [x, y]."""
    return [list(p) for p in case(u8(np.array(mask)))["outlines"][0]]


def spiral(w, h):
    """A one-pixel-wide rectangular spiral with a one-pixel gap between its turns: straight on while the pixel
    two ahead is free, else one turn to the right, else done."""
    m = np.zeros((h, w), bool)
    x, y, dx, dy = 0, 0, 1, 0
    m[0, 0] = True
    free = lambda u, v: not (0 <= u < w and 0 <= v < h and m[v, u])   # noqa: E731
    while True:
        for _ in range(2):
            nx, ny = x + dx, y + dy
            if 0 <= nx < w and 0 <= ny < h and free(nx, ny) and free(nx + dx, ny + dy):
                break
            dx, dy = -dy, dx
        else:
            return u8(m)
        x, y = nx, ny
        m[y, x] = True


def islands(w, h):
    """Thick nested rings with single pixels in the gaps between them: holes that are not traced, islands that
    are records of their own."""
    y, x = np.mgrid[0:h, 0:w]
    inset = np.minimum(np.minimum(x, w - 1 - x), np.minimum(y, h - 1 - y))
    return u8((inset % 8 < 3) | ((inset % 8 == 5) & (x % 3 == 0) & (y % 3 == 0)))


def edge_blob(w, h):
    """One blob that touches all four frame edges and has holes: a frame-wide grid of bars."""
    y, x = np.mgrid[0:h, 0:w]
    return u8((x % 5 == 0) | (y % 4 == 0) | (x == w - 1) | (y == h - 1))


def shapes(w, h):
    p = dict(patterns(w, h))
    y, x = np.mgrid[0:h, 0:w]
    p.update(spiral=spiral(w, h), islands=islands(w, h), edge_blob=edge_blob(w, h), diagonal_line=u8(x == y),
             nested=nested_outlines(0) if (w, h) == (130, 67) else u8((x + 2 * y) % 7 < 3))
    return p


# ---------------------------------------------------------------- CPU: the checkers, the step function, the interface

def test_hand_answers():
    assert first([[1, 1], [1, 1]]) == [[0, 0], [0, 1], [1, 1], [1, 0]]
    assert first([[1, 1, 1]]) == [[0, 0], [1, 0], [2, 0], [1, 0]]
    assert first([[0, 1], [1, 1]]) == [[1, 0], [0, 1], [1, 1]]
    assert first([[0, 0, 0], [0, 1, 0]]) == [[1, 1]]
    assert first([[1, 0], [0, 1]]) == [[0, 0], [1, 1]]
    x = first([[1, 0, 1], [0, 1, 0], [1, 0, 1]])
    assert x == [[0, 0], [1, 1], [0, 2], [1, 1], [2, 2], [1, 1], [2, 0], [1, 1]] and x.count([1, 1]) == 4
    # a hole is not traced, an island in it is a record of its own
    ring = np.ones((5, 5), np.uint8)
    ring[1:4, 1:4] = 0
    ring[2, 2] = 1
    ref = case(u8(ring))
    assert [len(o) for o in ref["outlines"]] == [16, 1] and ref["outlines"][1] == [(2, 2)]
    assert ref["outlines"][0][:6] == [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 4)]   # down the left side first


def test_untrusted_records_in_the_checker():
    ref = case(u8(np.ones((3, 4))))
    rec = ref["kept"][0].copy()
    for edit in ([5, 4], [5, -1], [6, 3], [7, 1], [7, -1]):
        r = rec.copy()
        r[edit[0]] = edit[1]
        assert outlines_of(ref["labels"], [r]) == [[]]
    r = rec.copy()
    r[5:7] = [1, 1]                                            # an inner pixel: a cycle of its own, finite
    assert len(outlines_of(ref["labels"], [r])[0]) == 8
    r[5:7] = [0, 1]                                            # on the left side, entered from above: the same ring from there
    o = outlines_of(ref["labels"], [r])[0]
    assert o == ref["outlines"][0][1:] + ref["outlines"][0][:1]
    r[5:7] = [3, 2]                                            # a border pixel whose start state the outline does not pass
    o = outlines_of(ref["labels"], [r])[0]
    assert o[0] == (3, 2) and 0 < len(o) != len(ref["outlines"][0])


def _small_masks():
    rng = np.random.default_rng(7)
    for bits in range(1, 1 << 12):                             # every 3 x 4 mask
        yield np.array([(bits >> i) & 1 for i in range(12)], np.uint8).reshape(3, 4)
    for bits in rng.choice(1 << 16, 1500, replace=False):      # a sample of the 4 x 4 ones (the device does them all)
        yield np.array([(int(bits) >> i) & 1 for i in range(16)], np.uint8).reshape(4, 4)
    for _ in range(150):
        w, h = rng.integers(1, 12, 2)
        yield (rng.random((h, w)) < rng.choice([0.3, 0.5, 0.7, 0.9])).astype(np.uint8)


def test_checkers_agree_and_the_outline_is_the_border_to_the_enclosing_background():
    n = 0
    for m in _small_masks():
        ref = regions_reference(u8(m), open3=False)
        lab = ref["labels"]
        a, b = outlines_of(lab, ref["kept"]), outlines_of(lab, ref["kept"], "crack")
        assert a == b, m
        # the background, padded by the outside of the frame, as 4-connected components
        bgl = regions_reference(u8(np.pad(lab < 0, 1, constant_values=True)), open3=False, connectivity=4)["labels"]
        for rec, o in zip(ref["kept"], a):
            enclosing = bgl[rec[6], rec[5] + 1]                # the pixel above the seed, padded coordinates
            assert enclosing >= 0
            near = np.zeros(lab.shape, bool)
            for dx, dy in ((1, 0), (0, -1), (-1, 0), (0, 1)):
                near |= bgl[1 + dy:1 + dy + lab.shape[0], 1 + dx:1 + dx + lab.shape[1]] == enclosing
            ys, xs = np.nonzero((lab == rec[7]) & near)
            assert sorted(set(o)) == sorted(zip(xs.tolist(), ys.tolist())), m
            assert len(o) <= max(1, 4 * rec[4])
            n += 1
    assert n > 8000


def test_checkers_agree_on_patterns():
    for w, h in [(1, 1), (97, 1), (1, 97), (7, 5), (33, 31)]:
        for name, m in shapes(w, h).items():
            ref = regions_reference(m, open3=False)
            assert outlines_of(ref["labels"], ref["kept"]) == outlines_of(ref["labels"], ref["kept"], "crack"), (name, w, h)
    ref = case(spiral(33, 31))
    # every pixel twice but the two ends, and once less per corner: the inner pass cuts it
    assert ref["num_all"] == 1 and 2 * ref["kept"][0, 4] - 2 - 31 <= len(ref["outlines"][0]) < 2 * ref["kept"][0, 4] - 2
    assert case(edge_blob(33, 31))["num_all"] == 1


def test_shared_step_function_for_all_inputs(tmp_path):
    """mdx_plan.h's outline_next_dir / outline_prev_dir / outline_dx / outline_dy, compiled for the host, against
    the tracer's inner loop for all 256 x 8 inputs."""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "outline_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "motion_detection_amd", "csrc"), "-I",
                    os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "outline_check.cpp"), "-o", exe], check=True)
    got = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in got[:16]] == [c for d in D for c in d]
    got = [int(v) for v in got[16:]]
    want = []
    for mask in range(256):
        for b in range(8):
            nxt = next((((b + i) & 7) for i in range(1, 9) if mask >> ((b + i) & 7) & 1), -1)
            prv = next((((b - i) & 7) for i in range(1, 9) if mask >> ((b - i) & 7) & 1), -1)
            want += [nxt, prv]
    assert got == want
    # the inverse: the state that steps from p in direction t is (p, prev_dir(mask, t))
    for mask in range(1, 256):
        for t in range(8):
            if mask >> t & 1:
                assert want[2 * (mask * 8 + want[2 * (mask * 8 + t) + 1])] == t
    assert [int(v) for v in subprocess.run([exe, "rounds"], check=True, capture_output=True,
                                           text=True).stdout.split()] == [3, 21, 24, 26]


def test_header_and_binding_declare_both_entries(mdx):
    from test_abi import HEADER, header_functions
    names = header_functions()
    for n in ("mdx_region_outlines_dev", "mdx_mask_region_outlines"):
        assert n in names and n in mdx._lib.EXPORTED
    assert sorted(mdx._lib.EXPORTED) == names
    hdr = open(HEADER).read()
    assert int(re.search(r"#define MDX_ABI_VERSION (\d+)", hdr).group(1)) == mdx._lib.ABI_VERSION == 11
    assert "no contour polylines" not in hdr
    assert "mdx_outline.hip" in mdx._lib.STAMPED


def test_null_context_is_einval(mdx):
    L = mdx.lib()
    m = np.zeros((4, 4), np.uint8)
    off = np.zeros(16, np.int32)
    n = C.c_int(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert L.mdx_region_outlines_dev(None, 1, p(off), 4, 4, None, 0, None, p(off), None, 0, None) == mdx._lib.MDX_EINVAL
    assert L.mdx_mask_region_outlines(None, p(m), 4, 4, 4, OPEN3, 1, None, 0, C.byref(n), C.byref(n), None, None, None,
                                      p(off), None, 0, C.byref(n)) == mdx._lib.MDX_EINVAL


def test_outlines_field_defaults(mdx):
    z = np.zeros((0, 8), np.int32)
    assert mdx.RegionResult(z, 0, 0).outlines is None and mdx.RegionTreeResult(z, 0, 0).outlines is None
    assert mdx.RegionResult(z, 0, 0, None, None).outlines is None


# ---------------------------------------------------------------- GPU: through the C-ABI

def run_outlines(c, masks, open3=False, min_area=1, max_regions=None, max_points=None, xy_null=False, edit=None,
                 external=False):
    """mdx_mask_regions_dev, (external) mdx_region_parents_dev, then mdx_region_outlines_dev on a batch of
    equal-sized masks, one stream, one sync at the end; every output buffer 0xAA.  edit(regs, nkept), when given,
    changes the records on the device after the first call (the one case with a sync in between)."""
    B = len(masks)
    h, w = masks[0].shape
    src = np.stack(masks)
    cap = ((w + 1) // 2) * ((h + 1) // 2) if max_regions is None else max_regions
    maxp = 2 * w * h + 8 if max_points is None else max_points
    host = dict(regs=np.full((B, max(cap, 1), 8), AA, np.int32), nall=np.full(B, AA, np.int32),
                nkept=np.full(B, AA, np.int32), labels=np.full((B, h, w), AA, np.int32),
                ext=np.full((B, max(cap, 1), 8), AA, np.int32), next=np.full(B, AA, np.int32),
                offsets=np.full((B, cap + 1), AA, np.int32), xy=np.full((B, max(maxp, 1), 2), AA, np.int32),
                npts=np.full(B, AA, np.int32))
    d = {k: c.dev_alloc(v.nbytes) for k, v in host.items()}
    d["src"] = c.dev_alloc(src.nbytes)
    try:
        for k, v in host.items():
            c.h2d(d[k], v)
        c.h2d(d["src"], src)
        c.mask_regions_dev(B, d["src"], w, h, w, h * w, open3, min_area, d["regs"], cap, d["nall"], d["nkept"],
                           d["labels"], 0)
        if edit is not None:
            c.sync()
            c.d2h(host["regs"], d["regs"]), c.d2h(host["nkept"], d["nkept"])
            edit(host["regs"], host["nkept"])
            c.h2d(d["regs"], host["regs"]), c.h2d(d["nkept"], host["nkept"])
        if external:
            c.region_parents_dev(B, d["labels"], w, h, d["regs"], cap, d["nkept"], 0, d["ext"], d["next"])
        c.region_outlines_dev(B, d["labels"], w, h, d["ext" if external else "regs"], cap,
                              d["next" if external else "nkept"], d["offsets"], 0 if xy_null else d["xy"], maxp, d["npts"])
        c.sync()
        for k, v in host.items():
            c.d2h(v, d[k])
    finally:
        for p in d.values():
            c.dev_free(p)
    host.update(cap=cap, maxp=maxp, external=external, xy_null=xy_null)
    return host


def same(out, i, ref, outlines=None):
    """Image i of a run_outlines result: the records equal the checker's, and every word of offsets, xy and
    num_points equals the tracer's outlines of the records that take part (`outlines`: of edited records)."""
    cap, maxp = out["cap"], out["maxp"]
    if outlines is None:
        r = min(len(ref["kept"]), cap)
        assert out["nkept"][i] == len(ref["kept"])
        assert np.array_equal(out["regs"][i, :r], ref["kept"][:r])
        assert np.array_equal(out["labels"][i], ref["labels"])
        recs = ref["kept"][:r]
        if out["external"]:
            recs = recs[parents_by_rule(ref["labels"], recs) == NO_PARENT]
            assert out["next"][i] == len(recs) and np.array_equal(out["ext"][i, :len(recs)], recs)
            outlines = outlines_of(ref["labels"], recs)
        else:
            outlines = ref["outlines"][:r] if "outlines" in ref else outlines_of(ref["labels"], recs)
    r = len(outlines)
    ends = np.cumsum([0] + [len(v) for v in outlines])
    want_off = np.concatenate([ends, np.full(cap - r, ends[-1])]).astype(np.int32)
    assert np.array_equal(out["offsets"][i], want_off), (out["offsets"][i][:r + 2], want_off[:r + 2])
    assert out["npts"][i] == ends[-1]
    flat = np.array([p for v in outlines for p in v], np.int32).reshape(-1, 2)
    m = 0 if out["xy_null"] else min(len(flat), maxp)
    bad = np.flatnonzero((out["xy"][i, :m] != flat[:m]).any(1))
    assert len(bad) == 0, (len(bad), bad[:4], out["xy"][i, bad[:4]], flat[bad[:4]])
    assert (out["xy"][i, m:] == AA).all()
    return outlines


def one(ctx, mask, open3=False, **kw):
    ref = case(mask, open3=open3, min_area=kw.get("min_area", 1))
    return same(run_outlines(ctx, [mask], open3=open3, **kw), 0, ref)


@functools.lru_cache(maxsize=None)
def exhaustive_4x4():
    """All 65,536 4 x 4 masks, each in a 6 x 6 cell with a background ring: 16 images of 384 x 384."""
    bits = np.arange(1 << 16, dtype=np.uint32)
    cells = np.zeros((1 << 16, 6, 6), np.uint8)
    for i in range(16):
        cells[:, 1 + i // 4, 1 + i % 4] = (bits >> i) & 1
    imgs = cells.reshape(16, 64, 64, 6, 6).transpose(0, 1, 3, 2, 4).reshape(16, 384, 384)
    return [u8(im) for im in imgs]


@pytest.mark.gpu
def test_every_4x4_mask(ctx):
    imgs = exhaustive_4x4()
    out = run_outlines(ctx, imgs, max_regions=16384, max_points=384 * 384)
    total = 0
    for i, m in enumerate(imgs):
        ref = case(m)
        same(out, i, ref)
        total += len(ref["kept"])
    assert total > 65535 and imgs[15][379:383, 379:383].all()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_shapes_equal_the_tracer(ctx, w, h):
    pats = shapes(w, h)
    names = list(pats)
    out = run_outlines(ctx, [pats[n] for n in names])               # one batch: no leakage between them either
    for i, n in enumerate(names):
        try:
            same(out, i, case(pats[n]))
        except AssertionError as e:
            raise AssertionError(f"{n} at {w}x{h}: {e}") from None
    if w >= 64 and h >= 63:
        sp = case(pats["spiral"])
        assert sp["num_all"] == 1 and len(sp["outlines"][0]) > sp["kept"][0, 4] > w * h // 3
        assert len(case(pats["full"])["outlines"][0]) == 2 * (w + h) - 4   # all four frame edges


@pytest.mark.gpu
@pytest.mark.parametrize("dens", [0.05, 0.40, 0.45, 0.60])
def test_random_640x480(ctx, dens):
    outs = one(ctx, big_random(dens))
    if dens >= 0.45:
        assert max(len(o) for o in outs) > 4000             # the giant component's outline


@pytest.mark.gpu
def test_opened_mask_and_min_area(ctx):
    outs = one(ctx, big_random(0.60), open3=True, min_area=20)
    assert len(outs) > 10 and all(len(o) >= 8 for o in outs)


@pytest.mark.gpu
def test_long_outline_needs_every_round(ctx):
    y, x = np.mgrid[0:512, 0:512]
    m = u8((y % 2 == 0) | ((y % 4 == 1) & (x == 511)) | ((y % 4 == 3) & (x == 0)))
    outs = one(ctx, m, max_regions=4)
    assert len(outs) == 1 and len(outs[0]) > 250000 > 1 << 17


@pytest.mark.gpu
def test_caps(ctx):
    m = patterns(130, 67)["random_0.45"]
    ref = case(m)
    total = sum(len(o) for o in ref["outlines"])
    cut = len(ref["outlines"][0]) + len(ref["outlines"][1]) // 2 + 1   # inside the second outline
    for maxp in (cut, 1, total - 1, total):
        same(run_outlines(ctx, [m], max_points=maxp), 0, ref)
    same(run_outlines(ctx, [m], max_points=0, xy_null=True), 0, ref)
    big = next(j for j, o in enumerate(ref["outlines"]) if len(o) > 200)   # a ranked outline cut in two
    same(run_outlines(ctx, [m], max_points=sum(len(o) for o in ref["outlines"][:big]) + 100), 0, ref)
    for cap in (1, 2, len(ref["kept"]) - 1):                           # num_kept > max_regions
        assert len(ref["kept"]) > cap
        same(run_outlines(ctx, [m], max_regions=cap), 0, ref)
    out = run_outlines(ctx, [m], max_regions=0)
    assert out["offsets"][0].tolist() == [0] and out["npts"][0] == 0 and (out["xy"] == AA).all()
    assert out["nkept"][0] == len(ref["kept"])


@pytest.mark.gpu
def test_external_records_only(ctx):
    for m in (nested_outlines(0), islands(130, 67), patterns(65, 63)["rings"]):
        ref = case(m)
        out = run_outlines(ctx, [m], external=True)
        outs = same(out, 0, ref)
        assert 0 < len(outs) < len(ref["kept"])


@pytest.mark.gpu
def test_batches_equal_single_calls(mdx):
    masks = [nested_outlines(s) if s % 2 else patterns(130, 67)[n] for s, n in
             zip(range(32), list(patterns(130, 67)) * 2)]
    masks = [m if m.shape == (67, 130) else patterns(130, 67)["thick_comb"] for m in masks]
    with mdx.Context(0, 130, 67, 32) as c:
        singles = [run_outlines(c, [m]) for m in masks]
        refs = [case(m) for m in masks]
        for i, s in enumerate(singles):
            same(s, 0, refs[i])
        for B in (2, 32):
            out = run_outlines(c, masks[:B])
            for i in range(B):
                for k in ("offsets", "xy", "npts", "regs"):
                    assert np.array_equal(out[k][i], singles[i][k][0]), (B, i, k)


@pytest.mark.gpu
def test_small_call_after_large_sees_no_stale_scratch(mdx):
    with mdx.Context(0, 640, 480, 1) as c:
        one(c, big_random(0.45))
        for w, h in ((7, 5), (65, 63)):
            for n in ("random_0.60", "rings", "full"):
                one(c, patterns(w, h)[n])
        a = run_outlines(c, [big_random(0.45)])
        b = run_outlines(c, [big_random(0.45)])
        assert all(np.array_equal(a[k], b[k]) for k in ("offsets", "xy", "npts"))


@pytest.mark.gpu
def test_records_edited_on_the_device(ctx):
    ring = np.zeros((40, 50), bool)
    ring[5:35, 5:45] = True
    ring[12:28, 12:38] = False                               # a thick ring: 7 wide
    ring[18:22, 20:30] = True                                # an island
    ring[0, 0:3] = True
    m = u8(ring)
    ref = case(m)
    assert ref["kept"][:, 7].tolist() == [0, 1, 2]
    k = ref["kept"]
    recs = np.repeat(k[1:2], 12, 0)                          # the ring's record, twelve times over
    recs[1, 5] = 50                                          # x = w
    recs[2, 5:7] = [-1, 6]
    recs[3, 6] = 40                                          # y = h
    recs[4, 6] = -7
    recs[5, 7] = 2                                           # the seed pixel carries another id
    recs[6, 5:7] = [3, 3]                                    # a background pixel
    recs[7, 7] = -1                                          # the background's own label
    recs[8, 5:7] = [5, 20]                                   # on the outer border, entered from above: the outline from there
    recs[9, 5:7] = [38, 20]                                  # on the hole's border: the hole's cycle
    recs[10, 5:7] = [8, 8]                                   # a member with eight member neighbours: a small cycle
    # recs[0] and recs[11] are the same honest record: both give the whole outline
    corner = k[1].copy()
    corner[5:7] = [44, 34]                                   # a border pixel whose start state no border cycle passes
    recs = np.concatenate([recs, k[2:3], k[0:1], corner[None]])   # two honest ones behind them, one more edited

    def edit(regs, nkept):
        regs[0, :len(recs)] = recs
        nkept[0] = len(recs)
    want = outlines_of(ref["labels"], recs)
    assert [len(o) for o in want[1:8]] == [0] * 7 and want[0] == want[11] == ref["outlines"][1]
    at = want[0].index((5, 20))
    assert want[8] == want[0][at:] + want[0][:at]
    assert want[9][0] == (38, 20) and len(want[9]) == 2 * (16 + 26) and not set(want[9]) & set(want[0])
    assert want[10][0] == (8, 8) and len(want[10]) == 8 and want[14][0] == (44, 34) and len(want[14]) == 8
    assert want[12] == ref["outlines"][2] and want[13] == ref["outlines"][0]
    out = run_outlines(ctx, [m], edit=edit, max_regions=20)
    same(out, 0, ref, outlines=want)


@pytest.mark.gpu
def test_einval_cases_leave_the_outputs_untouched(mdx, ctx):
    L = mdx.lib()
    w, h, M, V = 16, 8, 4, 64
    m = patterns(w, h)["thick_comb"]
    vp = C.c_void_p
    out = run_outlines(ctx, [m], max_regions=M, max_points=V)         # a good call's outputs, to start from
    words = 4096
    d = ctx.dev_alloc(words * 4)
    try:
        img = np.full(words, AA, np.int32)
        img[:w * h] = out["labels"][0].ravel()
        img[1024:1024 + 8 * M] = out["regs"][0].ravel()
        img[1100] = out["nkept"][0]
        ctx.h2d(d, img)
        lab, rec, nk, off, xy, nv = (vp(d + 4 * o) for o in (0, 1024, 1100, 2048, 2100, 2090))
        ok = dict(batch=1, labels=lab, w=w, h=h, regions=rec, max_regions=M, num_kept=nk, offsets=off, xy=xy,
                  max_points=V, nv=nv)

        def dev(**kw):
            a = dict(ok, **kw)
            return L.mdx_region_outlines_dev(ctx._h, a["batch"], a["labels"], a["w"], a["h"], a["regions"],
                                             a["max_regions"], a["num_kept"], a["offsets"], a["xy"], a["max_points"], a["nv"])
        bad = [dict(batch=0), dict(batch=-1), dict(w=0), dict(h=0), dict(w=-3), dict(w=1 << 13, h=(1 << 17) + 1),
               dict(w=1 << 14, h=(1 << 14) + 1), dict(max_regions=-1), dict(max_points=-1), dict(labels=None),
               dict(offsets=None), dict(regions=None), dict(num_kept=None), dict(xy=None)]
        for kw in bad:
            assert dev(**kw) == -1, kw
            assert b"mdx_region_outlines_dev" in L.mdx_last_error(ctx._h)
        ctx.sync()
        back = np.empty_like(img)
        ctx.d2h(back, d)
        assert np.array_equal(back, img)                              # no rejected call wrote anything
        assert dev(regions=None, num_kept=None, max_regions=0, xy=None, max_points=0) == 0   # nothing wanted: NULLs are fine
        assert dev(w=8193, h=1, max_regions=0) == 0                   # no span limit here
        assert dev() == 0
        ctx.sync()
        ctx.d2h(back, d)
        assert np.array_equal(back[2048:2048 + M + 1], out["offsets"][0]) and back[2090] == out["npts"][0]
        assert np.array_equal(back[2100:2100 + 2 * V], out["xy"][0].ravel())
        back[2048:2048 + M + 1] = back[2090] = back[2100:2100 + 2 * V] = AA
        assert np.array_equal(back, img)                              # and nothing else
    finally:
        ctx.dev_free(d)
    # the host entry: mdx_mask_regions' errors plus its own
    p = lambda a: a.ctypes.data_as(vp)   # noqa: E731
    regs, offs, pts = np.full((M, 8), AA, np.int32), np.full(M + 1, AA, np.int32), np.full((V, 2), AA, np.int32)
    cnt = [C.c_int(-5) for _ in range(3)]
    okh = dict(mask=p(m), w=w, h=h, stride=w, flags=OPEN3, regions=p(regs), max_regions=M, offsets=p(offs), xy=p(pts),
               max_points=V)

    def hst(**kw):
        a = dict(okh, **kw)
        return L.mdx_mask_region_outlines(ctx._h, a["mask"], a["w"], a["h"], a["stride"], a["flags"], 1, a["regions"],
                                          a["max_regions"], C.byref(cnt[0]), C.byref(cnt[1]), None, None, None,
                                          a["offsets"], a["xy"], a["max_points"], C.byref(cnt[2]))
    for kw in [dict(mask=None), dict(w=0), dict(h=-1), dict(stride=w - 1), dict(w=1 << 13, h=(1 << 17) + 1, stride=1 << 13),
               dict(w=1 << 14, h=(1 << 14) + 1, stride=1 << 14), dict(max_regions=-1), dict(regions=None), dict(flags=8),
               dict(max_points=-1), dict(offsets=None), dict(xy=None)]:
        assert hst(**kw) == -1, kw
        assert b"mdx_mask_region_outlines" in L.mdx_last_error(ctx._h)
    assert (regs == AA).all() and (offs == AA).all() and (pts == AA).all() and [v.value for v in cnt] == [-5] * 3
    assert hst() == 0 and hst(xy=None, max_points=0) == 0 and hst(regions=None, max_regions=0) == 0
    assert offs[0] == 0 and cnt[2].value == 0                         # max_regions 0: no record takes part


@pytest.mark.gpu
def test_host_entry_and_python_wrapper(mdx, ctx):
    L = mdx.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    m = np.zeros((129, 257), np.uint8)
    m[:67, :130] = nested_outlines(0)
    m[70:, :] = patterns(257, 59)["random_0.60"]
    for open3, min_area in ((False, 1), (True, 4)):
        ref = case(m, open3=open3, min_area=min_area)
        k = len(ref["kept"])
        ext = np.flatnonzero(parents_by_rule(ref["labels"], ref["kept"]) == NO_PARENT)
        assert 0 < len(ext) < k or open3
        r = ctx.mask_regions(m, open3=open3, min_area=min_area, want_outlines=True)
        assert type(r) is mdx.RegionResult and r.hulls is None
        assert (r.num_all, r.num_kept) == (ref["num_all"], k) and np.array_equal(r.regions, ref["kept"])
        assert len(r.outlines) == k and all(a.dtype == np.int32 and a.shape == (len(b), 2) and a.tolist() == [list(q) for q in b]
                                            for a, b in zip(r.outlines, ref["outlines"]))
        t = ctx.mask_regions(m, open3=open3, min_area=min_area, want_outlines=True, want_parents=True, want_hulls=True)
        assert type(t) is mdx.RegionTreeResult and np.array_equal(t.external, ext) and len(t.hulls) == len(ext)
        assert len(t.outlines) == len(ext) and all(a.tolist() == [list(q) for q in ref["outlines"][j]]
                                                   for a, j in zip(t.outlines, ext))
        assert ctx.mask_regions(m, open3=open3, min_area=min_area).outlines is None
        # the raw entry on a pitched view with 0xFF padding, every word of its outputs
        pitched = np.full((129, 300), 0xFF, np.uint8)
        pitched[:, :257] = m
        total = sum(len(o) for o in ref["outlines"])
        flat = np.array([q for o in ref["outlines"] for q in o], np.int32).reshape(-1, 2)
        cap, maxp = k + 3, total + 5
        regs, off = np.full((cap, 8), AA, np.int32), np.full(cap + 1, AA, np.int32)
        xy = np.full((maxp, 2), AA, np.int32)
        nall, nkept, npts = C.c_int(-5), C.c_int(-5), C.c_int(-5)
        fl = OPEN3 if open3 else 0
        assert L.mdx_mask_region_outlines(ctx._h, p(pitched), 257, 129, 300, fl, min_area, p(regs), cap, C.byref(nall),
                                          C.byref(nkept), None, None, None, p(off), p(xy), maxp, C.byref(npts)) == 0
        assert (nall.value, nkept.value, npts.value) == (ref["num_all"], k, total)
        assert np.array_equal(regs[:k], ref["kept"]) and (regs[k:] == AA).all()
        ends = np.cumsum([0] + [len(o) for o in ref["outlines"]])
        assert np.array_equal(off, np.concatenate([ends, [total] * 3]))
        assert np.array_equal(xy[:total], flat) and (xy[total:] == AA).all()
        # cut short: only the points that exist and fit come back
        xy[:] = AA
        assert L.mdx_mask_region_outlines(ctx._h, p(pitched), 257, 129, 300, fl, min_area, p(regs), cap, None, None, None,
                                          None, None, p(off), p(xy), 7, C.byref(npts)) == 0
        assert npts.value == total and np.array_equal(xy[:7], flat[:7]) and (xy[7:] == AA).all()
        # the external records: parents and external_index as mdx_mask_regions_tree's
        par, ei, next_ = np.full(cap, AA, np.int32), np.full(cap, AA, np.int32), C.c_int(-5)
        xy[:] = AA
        assert L.mdx_mask_region_outlines(ctx._h, p(pitched), 257, 129, 300, fl, min_area, p(regs), cap, None, None, p(par),
                                          p(ei), C.byref(next_), p(off), p(xy), maxp, C.byref(npts)) == 0
        assert next_.value == len(ext) and np.array_equal(ei[:len(ext)], ext) and (ei[len(ext):] == AA).all()
        assert np.array_equal(par[:k], parents_by_rule(ref["labels"], ref["kept"])) and (par[k:] == AA).all()
        eflat = np.array([q for j in ext for q in ref["outlines"][j]], np.int32).reshape(-1, 2)
        assert npts.value == len(eflat) and np.array_equal(xy[:len(eflat)], eflat) and (xy[len(eflat):] == AA).all()


@pytest.mark.gpu
def test_python_wrapper_asks_again_when_the_points_outgrow_its_guess(ctx):
    y, x = np.mgrid[0:64, 0:96]
    m = u8((y % 2 == 0) | ((y % 4 == 1) & (x == 95)) | ((y % 4 == 3) & (x == 0)))
    ref = case(m)
    assert len(ref["outlines"][0]) > max(4096, 64 * 96 // 4)
    r = ctx.mask_regions(m, open3=False, want_outlines=True)
    assert [a.tolist() for a in r.outlines] == [[list(q) for q in o] for o in ref["outlines"]]


# ---------------------------------------------------------------- end to end: chained behind the pair entry

@pytest.mark.gpu
def test_chained_behind_the_pair_entry(mdx):
    """mdx_flow_warp_diff_batch_dev -> mdx_mask_regions_dev -> mdx_region_parents_dev -> mdx_region_outlines_dev
    on d_external, one stream, no sync in between, on the golden rgb pair."""
    w, h, B, cap, maxp = 160, 120, 1, 64, 4096
    with mdx.Context(0, w, h, B, fit_mode=mdx.FIT_EXTERNAL, thresh=30) as c:
        host = dict(regs=np.full((B, cap, 8), AA, np.int32), nall=np.full(B, AA, np.int32),
                    nkept=np.full(B, AA, np.int32), mask=np.full((B, h, w), 0xAA, np.uint8),
                    labels=np.full((B, h, w), AA, np.int32), ext=np.full((B, cap, 8), AA, np.int32),
                    next=np.full(B, AA, np.int32), offsets=np.full((B, cap + 1), AA, np.int32),
                    xy=np.full((B, maxp, 2), AA, np.int32), npts=np.full(B, AA, np.int32))
        d = {k: c.dev_alloc(v.nbytes) for k, v in host.items()}
        try:
            for k, v in host.items():
                c.h2d(d[k], v)
            g = np.load(os.path.join(ROOT, "tests", "golden", "synth_160x120_rgb.npz"))
            # the identity as the external fit: the mask is the frame difference, which has blobs of every size
            g1, g2, Hs = g["img1"][None].copy(), g["img2"][None].copy(), np.eye(3)[None].copy()
            n = mdx.grid_count(w, h, c.params.pixel_step)
            d.update(i1=c.dev_alloc(g1.nbytes), i2=c.dev_alloc(g2.nbytes), H=c.dev_alloc(Hs.nbytes),
                     np=c.dev_alloc(B * n * 8), st=c.dev_alloc(B * n))
            c.h2d(d["i1"], g1), c.h2d(d["i2"], g2), c.h2d(d["H"], Hs)
            c.flow_warp_diff_batch_dev(B, d["i1"], d["i2"], w, h, 3 * w, 3 * w * h, mdx.FMT_RGB8, d["np"], d["st"], 0,
                                       d["mask"], 0, d["H"], 0)
            c.mask_regions_dev(B, d["mask"], w, h, w, w * h, True, 50, d["regs"], cap, d["nall"], d["nkept"], d["labels"])
            c.region_parents_dev(B, d["labels"], w, h, d["regs"], cap, d["nkept"], 0, d["ext"], d["next"])
            c.region_outlines_dev(B, d["labels"], w, h, d["ext"], cap, d["next"], d["offsets"], d["xy"], maxp, d["npts"])
            c.sync()
            for k, v in host.items():
                c.d2h(v, d[k])
        finally:
            for p in d.values():
                c.dev_free(p)
    host.update(cap=cap, maxp=maxp, external=True, xy_null=False)
    ref = case(host["mask"][0], open3=True, min_area=50)
    assert host["nall"][0] == ref["num_all"] and host["nkept"][0] >= 1      # else the comparison is vacuous
    outs = same(host, 0, ref)
    assert len(outs) >= 1 and all(len(o) >= 20 for o in outs)
