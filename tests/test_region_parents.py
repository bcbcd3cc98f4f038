"""Which mask region lies inside which, on the device (mdx_region_parents_dev / mdx_mask_regions_tree).

The reference asks findContours for CV_RETR_EXTERNAL (common/src/background_subtractor.cpp:31-35): only the
blobs that lie in no other blob's hole are detections.  Restated, and unpinned against a real build like the
rest of the recipe.

Two checkers, written from the definitions in include/mdx.h; neither shares anything with the kernels:
  parents_by_enclosure  K encloses C iff a 4-connected walk from outside the frame over pixels that are not K
                        never reaches C; the parent is the innermost encloser.  One flood fill per candidate K.
  parents_by_rule       the two "pixel above" rules on a flood fill of the padded background
                        (test_regions.regions_reference with connectivity=4).
Everything is integer and exact: every output buffer is prefilled with 0xAA words and every word is compared.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from test_hulls import hull_oracle  # noqa: F401  (expected_hulls applies it)
from test_region_hulls import expected_hulls
from test_regions import AA, OPEN3, ROOT, SIZES, big_random, patterns, regions_reference

NO_PARENT, UNKNOWN = -1, -2


# ---------------------------------------------------------------- the checkers

def _untrusted(labels, rec):
    """A record the entry cannot trust (include/mdx.h): seed outside the frame, seed pixel not the record's id,
    or the pixel above the seed not background."""
    h, w = labels.shape
    sx, sy, cid = int(rec[5]), int(rec[6]), int(rec[7])
    if not (0 <= sx < w and 0 <= sy < h) or cid < 0 or labels[sy, sx] != cid:
        return True
    return sy > 0 and labels[sy - 1, sx] >= 0


def parents_by_rule(labels, recs):
    """The background of the label image, padded by one ring of background (the outside of the frame), as
    4-connected components: component 0 holds the padding, so it is the frame background; the others are the
    holes and their seeds the holes' first pixels."""
    labels = np.asarray(labels)
    bg = np.pad(labels < 0, 1, constant_values=True)
    r = regions_reference(np.where(bg, 255, 0).astype(np.uint8), open3=False, connectivity=4)
    bl, holes = r["labels"], r["kept"]
    assert bl[0, 0] == 0
    out = []
    for rec in np.asarray(recs).reshape(-1, 8):
        if _untrusted(labels, rec):
            out.append(UNKNOWN)
            continue
        comp = bl[rec[6], rec[5] + 1]                    # (seed_x, seed_y - 1) in padded coordinates
        assert comp >= 0
        if comp == 0:
            out.append(NO_PARENT)
            continue
        hx, hy = holes[comp, 5] - 1, holes[comp, 6] - 1  # the hole's first pixel, frame coordinates
        assert hy >= 1 and labels[hy - 1, hx] >= 0
        out.append(int(labels[hy - 1, hx]))
    return np.array(out, np.int32)


def _reached_without(labels, k):
    """The frame's pixels that a 4-connected walk from outside reaches without stepping on component k."""
    h, w = labels.shape
    w2 = w + 2
    free = np.zeros((h + 4, w2), np.uint8)               # a ring of outside, then a row of wall above and below
    free[1:-1] = 1                                       # (a step off a row's end lands in the ring again: harmless)
    free[2:-2, 1:-1] = labels != k
    todo = bytearray(free.tobytes())
    start = w2
    todo[start] = 0
    stack, seen = [start], []
    while stack:
        p = stack.pop()
        seen.append(p)
        for o in (-w2, -1, 1, w2):
            if todo[p + o]:
                todo[p + o] = 0
                stack.append(p + o)
    out = np.zeros((h + 4) * w2, bool)
    out[seen] = True
    return out.reshape(h + 4, w2)[2:-2, 1:-1]


def enclosure_tree(labels, all_recs):
    """parent id (or -1) and depth of EVERY component, from the definition of enclosure alone."""
    labels = np.asarray(labels)
    all_recs = np.asarray(all_recs).reshape(-1, 8)
    n = len(all_recs)
    enclosers = [[] for _ in range(n)]
    for k in range(n):
        # a barrier against a 4-connected walk surrounds at least one pixel: it spans 3 x 3 or more
        if all_recs[k, 2] < 3 or all_recs[k, 3] < 3:
            continue
        reached = _reached_without(labels, k)
        for c in range(n):
            if c != k and not reached[all_recs[c, 6], all_recs[c, 5]]:
                enclosers[c].append(k)
    depth = [len(e) for e in enclosers]
    parent = [max(e, key=lambda k: depth[k]) if e else NO_PARENT for e in enclosers]
    for c in range(n):                                   # enclosers are nested: a chain of distinct depths
        assert sorted(depth[k] for k in enclosers[c]) == list(range(len(enclosers[c])))
    return np.array(parent, np.int32), np.array(depth, np.int32)


def parents_by_enclosure(labels, recs, all_recs):
    tree, _ = enclosure_tree(labels, all_recs)
    return np.array([UNKNOWN if _untrusted(labels, r) else tree[r[7]] for r in np.asarray(recs).reshape(-1, 8)], np.int32)


def u8(a):
    return np.where(np.asarray(a) != 0, 255, 0).astype(np.uint8)


def outline_rect(m, x0, y0, x1, y1):
    m[y0, x0:x1 + 1] = m[y1, x0:x1 + 1] = True
    m[y0:y1 + 1, x0] = m[y0:y1 + 1, x1] = True


def outline_diamond(m, cx, cy, r):
    y, x = np.mgrid[0:m.shape[0], 0:m.shape[1]]
    m |= np.abs(x - cx) + np.abs(y - cy) == r


def nested_outlines(seed):
    """Rectangle and diamond outlines recursed into their interiors; some interiors split in two; single pixels
    at the leaves.  What is drawn inside an outline keeps one background pixel from it in all 8 directions."""
    rng = np.random.default_rng(1000 + seed)
    w, h = (130, 67) if seed == 0 else (40 + (seed * 37) % 91, 20 + (seed * 17) % 48)
    m = np.zeros((h, w), bool)

    def fill(x0, y0, x1, y1):
        bw, bh = x1 - x0 + 1, y1 - y0 + 1
        if bw < 1 or bh < 1:
            return
        if bw < 5 or bh < 5:
            m[(y0 + y1) // 2, (x0 + x1) // 2] = True
            return
        kind = int(rng.integers(4))
        if kind == 0 and bw >= 11:
            mid = x0 + int(rng.integers(5, bw - 5))
            fill(x0, y0, mid - 1, y1), fill(mid + 1, y0, x1, y1)
        elif kind == 1 and min(bw, bh) >= 7:
            r = (min(bw, bh) - 1) // 2
            cx, cy = x0 + r + int(rng.integers(0, bw - 2 * r)), y0 + r + int(rng.integers(0, bh - 2 * r))
            outline_diamond(m, cx, cy, r)
            s = (r - 3) // 2                             # |dx| + |dy| <= r - 3 is not 8-adjacent to the outline
            fill(cx - s, cy - s, cx + s, cy + s)
        else:
            a, b = int(rng.integers(0, min(3, bw - 4))), int(rng.integers(0, min(3, bh - 4)))
            x0, y0 = x0 + a, y0 + b                          # at least 5 x 5 stays
            x1, y1 = x1 - int(rng.integers(0, min(3, bw - 4 - a))), y1 - int(rng.integers(0, min(3, bh - 4 - b)))
            outline_rect(m, x0, y0, x1, y1)
            fill(x0 + 2, y0 + 2, x1 - 2, y1 - 2)
    fill(0, 0, w - 1, h - 1)
    return u8(m)


@functools.lru_cache(maxsize=None)
def outline_case(seed):
    m = nested_outlines(seed)
    ref = regions_reference(m, open3=False)
    return m, ref, parents_by_rule(ref["labels"], ref["kept"])


def ring7():
    m = np.zeros((7, 7), np.uint8)
    m[0, :] = m[6, :] = m[:, 0] = m[:, 6] = 1
    m[3, 3] = 1
    return u8(m)


def diamond_with_pixel(w=9, h=9, cx=4, cy=4, r=3):
    m = np.zeros((h, w), bool)
    outline_diamond(m, cx, cy, r)
    m[cy, cx] = True
    return u8(m)


# ---------------------------------------------------------------- CPU

def test_header_and_binding_declare_both_entries(mdx):
    from test_abi import HEADER, header_functions
    names = header_functions()
    for n in ("mdx_region_parents_dev", "mdx_mask_regions_tree"):
        assert n in names and n in mdx._lib.EXPORTED
    assert sorted(mdx._lib.EXPORTED) == names
    hdr = open(HEADER).read()
    assert int(re.search(r"#define MDX_ABI_VERSION (\d+)", hdr).group(1)) == mdx._lib.ABI_VERSION == 11
    assert re.search(r"#define MDX_REGION_NO_PARENT \(-1\)", hdr) and re.search(r"#define MDX_REGION_PARENT_UNKNOWN \(-2\)", hdr)
    assert (mdx._lib.REGION_NO_PARENT, mdx._lib.REGION_PARENT_UNKNOWN) == (NO_PARENT, UNKNOWN)
    assert C.sizeof(mdx._lib.MdxParams) == 80


def test_null_context_is_einval(mdx):
    L = mdx.lib()
    m = np.zeros((4, 4), np.uint8)
    off = np.zeros(16, np.int32)
    n = C.c_int(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert L.mdx_region_parents_dev(None, 1, p(off), 4, 4, None, 0, None, None, None, None) == mdx._lib.MDX_EINVAL
    assert L.mdx_mask_regions_tree(None, p(m), 4, 4, 4, OPEN3, 1, None, 0, C.byref(n), C.byref(n), None, None, C.byref(n),
                                   None, None, 0, None) == mdx._lib.MDX_EINVAL


def test_result_type_extends_region_result(mdx):
    import dataclasses
    assert issubclass(mdx.RegionTreeResult, mdx.RegionResult)
    assert [f.name for f in dataclasses.fields(mdx.RegionTreeResult)][-3:] == ["hulls", "parent", "external"]
    z = np.array([[1, 2, 3, 4, 12, 1, 2, 0], [2, 3, 1, 1, 1, 2, 3, 1]], np.int32)
    r = mdx.RegionTreeResult(z, 2, 2, parent=np.array([-1, 0], np.int32), external=np.array([0], np.int32))
    assert r.rectangles == [(1, 2, 3, 4), (2, 3, 1, 1)] and r.external_rectangles == [(1, 2, 3, 4)]


def test_hand_cases():
    ref = regions_reference(ring7(), open3=False)
    assert parents_by_rule(ref["labels"], ref["kept"]).tolist() == [-1, 0]
    assert parents_by_enclosure(ref["labels"], ref["kept"], ref["kept"]).tolist() == [-1, 0]
    # a U open to each frame edge, a pixel in its pocket: the pocket is frame background
    u = np.zeros((7, 7), np.uint8)
    u[1:6, 1] = u[1:6, 5] = u[5, 1:6] = 1                    # open to the top: the pocket reaches row 0
    u[3, 3] = 1
    for k in range(4):
        m = u8(np.rot90(u, k))
        ref = regions_reference(m, open3=False)
        assert ref["num_all"] == 2
        assert parents_by_rule(ref["labels"], ref["kept"]).tolist() == [-1, -1], k
        assert parents_by_enclosure(ref["labels"], ref["kept"], ref["kept"]).tolist() == [-1, -1], k
    # a diamond outline with a pixel inside: the background inside meets the outside only through diagonals
    m = diamond_with_pixel()
    ref = regions_reference(m, open3=False)
    assert ref["num_all"] == 2 and ref["kept"][0, 4] == 12
    assert parents_by_rule(ref["labels"], ref["kept"]).tolist() == [-1, 0]
    assert parents_by_enclosure(ref["labels"], ref["kept"], ref["kept"]).tolist() == [-1, 0]
    bg = np.pad(ref["labels"] < 0, 1, constant_values=True)
    assert regions_reference(u8(bg), open3=False, connectivity=8)["num_all"] == 1   # joined through diagonals: external
    assert regions_reference(u8(bg), open3=False, connectivity=4)["num_all"] == 2


def test_untrusted_records_are_unknown():
    ref = regions_reference(ring7(), open3=False)
    recs = np.repeat(ref["kept"][:1], 6, 0)
    recs[1, 5] = 7                                           # x = w
    recs[2, 5:7] = [-1, 1]
    recs[3, 6] = 7                                           # y = h
    recs[4, 7] = 1                                           # another id
    recs[5, 5:7] = [0, 1]                                    # not the first pixel: the ring lies above it
    assert parents_by_rule(ref["labels"], recs).tolist() == [-1, -2, -2, -2, -2, -2]
    assert parents_by_enclosure(ref["labels"], recs, ref["kept"]).tolist() == [-1, -2, -2, -2, -2, -2]


@pytest.mark.parametrize("w,h", [(1, 1), (97, 1), (1, 97), (7, 5), (33, 31)])
def test_checkers_agree_on_patterns(w, h):
    for name, m in patterns(w, h).items():
        for open3 in (False, True):
            ref = regions_reference(m, open3=open3)
            a = parents_by_rule(ref["labels"], ref["kept"])
            b = parents_by_enclosure(ref["labels"], ref["kept"], ref["kept"])
            assert np.array_equal(a, b), (name, w, h, open3)


def test_checkers_agree_on_nested_outlines_and_the_family_nests():
    nested, deepest = 0, 0
    for seed in range(20):
        m, ref, rule = outline_case(seed)
        tree, depth = enclosure_tree(ref["labels"], ref["kept"])
        assert np.array_equal(rule, tree), seed
        nested += int((tree >= 0).sum())
        deepest = max(deepest, int(depth.max()))
    assert nested >= 100 and deepest >= 3
    assert outline_case(0)[0].shape == (67, 130)


def test_rings_all_but_the_outermost_are_nested():
    ref = regions_reference(patterns(65, 63)["rings"], open3=False)
    par = parents_by_rule(ref["labels"], ref["kept"])
    assert len(par) >= 10 and par.tolist() == [-1] + list(range(len(par) - 1))
    assert np.array_equal(par, parents_by_enclosure(ref["labels"], ref["kept"], ref["kept"]))


# ---------------------------------------------------------------- GPU: through the C-ABI

def run_parents(c, masks, open3=False, min_area=1, max_regions=None, edit=None, want=("parent", "ext", "next"),
                hulls=False, maxv=None):
    """mdx_mask_regions_dev, mdx_region_parents_dev and (hulls) mdx_region_hulls_dev on the external records, on a
    batch of equal-sized masks, one stream, one sync at the end; every output buffer 0xAA.  edit(regs, nkept),
    when given, changes the records on the device between the first two calls (the one case with a sync in
    between).  Returns the whole buffers."""
    B = len(masks)
    h, w = masks[0].shape
    src = np.stack(masks)
    cap = ((w + 1) // 2) * ((h + 1) // 2) if max_regions is None else max_regions
    maxv = (min(w * h, 2 * min(w, h) * cap) + 8 if maxv is None else maxv) if hulls else 1
    host = dict(regs=np.full((B, max(cap, 1), 8), AA, np.int32), nall=np.full(B, AA, np.int32),
                nkept=np.full(B, AA, np.int32), labels=np.full((B, h, w), AA, np.int32),
                parent=np.full((B, max(cap, 1)), AA, np.int32), ext=np.full((B, max(cap, 1), 8), AA, np.int32),
                next=np.full(B, AA, np.int32), offsets=np.full((B, cap + 1), AA, np.int32),
                xy=np.full((B, max(maxv, 1), 2), AA, np.int32), nv=np.full(B, AA, np.int32))
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
        c.region_parents_dev(B, d["labels"], w, h, d["regs"], cap, d["nkept"], *(d[k] if k in want else 0
                                                                                 for k in ("parent", "ext", "next")))
        if hulls:
            c.region_hulls_dev(B, d["labels"], w, h, d["ext"], cap, d["next"], d["offsets"], d["xy"], maxv, d["nv"])
        c.sync()
        for k, v in host.items():
            c.d2h(v, d[k])
    finally:
        for p in d.values():
            c.dev_free(p)
    host.update(cap=cap, maxv=maxv, hulls=hulls, want=want)
    return host


def same(out, i, ref, want=None, recs=None):
    """Image i of a run_parents result: the records equal the checker's (unless recs gives edited ones); every
    word of parent, ext and next equals `want` (default: parents_by_rule) and what follows from it; the hulls,
    when run, are expected_hulls of the external records.  Returns the parents."""
    cap = out["cap"]
    if recs is None:
        r = min(len(ref["kept"]), cap)
        assert out["nkept"][i] == len(ref["kept"])
        assert np.array_equal(out["regs"][i, :r], ref["kept"][:r])
        assert np.array_equal(out["labels"][i], ref["labels"])
        recs = ref["kept"][:r]
    r = len(recs)
    if want is None:
        want = parents_by_rule(ref["labels"], recs)
    assert len(want) == r
    ext = recs[want == NO_PARENT]
    if "parent" in out["want"]:
        assert np.array_equal(out["parent"][i, :r], want), (out["parent"][i, :r], want)
        assert (out["parent"][i, r:] == AA).all()
    else:
        assert (out["parent"][i] == AA).all()
    if "ext" in out["want"]:
        assert np.array_equal(out["ext"][i, :len(ext)], ext)
        assert (out["ext"][i, len(ext):] == AA).all()
    else:
        assert (out["ext"][i] == AA).all()
    assert out["next"][i] == (len(ext) if "next" in out["want"] else AA)
    if out["hulls"]:
        hulls = expected_hulls(ref["labels"], ext)
        ends = np.cumsum([0] + [len(v) for v in hulls])
        want_off = np.concatenate([ends, np.full(cap - len(ext), ends[-1])]).astype(np.int32)
        assert np.array_equal(out["offsets"][i], want_off)
        assert out["nv"][i] == ends[-1]
        flat = np.array([p for v in hulls for p in v], np.int32).reshape(-1, 2)
        m = min(len(flat), out["maxv"])
        assert np.array_equal(out["xy"][i, :m], flat[:m]) and (out["xy"][i, m:] == AA).all()
    return want


def one(ctx, mask, open3=False, **kw):
    ref = regions_reference(mask, open3=open3, min_area=kw.get("min_area", 1))
    return same(run_parents(ctx, [mask], open3=open3, **kw), 0, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_patterns_equal_the_checkers(ctx, w, h):
    pats = patterns(w, h)
    names = list(pats)
    for open3 in (False, True):
        out = run_parents(ctx, [pats[n] for n in names], open3=open3)   # one batch: no leakage between them either
        for i, n in enumerate(names):
            ref = regions_reference(pats[n], open3=open3)
            try:
                par = same(out, i, ref)
                if w * h <= 65 * 63:
                    assert np.array_equal(par, parents_by_enclosure(ref["labels"], ref["kept"], ref["kept"]))
            except AssertionError as e:
                raise AssertionError(f"{n} at {w}x{h}, open3={open3}: {e}") from None


@pytest.mark.gpu
@pytest.mark.parametrize("dens", [0.40, 0.45, 0.60])
def test_random_640x480(ctx, dens):
    m = big_random(dens)
    par = one(ctx, m)
    assert (par >= 0).sum() > 50 and (par == NO_PARENT).sum() > 10   # holes with islands, and external blobs


@pytest.mark.gpu
def test_nested_outlines(ctx):
    for seed in range(20):
        m, ref, rule = outline_case(seed)
        try:
            par = same(run_parents(ctx, [m], hulls=seed < 4), 0, ref, want=rule)
            if seed < 6:
                assert np.array_equal(par, parents_by_enclosure(ref["labels"], ref["kept"], ref["kept"]))
        except AssertionError as e:
            raise AssertionError(f"seed {seed}, {m.shape}: {e}") from None


def tile_cases():
    """Hand-made masks in a 130 x 67 frame, around the 64 x 32 tiles; name -> (mask, its records' parents)."""
    w, h = 130, 67
    z = lambda: np.zeros((h, w), bool)   # noqa: E731
    out = {}
    m = z()
    outline_diamond(m, 64, 32, 3)
    m[32, 64] = True
    out["diamond on the tile corner"] = (m, [-1, 0])         # inside and outside touch only across (64, 32)'s corner
    m = z()
    outline_diamond(m, 64, 32, 1)                            # the smallest: its hole is the corner pixel itself
    out["one-pixel hole on the tile corner"] = (m, [-1])
    m = z()
    outline_rect(m, 10, 31, 20, 40)                          # the hole's first pixel (11, 32): row 0 of a tile
    m[35, 15] = True
    outline_rect(m, 63, 5, 70, 12)                           # the hole's first pixel (64, 6): column 0 of a tile
    m[8, 66] = True
    out["hole starts on a tile's row 0 / column 0"] = (m, [-1, 0, -1, 2])
    m = z()
    outline_rect(m, 40, 20, 90, 50)                          # the hole spans four tiles
    m[35, 64] = True
    out["hole over four tiles"] = (m, [-1, 0])
    m = z()
    outline_rect(m, 5, 5, 7, 7)                              # a one-pixel hole, nothing in it
    outline_rect(m, 20, 5, 40, 25)                           # a hole with two islands
    m[10, 25] = m[15, 35] = True
    out["one-pixel hole; two islands"] = (m, [-1, -1, 1, 1])
    m = z()
    outline_rect(m, 2, 2, 127, 64)
    outline_rect(m, 30, 10, 100, 60)
    outline_rect(m, 50, 20, 80, 50)
    m[33, 65] = True
    out["depth 3"] = (m, [-1, 0, 1, 2])
    m = z()
    outline_rect(m, 60, 0, 70, 10)                           # seed at y = 0; its island's hole is no frame background
    m[5, 65] = True
    out["seed at y = 0"] = (m, [-1, 0])
    m = z()
    m[:, :] = True
    out["full"] = (m, [-1])
    out["empty"] = (z(), [])
    m = z()
    outline_rect(m, 0, 0, w - 1, h - 1)                      # no frame background inside the frame at all
    m[33, 64] = True
    out["frame ring"] = (m, [-1, 0])
    return {k: (u8(v), p) for k, (v, p) in out.items()}


@pytest.mark.gpu
def test_tile_geometry(ctx):
    cases = tile_cases()
    names = list(cases)
    out = run_parents(ctx, [cases[n][0] for n in names], hulls=True)
    for i, n in enumerate(names):
        m, hand = cases[n]
        ref = regions_reference(m, open3=False)
        try:
            par = same(out, i, ref)
            assert np.array_equal(par, parents_by_enclosure(ref["labels"], ref["kept"], ref["kept"]))
            assert par.tolist() == hand
        except AssertionError as e:
            raise AssertionError(f"{n}: {e}") from None

def thin_ring_case():
    m = np.zeros((67, 130), bool)
    outline_rect(m, 10, 10, 20, 20)                          # a thin ring: 40 pixels
    m[14:17, 14:17] = True                                   # a 9-pixel child inside it
    m[40:50, 60:90] = True                                   # and a solid blob elsewhere
    return u8(m)


@pytest.mark.gpu
def test_min_area_drops_the_ring_but_not_the_parent(ctx):
    assert one(ctx, thin_ring_case()).tolist() == [-1, 0, -1]
    m = np.zeros((67, 130), bool)
    outline_rect(m, 10, 10, 30, 30)                          # a thin ring: 80 pixels
    m[13:28, 13:28] = True                                   # its child: 225 pixels
    m[40:50, 60:90] = True                                   # a solid blob elsewhere: 300 pixels
    m = u8(m)
    ref = regions_reference(m, open3=False, min_area=100)
    assert ref["kept"][:, 7].tolist() == [1, 2]              # the ring (id 0) is left out of the records
    out = run_parents(ctx, [m], min_area=100, hulls=True)
    assert same(out, 0, ref).tolist() == [0, -1]             # the child's parent is the unkept ring's id: not external
    assert out["next"][0] == 1 and out["ext"][0, 0, 7] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("max_regions", [0, 1, 3, 5])
def test_max_regions_below_num_kept(ctx, max_regions):
    m, ref, rule = outline_case(0)
    assert len(ref["kept"]) > 5 and (rule[:5] >= 0).any() and (rule[:5] == NO_PARENT).any()
    out = run_parents(ctx, [m, m], max_regions=max_regions, hulls=True)
    for i in range(2):
        par = same(out, i, ref)                              # nothing past r is written; next counts among the first r
        assert len(par) == max_regions
        assert out["next"][i] == (rule[:max_regions] == NO_PARENT).sum()


@pytest.mark.gpu
def test_any_output_may_be_null(ctx):
    m, ref, rule = outline_case(1)
    for want in [("parent",), ("ext",), ("next",), ("ext", "next"), ()]:
        same(run_parents(ctx, [m], want=want), 0, ref, want=rule)


@pytest.mark.gpu
def test_records_edited_on_the_device(ctx):
    """Image 0 of a batch of two, so that a missing bounds test reads inside the batch's own buffers and shows
    as a wrong value: every edited seed is chosen so that the word it would alias carries the record's id."""
    w, h = 130, 67
    m = np.zeros((h, w), bool)
    m[0, 125:130] = True                                     # id 0, holds (w - 1, 0): what (-1, 1) aliases
    m[3, 5] = True                                           # id 1, seed (5, 3) ...
    m[4, 0:6] = True                                         # ... and holds (0, 4): what (w, 3) aliases
    outline_rect(m, 20, 10, 100, 60)                         # id 2
    m[30, 50] = True                                         # id 3, inside it
    m = u8(m)
    ref = regions_reference(m, open3=False)
    k = len(ref["kept"])
    assert ref["kept"][:, 5:8].tolist() == [[125, 0, 0], [5, 3, 1], [20, 10, 2], [50, 30, 3]]
    assert ref["labels"][0, w - 1] == 0 and ref["labels"][4, 0] == 1
    edited = {}

    def edit(regs, nkept):
        rows = []
        for src, sx, sy, cid in [(1, w, 3, 1),               # x = w: aliases (0, 4), which carries id 1
                                 (0, -1, 1, 0),              # x = -1 on row 1: aliases (w - 1, 0), which carries id 0
                                 (0, 50, h, 0),              # y = h: aliases image 1's (50, 0), which carries id 0
                                 (2, 20, 10, 3),             # the seed pixel carries another id
                                 (2, 20, 11, 2),             # not the first pixel: the pixel above is the blob's own
                                 (3, 60, 30, -1),            # a background pixel "carries" -1
                                 (3, 50, 30, 3)]:            # and an untouched copy, behind them
            r = regs[0, src].copy()
            r[5:8] = [sx, sy, cid]
            rows.append(r)
        regs[0, k:k + len(rows)] = rows
        nkept[0] = k + len(rows)
        edited["recs"] = regs[0, :nkept[0]].copy()
    full = np.full((h, w), 255, np.uint8)                    # image 1: every label is 0
    out = run_parents(ctx, [m, full], edit=edit, hulls=True)
    recs = edited["recs"]
    want = parents_by_rule(ref["labels"], recs)
    assert want.tolist() == [-1, -1, -1, 2] + [UNKNOWN] * 6 + [2]
    same(out, 0, ref, want=want, recs=recs)
    assert np.array_equal(out["labels"][0], ref["labels"])
    assert out["next"][0] == 3
    assert same(out, 1, regions_reference(full, open3=False)).tolist() == [-1]


@pytest.mark.gpu
def test_batch_of_32_equals_single_calls(mdx):
    masks = []
    for seed in range(32):
        m = nested_outlines(0 if seed % 8 == 0 else 100 + seed)
        f = np.zeros((67, 130), np.uint8)
        f[:m.shape[0], :m.shape[1]] = m
        masks.append(np.roll(f, seed, 1) if seed % 3 == 0 else f)
    with mdx.Context(0, 320, 240, 1) as c:
        batch = run_parents(c, masks, hulls=True)
        for i in (0, 5, 17, 31):
            solo = run_parents(c, [masks[i]], hulls=True)
            for k in ("regs", "nkept", "parent", "ext", "next", "offsets", "xy", "nv"):
                assert batch[k][i].tobytes() == solo[k][0].tobytes(), (i, k)
        for i, m in enumerate(masks):
            same(batch, i, regions_reference(m, open3=False))
        assert len(set(batch["parent"][i].tobytes() for i in range(32))) > 16


@pytest.mark.gpu
def test_nested_then_empty_then_nested_sees_no_stale_scratch(mdx):
    with mdx.Context(0, 320, 240, 1) as c:
        m, ref, rule = outline_case(0)
        a = run_parents(c, [m])
        same(a, 0, ref, want=rule)
        e = np.zeros_like(m)
        same(run_parents(c, [e]), 0, regions_reference(e, open3=False))
        full = np.full_like(m, 255)
        assert same(run_parents(c, [full]), 0, regions_reference(full, open3=False)).tolist() == [-1]
        small = ring7()
        assert same(run_parents(c, [small]), 0, regions_reference(small, open3=False)).tolist() == [-1, 0]
        b = run_parents(c, [m])
        for k in ("parent", "ext", "next"):
            assert a[k].tobytes() == b[k].tobytes(), k       # the same call twice: identical bytes


@pytest.mark.gpu
def test_einval_cases_leave_the_outputs_untouched(mdx, ctx):
    L = mdx.lib()
    w, h, M = 16, 8, 4
    m = patterns(w, h)["thick_comb"]
    vp = C.c_void_p
    out = run_parents(ctx, [m], max_regions=M)
    words = 4096
    d = ctx.dev_alloc(words * 4)
    try:
        img = np.full(words, AA, np.int32)
        img[:w * h] = out["labels"][0].ravel()
        img[1024:1024 + 8 * M] = out["regs"][0].ravel()
        img[1100] = out["nkept"][0]
        ctx.h2d(d, img)
        lab, rec, nk, par, ext, nx = (vp(d + 4 * o) for o in (0, 1024, 1100, 2048, 2100, 2090))
        ok = dict(batch=1, labels=lab, w=w, h=h, regions=rec, max_regions=M, num_kept=nk, parent=par, ext=ext, nx=nx)

        def dev(**kw):
            a = dict(ok, **kw)
            return L.mdx_region_parents_dev(ctx._h, a["batch"], a["labels"], a["w"], a["h"], a["regions"], a["max_regions"],
                                            a["num_kept"], a["parent"], a["ext"], a["nx"])
        bad = [dict(batch=0), dict(batch=-1), dict(w=0), dict(h=0), dict(w=-3), dict(w=1 << 13, h=(1 << 17) + 1),
               dict(max_regions=-1), dict(labels=None), dict(regions=None), dict(num_kept=None), dict(ext=rec),
               dict(ext=vp(d + 4 * 1024 + 32)), dict(ext=vp(d + 4 * 1024 - 32 * M + 4))]
        for kw in bad:
            assert dev(**kw) == -1, kw
            assert b"mdx_region_parents_dev" in L.mdx_last_error(ctx._h)
        ctx.sync()
        back = np.empty_like(img)
        ctx.d2h(back, d)
        assert np.array_equal(back, img)                              # no rejected call wrote anything
        assert dev(ext=vp(d + 4 * 1024 + 32 * M)) == 0                # right behind the records: no overlap
        assert dev(regions=None, num_kept=None, max_regions=0) == 0   # nothing asked: NULLs are fine, next = 0
        ctx.sync()
        ctx.d2h(back, d)
        assert back[2090] == 0
        assert dev() == 0
        ctx.sync()
        ctx.d2h(back, d)
        ne = out["next"][0]
        assert back[2090] == ne and np.array_equal(back[2048:2048 + M], out["parent"][0])
        assert np.array_equal(back[2100:2100 + 8 * ne], out["ext"][0, :ne].ravel())
    finally:
        ctx.dev_free(d)
    # the host entry: mdx_mask_regions' errors, plus the hulls' when offsets is given
    p = lambda a: a.ctypes.data_as(vp)   # noqa: E731
    V = 32
    regs, par, ext = np.full((M, 8), AA, np.int32), np.full(M, AA, np.int32), np.full(M, AA, np.int32)
    offs, pts = np.full(M + 1, AA, np.int32), np.full((V, 2), AA, np.int32)
    cnt = [C.c_int(-5) for _ in range(4)]
    okh = dict(mask=p(m), w=w, h=h, stride=w, flags=0, regions=p(regs), max_regions=M, offsets=p(offs), xy=p(pts),
               max_vertices=V)

    def hst(**kw):
        a = dict(okh, **kw)
        return L.mdx_mask_regions_tree(ctx._h, a["mask"], a["w"], a["h"], a["stride"], a["flags"], 1, a["regions"],
                                       a["max_regions"], C.byref(cnt[0]), C.byref(cnt[1]), p(par), p(ext), C.byref(cnt[2]),
                                       a["offsets"], a["xy"], a["max_vertices"], C.byref(cnt[3]))
    wide = np.zeros((1, 8193), np.uint8)
    for kw in [dict(mask=None), dict(w=0), dict(h=-1), dict(stride=w - 1), dict(w=1 << 13, h=(1 << 17) + 1, stride=1 << 13),
               dict(max_regions=-1), dict(regions=None), dict(flags=8), dict(flags=2), dict(flags=4),
               dict(mask=p(wide), w=8193, h=1, stride=8193), dict(max_vertices=-1), dict(xy=None)]:
        assert hst(**kw) == -1, kw
        assert b"mdx_mask_regions_tree" in L.mdx_last_error(ctx._h)
    for a in (regs, par, ext, offs, pts):
        assert (a == AA).all()
    assert [v.value for v in cnt] == [-5] * 4
    assert hst() == 0 and hst(xy=None, max_vertices=0) == 0 and hst(regions=None, max_regions=0) == 0
    assert offs[0] == 0 and cnt[2].value == 0 and cnt[3].value == 0   # max_regions 0: no record takes part
    # without offsets the hull arguments are ignored, a frame wider than the hulls' span included
    assert hst(offsets=None, xy=None, max_vertices=-1) == 0
    assert hst(mask=p(wide), w=8193, h=1, stride=8193, offsets=None) == 0


# ---------------------------------------------------------------- the host entry and the Python wrapper

@pytest.mark.gpu
def test_host_entry_equals_the_device_chain(mdx, ctx):
    L = mdx.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    for m, open3, min_area in [(outline_case(0)[0], False, 1), (patterns(257, 129)["random_0.60"], False, 4),
                               (patterns(257, 129)["random_0.60"], True, 4), (thin_ring_case(), False, 1)]:
        h, w = m.shape
        ref = regions_reference(m, open3=open3, min_area=min_area)
        dev = run_parents(ctx, [m], open3=open3, min_area=min_area, hulls=True)
        want = same(dev, 0, ref)
        k, ne, nvd = len(ref["kept"]), int(dev["next"][0]), int(dev["nv"][0])
        idx = np.flatnonzero(want == NO_PARENT)
        pitched = np.full((h, w + 43), 0xFF, np.uint8)
        pitched[:, :w] = m
        cap, maxv = k + 3, nvd + 5
        regs, par, ext = np.full((cap, 8), AA, np.int32), np.full(cap, AA, np.int32), np.full(cap, AA, np.int32)
        off, xy = np.full(cap + 1, AA, np.int32), np.full((maxv, 2), AA, np.int32)
        nall, nkept, next_, nv = (C.c_int(-5) for _ in range(4))
        assert L.mdx_mask_regions_tree(ctx._h, p(pitched), w, h, w + 43, OPEN3 if open3 else 0, min_area, p(regs), cap,
                                       C.byref(nall), C.byref(nkept), p(par), p(ext), C.byref(next_), p(off), p(xy), maxv,
                                       C.byref(nv)) == 0
        assert (nall.value, nkept.value, next_.value, nv.value) == (ref["num_all"], k, ne, nvd)
        assert np.array_equal(regs[:k], ref["kept"]) and (regs[k:] == AA).all()
        assert np.array_equal(par[:k], want) and (par[k:] == AA).all()
        assert np.array_equal(ext[:ne], idx) and (ext[ne:] == AA).all()
        assert np.array_equal(off, np.concatenate([dev["offsets"][0, :ne + 1], [nvd] * (cap - ne)]))
        assert np.array_equal(xy[:nvd], dev["xy"][0, :nvd]) and (xy[nvd:] == AA).all()
        # offsets NULL: no hulls, everything else the same; parent and external_index may be NULL too
        par[:] = ext[:] = AA
        nv.value = -5
        assert L.mdx_mask_regions_tree(ctx._h, p(pitched), w, h, w + 43, OPEN3 if open3 else 0, min_area, p(regs), cap,
                                       None, None, p(par), p(ext), C.byref(next_), None, None, 0, C.byref(nv)) == 0
        assert np.array_equal(par[:k], want) and np.array_equal(ext[:ne], idx) and nv.value == -5
        ext[:] = AA
        assert L.mdx_mask_regions_tree(ctx._h, p(pitched), w, h, w + 43, OPEN3 if open3 else 0, min_area, p(regs), cap,
                                       None, None, None, p(ext), None, None, None, 0, None) == 0
        assert np.array_equal(ext[:ne], idx) and (ext[ne:] == AA).all()
        # the wrapper
        r = ctx.mask_regions(m, open3=open3, min_area=min_area, want_parents=True, want_hulls=True)
        assert isinstance(r, mdx.RegionTreeResult) and isinstance(r, mdx.RegionResult)
        assert (r.num_all, r.num_kept) == (ref["num_all"], k) and np.array_equal(r.regions, ref["kept"])
        assert np.array_equal(r.parent, want) and np.array_equal(r.external, idx)
        assert r.external_rectangles == [tuple(v[:4]) for v in ref["kept"][idx].tolist()]
        hulls = expected_hulls(ref["labels"], ref["kept"][idx])
        assert len(r.hulls) == ne and all(a.tolist() == [list(q) for q in b] for a, b in zip(r.hulls, hulls))
        q = ctx.mask_regions(m, open3=open3, min_area=min_area, want_parents=True, want_labels=True)
        assert q.hulls is None and np.array_equal(q.parent, want) and np.array_equal(q.labels, ref["labels"])
        plain = ctx.mask_regions(m, open3=open3, min_area=min_area)
        assert type(plain) is mdx.RegionResult


# ---------------------------------------------------------------- end to end: chained behind the pair entry

def _chain(mdx, masks_in=None):
    """mdx_flow_warp_diff_batch_dev -> mdx_mask_regions_dev -> mdx_region_parents_dev -> mdx_region_hulls_dev on
    d_external, one stream, no sync in between.  masks_in: hand-made masks fed in as the mask instead."""
    w, h = 160, 120
    B = 1 if masks_in is None else len(masks_in)
    cap, maxv = 64, 2048
    with mdx.Context(0, w, h, B, fit_mode=mdx.FIT_EXTERNAL, thresh=30) as c:
        host = dict(regs=np.full((B, cap, 8), AA, np.int32), nall=np.full(B, AA, np.int32),
                    nkept=np.full(B, AA, np.int32), mask=np.full((B, h, w), 0xAA, np.uint8),
                    labels=np.full((B, h, w), AA, np.int32), parent=np.full((B, cap), AA, np.int32),
                    ext=np.full((B, cap, 8), AA, np.int32), next=np.full(B, AA, np.int32),
                    offsets=np.full((B, cap + 1), AA, np.int32), xy=np.full((B, maxv, 2), AA, np.int32),
                    nv=np.full(B, AA, np.int32))
        if masks_in is not None:
            host["mask"] = np.stack(masks_in)
        d = {k: c.dev_alloc(v.nbytes) for k, v in host.items()}
        try:
            for k, v in host.items():
                c.h2d(d[k], v)
            if masks_in is None:
                g = np.load(os.path.join(ROOT, "tests", "golden", "synth_160x120_rgb.npz"))
                # the identity as the external fit: the mask is the frame difference, which has blobs of every size
                g1, g2, Hs = g["img1"][None].copy(), g["img2"][None].copy(), np.eye(3)[None].copy()
                n = mdx.grid_count(w, h, c.params.pixel_step)
                d.update(i1=c.dev_alloc(g1.nbytes), i2=c.dev_alloc(g2.nbytes), H=c.dev_alloc(Hs.nbytes),
                         np=c.dev_alloc(B * n * 8), st=c.dev_alloc(B * n))
                c.h2d(d["i1"], g1), c.h2d(d["i2"], g2), c.h2d(d["H"], Hs)
                c.flow_warp_diff_batch_dev(B, d["i1"], d["i2"], w, h, 3 * w, 3 * w * h, mdx.FMT_RGB8, d["np"], d["st"], 0,
                                           d["mask"], 0, d["H"], 0)
            min_area = 50 if masks_in is None else 1
            c.mask_regions_dev(B, d["mask"], w, h, w, w * h, masks_in is None, min_area, d["regs"], cap, d["nall"],
                               d["nkept"], d["labels"])
            c.region_parents_dev(B, d["labels"], w, h, d["regs"], cap, d["nkept"], d["parent"], d["ext"], d["next"])
            c.region_hulls_dev(B, d["labels"], w, h, d["ext"], cap, d["next"], d["offsets"], d["xy"], maxv, d["nv"])
            c.sync()
            for k, v in host.items():
                c.d2h(v, d[k])
        finally:
            for p in d.values():
                c.dev_free(p)
    host.update(cap=cap, maxv=maxv, hulls=True, want=("parent", "ext", "next"))
    pars = []
    for i in range(B):
        ref = regions_reference(host["mask"][i], open3=masks_in is None, min_area=50 if masks_in is None else 1)
        assert host["nall"][i] == ref["num_all"] and host["nkept"][i] >= 1   # else the comparison is vacuous
        pars.append(same(host, i, ref))
    return pars


@pytest.mark.gpu
def test_chained_behind_the_pair_entry(mdx):
    _chain(mdx)


@pytest.mark.gpu
def test_chained_on_a_hand_made_nested_mask(mdx):
    m = np.zeros((120, 160), bool)
    outline_rect(m, 10, 10, 150, 110)
    outline_diamond(m, 64, 64, 30)
    m[60:70, 60:70] = True
    m[20:25, 100:140] = True
    m[0:3, 0:5] = True
    pars = _chain(mdx, [u8(m), u8(m[::-1]), u8(m.T[:120, :].repeat(2, 1)[:, :160])])
    assert pars[0].tolist() == [-1, -1, 1, 1, 3]
