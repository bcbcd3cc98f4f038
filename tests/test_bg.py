"""Background subtraction (include/mdx.h mdx_bg_*): the MOG2 mixture model, its mask and its
background image.

Two independent restatements of the header's contract run on the CPU: tests/bg_check.cpp (scalar C++, one pixel
at a time, compiled here with g++ -O1 -ffp-contract=off) and np_run below (numpy float32, vectorised over the
pixels, looping over the modes).  They must agree on every output word of every case, and the C++ one's branch
counters must all be positive over the case set, so the inputs are known to reach every branch of the rule.  The
GPU tests then compare every mask byte, every background byte, `modes` and every state float (as uint32, below
`modes`) of the device with the C++ oracle, from 0xAA-prefilled outputs.
"""
import ctypes as C
import functools
import os
import re
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
DEFAULTS = dict(history=500, nmixtures=5, var_threshold=16.0, var_threshold_gen=9.0, background_ratio=0.9, var_init=15.0,
                var_min=4.0, var_max=75.0, ct=0.05, detect_shadows=1, shadow_value=127, tau=0.5)
COUNTERS = ("fit_mode0", "fit_swapped", "var_clamp_low", "var_clamp_high", "prune_last", "prune_not_last", "new_appended",
            "new_replaced", "new_bubbled", "shadow_true", "shadow_false_tw", "shadow_den_zero", "background_not_first",
            "image_break_early")
QNAN = 0x7FC00000


def params_of(**kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        assert k in p, k
        p[k] = v
    return p


def pack_params(p):
    return struct.pack("<ii7fiif", p["history"], p["nmixtures"], p["var_threshold"], p["var_threshold_gen"],
                       p["background_ratio"], p["var_init"], p["var_min"], p["var_max"], p["ct"], p["detect_shadows"],
                       p["shadow_value"], p["tau"])


def alpha_of(p, nframes, lr):
    if lr >= 0 and nframes > 1:
        return f32(lr)
    return f32(1.0 / min(2 * nframes, p["history"]))


def empty_state(h, w, cn, nm):
    return dict(weight=np.zeros((h, w, nm), f32), variance=np.zeros((h, w, nm), f32), mean=np.zeros((h, w, nm, cn), f32),
                modes=np.zeros((h, w), np.uint8), nframes=0)


def canonical(st):
    """A state as the entries report it: nothing at or above a pixel's count, a NaN as 0x7fc00000; floats as uint32."""
    nm = st["weight"].shape[2]
    live = np.arange(nm)[None, None, :] < st["modes"][:, :, None]
    out = dict(modes=st["modes"].copy(), nframes=int(st["nframes"]))
    for k in ("weight", "variance", "mean"):
        a = np.ascontiguousarray(st[k], f32)
        u = a.view(np.uint32).copy()
        u[np.isnan(a)] = QNAN
        out[k] = np.where(live if k != "mean" else live[..., None], u, 0).astype(np.uint32)
    return out


# ---------------------------------------------------------------- the C++ restatement

@functools.lru_cache(maxsize=None)
def bg_exe():
    if shutil.which("g++") is None:
        return None
    d = tempfile.mkdtemp(prefix="bg_check_")
    exe = os.path.join(d, "bg_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "bg_check.cpp"), "-o", exe],
                   check=True)
    return exe


def cpp_run(frames, p, lr=-1.0, state=None):
    """frames (T, h, w, cn) uint8 -> masks, images (after each frame), the final canonical state, the counters."""
    exe = bg_exe()
    T, h, w, cn = frames.shape
    nm = p["nmixtures"]
    blob = struct.pack("<6i", w, h, cn, T, 1 if state else 0, state["nframes"] if state else 0) + pack_params(p)
    blob += struct.pack("<d", lr) + np.ascontiguousarray(frames).tobytes()
    if state:
        for k, t in (("weight", f32), ("variance", f32), ("mean", f32), ("modes", np.uint8)):
            blob += np.ascontiguousarray(state[k], t).tobytes()
    d = os.path.dirname(exe)
    fd, fin = tempfile.mkstemp(dir=d)
    with os.fdopen(fd, "wb") as f:
        f.write(blob)
    fout = fin + ".out"
    try:
        subprocess.run([exe, fin, fout], check=True)
        raw = np.fromfile(fout, np.uint8)
    finally:
        for f in (fin, fout):
            if os.path.exists(f):
                os.remove(f)
    n, o = h * w, 0

    def take(count, dtype, shape):
        nonlocal o
        nb = count * np.dtype(dtype).itemsize
        a = raw[o:o + nb].view(dtype).reshape(shape).copy()
        o += nb
        return a
    res = dict(masks=take(T * n, np.uint8, (T, h, w)), images=take(T * n * cn, np.uint8, (T, h, w, cn)))
    st = dict(weight=take(n * nm, np.uint32, (h, w, nm)), variance=take(n * nm, np.uint32, (h, w, nm)),
              mean=take(n * nm * cn, np.uint32, (h, w, nm, cn)), modes=take(n, np.uint8, (h, w)))
    st["nframes"] = int(take(1, np.int32, (1,))[0])
    res["state"] = st
    res["counters"] = dict(zip(COUNTERS, (int(v) for v in take(len(COUNTERS), np.int64, (len(COUNTERS),)))))
    assert o == len(raw)
    return res


# ---------------------------------------------------------------- the numpy restatement

def _swap(wt, vr, mu, sel, i):
    idx = np.nonzero(sel)[0]
    for a in (wt, vr, mu):
        t = a[idx, i].copy()
        a[idx, i] = a[idx, i - 1]
        a[idx, i - 1] = t


def _seq_sum(terms):
    s = terms[0]
    for t in terms[1:]:
        s = s + t
    return s


def np_frame(wt, vr, mu, modes, data, alphaT, p):
    """One frame over all pixels: wt, vr (N, nm), mu (N, nm, cn), modes (N,) int, data (N, cn) float32; in place."""
    N, nm = wt.shape
    cn = data.shape[1]
    Tb, Tg, TB, tau = f32(p["var_threshold"]), f32(p["var_threshold_gen"]), f32(p["background_ratio"]), f32(p["tau"])
    vmin, vmax = f32(p["var_min"]), f32(p["var_max"])
    alphaT = f32(alphaT)
    alpha1 = f32(1.0) - alphaT
    prune = -alphaT * f32(p["ct"])
    n = modes.astype(np.int64).copy()
    n0 = n.copy()
    fits, bgd, total = np.zeros(N, bool), np.zeros(N, bool), np.zeros(N, f32)
    rows = np.arange(N)
    for m in range(nm):
        act = m < n
        w = alpha1 * wt[:, m] + prune
        swaps = np.zeros(N, np.int64)
        tryfit = act & ~fits
        var = vr[:, m].copy()
        d = mu[:, m, :] - data
        dist2 = _seq_sum([d[:, c] * d[:, c] for c in range(cn)])
        bgd |= tryfit & (total < TB) & (dist2 < Tb * var)
        fit = tryfit & (dist2 < Tg * var)
        fits |= fit
        w = np.where(fit, w + alphaT, w)
        k = alphaT / w
        newmu = mu[:, m, :] - k[:, None] * d
        mu[fit, m, :] = newmu[fit]
        vn = var + k * (dist2 - var)
        vn = np.where(vn > vmin, vn, vmin)
        vn = np.where(vn < vmax, vn, vmax)
        vr[fit, m] = vn[fit]
        go = fit.copy()
        for i in range(m, 0, -1):
            go &= ~(w < wt[:, i - 1])
            _swap(wt, vr, mu, go, i)
            swaps += go
        pr = act & (w < -prune)
        w = np.where(pr, f32(0), w)
        n = n - pr
        wt[rows[act], (m - swaps)[act]] = w[act]
        total = np.where(act, total + w, total)
    inv = f32(1.0) / total
    for m in range(nm):
        sel = m < n
        wt[sel, m] = wt[sel, m] * inv[sel]
    n = n0
    nf = ~fits
    n = np.where(nf & (n != nm), n + 1, n)
    one = n == 1
    slot = n - 1
    for j in range(nm):
        sel = nf & ~one & (j < n - 1)
        wt[sel, j] = wt[sel, j] * alpha1
    wt[rows[nf], slot[nf]] = np.where(one[nf], f32(1), alphaT)
    mu[rows[nf], slot[nf], :] = data[nf]
    vr[rows[nf], slot[nf]] = f32(p["var_init"])
    go = nf.copy()
    for i in range(nm - 1, 0, -1):
        cond = go & (i <= n - 1)
        brk = cond & (alphaT < wt[:, i - 1])
        go &= ~brk
        _swap(wt, vr, mu, cond & ~brk, i)
    modes[:] = n
    # detectShadowGMM on the updated state
    res, done, tw = np.zeros(N, bool), np.zeros(N, bool), np.zeros(N, f32)
    for m in range(nm):
        act = (m < n) & ~done
        num = _seq_sum([f32(0)] + [data[:, c] * mu[:, m, c] for c in range(cn)])
        den = _seq_sum([f32(0)] + [mu[:, m, c] * mu[:, m, c] for c in range(cn)])
        dz = act & (den == 0)
        done |= dz
        act = act & ~dz
        a = num / den
        s = _seq_sum([f32(0)] + [(a * mu[:, m, c] - data[:, c]) * (a * mu[:, m, c] - data[:, c]) for c in range(cn)])
        hit = act & (num <= den) & (num >= tau * den) & (s < Tb * vr[:, m] * a * a)
        res |= hit
        done |= hit
        act = act & ~hit
        tw = np.where(act, tw + wt[:, m], tw)
        done |= act & (tw > TB)
    shadow = res if p["detect_shadows"] else np.zeros(N, bool)
    return np.where(bgd, 0, np.where(shadow, p["shadow_value"], 255)).astype(np.uint8)


def np_image(wt, mu, modes, p):
    N, nm = wt.shape
    cn = mu.shape[2]
    TB = f32(p["background_ratio"])
    acc, tot, done = np.zeros((N, cn), f32), np.zeros(N, f32), np.zeros(N, bool)
    for m in range(nm):
        act = (m < modes) & ~done
        acc[act] = acc[act] + wt[act, m][:, None] * mu[act, m, :]
        tot[act] = tot[act] + wt[act, m]
        done |= act & (tot > TB)
    v = acc * (f32(1.0) / tot)[:, None]
    v = np.where(v >= 0, v, f32(0))
    v = np.where(v > 255, f32(255), v)
    return np.where((modes > 0)[:, None], np.rint(v), 0).astype(np.uint8)


def np_run(frames, p, lr=-1.0, state=None):
    T, h, w, cn = frames.shape
    nm, N = p["nmixtures"], h * w
    st = state or empty_state(h, w, cn, nm)
    wt = np.array(st["weight"], f32).reshape(N, nm)
    vr = np.array(st["variance"], f32).reshape(N, nm)
    mu = np.array(st["mean"], f32).reshape(N, nm, cn)
    modes = np.array(st["modes"]).astype(np.int64).reshape(N)
    nframes = int(st["nframes"])
    masks, images = np.zeros((T, h, w), np.uint8), np.zeros((T, h, w, cn), np.uint8)
    with np.errstate(all="ignore"):
        for t in range(T):
            nframes += 1
            data = frames[t].reshape(N, cn).astype(f32)
            masks[t] = np_frame(wt, vr, mu, modes, data, alpha_of(p, nframes, lr), p).reshape(h, w)
            images[t] = np_image(wt, mu, modes, p).reshape(h, w, cn)
    fin = dict(weight=wt.reshape(h, w, nm), variance=vr.reshape(h, w, nm), mean=mu.reshape(h, w, nm, cn),
               modes=modes.astype(np.uint8).reshape(h, w), nframes=nframes)
    return dict(masks=masks, images=images, state=canonical(fin))


# ---------------------------------------------------------------- the cases

def _scene(rng, h, w, cn):
    s = rng.integers(40, 200, (h, w, cn)).astype(np.int64)
    s[:, : max(1, w // 5)] = 0                                      # a black band: a mode of mean 0 (den == 0)
    return s


def _noisy(rng, img, amp):
    return np.clip(img + rng.integers(-amp, amp + 1, img.shape), 0, 255).astype(np.uint8)


def seq_moving(seed, w, h, cn, T=12, amp=13):
    """A noisy static scene with a bright square moving two pixels a frame."""
    rng = np.random.default_rng(seed)
    base = _scene(rng, h, w, cn)
    side = max(1, min(8, w // 2, h // 2))
    out = []
    for t in range(T):
        f = base.copy()
        x0, y0 = (2 * t) % max(1, w - side + 1), t % max(1, h - side + 1)
        f[y0:y0 + side, x0:x0 + side] = 250
        out.append(_noisy(rng, f, amp))
    return np.stack(out)


def seq_darken(seed, w, h, cn, T=12, amp=3):
    """A scene that darkens to 0.6 of itself half way (shadows)."""
    rng = np.random.default_rng(seed)
    base = _scene(rng, h, w, cn)
    return np.stack([_noisy(rng, base if t < T // 2 else (base * 6) // 10, amp) for t in range(T)])


def seq_bimodal(seed, w, h, cn, T=12, amp=2):
    """A scene that alternates between two backgrounds, unevenly."""
    rng = np.random.default_rng(seed)
    a, b = _scene(rng, h, w, cn), _scene(rng, h, w, cn)
    order = [0, 0, 0, 1, 0, 1, 1, 0, 1, 1, 1, 0] * ((T + 11) // 12)
    return np.stack([_noisy(rng, b if order[t] else a, amp) for t in range(T)])


def crafted(cn, nm, rows):
    """A 1-row state: rows = [(modes, [(weight, variance, mean), ...]), ...], every channel of a mode at `mean`."""
    st = empty_state(1, len(rows), cn, nm)
    for x, (n, ms) in enumerate(rows):
        st["modes"][0, x] = n
        for m, (wgt, var, mean) in enumerate(ms):
            st["weight"][0, x, m], st["variance"][0, x, m], st["mean"][0, x, m, :] = wgt, var, mean
    st["nframes"] = 50
    return st


def _flat(values, cn, T=1):
    """T identical 1-row frames whose pixel x holds values[x] in every channel."""
    f = np.zeros((T, 1, len(values), cn), np.uint8)
    f[:, 0, :, :] = np.asarray(values, np.uint8)[None, :, None]
    return f


def crafted_cases(cn):
    """Starting states built to reach the branches the sequences leave to chance; one pixel each, described by
    (state row, frame value).  The asserts on the counters (test_counters_all_reached) are what holds them to it."""
    nm = 3
    rows = [
        # fit at mode 1 whose weight then exceeds mode 0's: one swap
        ((2, [(0.5, 15.0, 100.0), (0.5, 15.0, 50.0)]), 50),
        # variance clamped low (a near-perfect fit of a mode at var_min) and high (a far fit at var_max)
        ((1, [(1.0, 4.0, 80.0)]), 80),
        ((1, [(1.0, 75.0, 80.0)]), 80 + (25 if cn == 1 else 14)),
        # the last mode pruned; a middle mode pruned (the loop bound shrinks, the last mode is skipped)
        ((2, [(0.99, 15.0, 100.0), (0.001, 15.0, 30.0)]), 100),
        ((3, [(0.9, 15.0, 100.0), (0.001, 15.0, 30.0), (0.099, 15.0, 200.0)]), 100),
        # no fit: appended; replacing the weakest of a full mixture; bubbled above a weaker older mode
        ((1, [(1.0, 15.0, 100.0)]), 200),
        ((3, [(0.6, 15.0, 100.0), (0.3, 15.0, 30.0), (0.1, 15.0, 60.0)]), 200),
        ((2, [(0.995, 15.0, 100.0), (0.005, 15.0, 30.0)]), 200),
        # shadow: 0.6 of a learnt grey; the same value not fitting with tw > TB; a black first mode (den == 0)
        ((1, [(1.0, 15.0, 200.0)]), 120),
        ((1, [(1.0, 15.0, 100.0)]), 250),
        ((1, [(1.0, 15.0, 0.0)]), 90),
        # background through the second mode: the first holds less than TB and does not match
        ((2, [(0.5, 15.0, 100.0), (0.5, 15.0, 50.0)]), 51),
        # the image's sum stops at the first mode
        ((2, [(0.95, 15.0, 100.0), (0.05, 15.0, 30.0)]), 100),
        # a NaN weight in the state comes back as 0x7fc00000
        ((2, [(float("nan"), 15.0, 100.0), (0.5, 15.0, 50.0)]), 100),
    ]
    st = crafted(cn, nm, [r[0] for r in rows])
    return dict(frames=_flat([r[1] for r in rows], cn, T=2), p=params_of(nmixtures=nm, history=20), lr=-1.0, state=st)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(frames, p, lr, state, pitch): pitch is the extra bytes per row the GPU tests add (0: packed)."""
    out = {}

    def add(name, frames, pitch=0, lr=-1.0, state=None, **p):
        out[name] = dict(frames=frames, p=params_of(**p), lr=lr, state=state, pitch=pitch)
    add("moving_67x35_rgb", seq_moving(1, 67, 35, 3))
    add("moving_67x35_gray_pitch3", seq_moving(2, 67, 35, 1), pitch=3)
    add("darken_64x8_rgb_pitch5", seq_darken(3, 64, 8, 3), pitch=5)
    add("darken_64x8_gray_noshadow", seq_darken(4, 64, 8, 1), detect_shadows=0)
    add("darken_67x35_rgb_noshadow_pitch4", seq_darken(5, 67, 35, 3), pitch=4, detect_shadows=0)
    add("bimodal_64x8_gray_h4", seq_bimodal(6, 64, 8, 1), history=4)
    add("bimodal_67x35_rgb_h4_nm3_pitch1", seq_bimodal(7, 67, 35, 3), pitch=1, history=4, nmixtures=3)
    add("bimodal_64x8_gray_nm8", seq_bimodal(8, 64, 8, 1), nmixtures=8)
    add("moving_1x1_gray", seq_moving(9, 1, 1, 1, amp=40))
    add("moving_1x1_rgb_h4", seq_moving(10, 1, 1, 3, amp=40), history=4)
    add("moving_257x3_rgb_nm8_h4", seq_moving(11, 257, 3, 3, amp=25), nmixtures=8, history=4)
    add("moving_257x3_gray_nm1_pitch2", seq_moving(12, 257, 3, 1), pitch=2, nmixtures=1)
    add("moving_257x3_rgb_nm1_h8", seq_moving(13, 257, 3, 3), nmixtures=1, history=8)
    add("moving_64x8_gray_lr0", seq_moving(14, 64, 8, 1), lr=0.0)
    add("bimodal_64x8_rgb_lr05", seq_bimodal(15, 64, 8, 3), lr=0.5)
    add("moving_67x35_gray_lr1_nm3", seq_moving(16, 67, 35, 1), lr=1.0, nmixtures=3)
    add("moving_64x8_rgb_lr1_h4", seq_moving(17, 64, 8, 3), lr=1.0, history=4)
    add("moving_64x8_gray_nm8_h8_noisy", seq_moving(18, 64, 8, 1, amp=40), nmixtures=8, history=8)
    add("moving_67x35_rgb_nm3_h8_noisy", seq_moving(19, 67, 35, 3, amp=30), nmixtures=3, history=8)
    for cn in (1, 3):
        c = crafted_cases(cn)
        add(f"crafted_{cn}", c["frames"], state=c["state"], **{k: c["p"][k] for k in ("nmixtures", "history")})
    return out


CASE_NAMES = sorted(cases())


@functools.lru_cache(maxsize=None)
def reference(name):
    """The C++ oracle's result of a case, computed once and shared (never modified by a test)."""
    c = cases()[name]
    return cpp_run(c["frames"], c["p"], c["lr"], c["state"])


needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def assert_same(got, ref, what, fields=("masks", "images", "state")):
    for k in fields:
        if k == "state":
            assert np.array_equal(got["state"]["modes"], ref["state"]["modes"]), f"{what}: modes"
            assert got["state"]["nframes"] == ref["state"]["nframes"], f"{what}: nframes"
            for f in ("weight", "variance", "mean"):
                bad = np.argwhere(got["state"][f] != ref["state"][f])
                assert len(bad) == 0, f"{what}: {f} differs at {bad[:4].tolist()} ({len(bad)} words)"
        else:
            bad = np.argwhere(got[k] != ref[k])
            assert len(bad) == 0, f"{what}: {k} differs at {bad[:4].tolist()} ({len(bad)} bytes)"


# ---------------------------------------------------------------- CPU

@needs_gxx
@pytest.mark.parametrize("name", CASE_NAMES)
def test_two_restatements_agree(name):
    c = cases()[name]
    assert_same(np_run(c["frames"], c["p"], c["lr"], c["state"]), reference(name), name)


@needs_gxx
def test_counters_all_reached():
    total = dict.fromkeys(COUNTERS, 0)
    for name in CASE_NAMES:
        for k, v in reference(name)["counters"].items():
            total[k] += v
    print(total)
    assert all(v > 0 for v in total.values()), total
    # the crafted states reach theirs on their own
    for cn in (1, 3):
        got = reference(f"crafted_{cn}")["counters"]
        assert all(got[k] > 0 for k in COUNTERS), got


@needs_gxx
@pytest.mark.parametrize("restate", [cpp_run, np_run])
@pytest.mark.parametrize("cn", [1, 3])
def test_constant_stream_known_answers(restate, cn):
    """Mask 255 on frame 1 and 0 from frame 2 on, one mode of weight 1 whose mean is the value, the background equal
    to the frame.  The 255 is the answer with shadows off.  With them on (the default) rule 5 runs shadow() on the
    UPDATED state, where the mode just created from the pixel matches it exactly (num == den, a == 1, s == 0), so
    frame 1 is shadow_value: a quirk of the source that the contract keeps, and that is pinned here too."""
    frames = np.full((6, 5, 7, cn), 93, np.uint8)
    for shadows, first in ((0, 255), (1, 127)):
        r = restate(frames, params_of(detect_shadows=shadows))
        assert (r["masks"][0] == first).all() and (r["masks"][1:] == 0).all()
        st = r["state"]
        assert (st["modes"] == 1).all() and st["nframes"] == 6
        assert (st["weight"][..., 0].view(f32) == 1.0).all() and (st["weight"][..., 1:] == 0).all()
        assert (st["mean"][:, :, 0, :].view(f32) == 93.0).all()
        assert (r["images"] == 93).all()                      # the background of that stream is the frame


@needs_gxx
@pytest.mark.parametrize("restate", [cpp_run, np_run])
@pytest.mark.parametrize("cn", [1, 3])
def test_shadow_known_answer(restate, cn):
    frames = np.full((9, 2, 2, cn), 200, np.uint8)
    frames[8] = 120                                       # 0.6 of the learnt grey
    assert (restate(frames, params_of())["masks"][8] == 127).all()
    assert (restate(frames, params_of(detect_shadows=0))["masks"][8] == 255).all()


def test_abi_params_defaults_and_version(mdx):
    from test_abi import HEADER, header_functions
    L = mdx.lib()
    assert L.mdx_bg_params_size() == C.sizeof(mdx._lib.MdxBgParams) == 48
    p = mdx._lib.bg_default_params()
    for k, v in DEFAULTS.items():
        assert getattr(p, k) == (f32(v) if isinstance(v, float) else v), k
    hdr = open(HEADER).read()
    assert int(re.search(r"#define MDX_ABI_VERSION (\d+)", hdr).group(1)) == mdx._lib.ABI_VERSION == L.mdx_abi_version() == 11
    assert int(re.search(r"#define MDX_BG_MAX_MIXTURES (\d+)", hdr).group(1)) == mdx._lib.BG_MAX_MIXTURES == 8
    assert int(re.search(r"#define MDX_BG_MAX_FRAMES_PER_LAUNCH (\d+)", hdr).group(1)) == mdx._lib.BG_MAX_FRAMES_PER_LAUNCH
    names = header_functions()
    for n in ("mdx_bg_default_params", "mdx_bg_params_size", "mdx_bg_create", "mdx_bg_destroy", "mdx_bg_reset",
              "mdx_bg_frames", "mdx_bg_apply_dev", "mdx_bg_image_dev", "mdx_bg_apply", "mdx_bg_image", "mdx_bg_get_state",
              "mdx_bg_set_state"):
        assert n in names and n in mdx._lib.EXPORTED and hasattr(L, n), n
    assert "mdx_bg.hip" in mdx._lib.STAMPED and "mdx_bg_api.cpp" in mdx._lib.STAMPED
    assert hasattr(mdx, "BackgroundSubtractor")


def test_null_context_is_einval(mdx):
    L = mdx.lib()
    out = C.c_void_p(0)
    assert L.mdx_bg_create(None, 1, 4, 4, 1, None, C.byref(out)) == mdx._lib.MDX_EINVAL and not out.value
    for f in (L.mdx_bg_destroy, L.mdx_bg_reset, L.mdx_bg_frames):
        assert f(None, None) == mdx._lib.MDX_EINVAL
    assert L.mdx_bg_apply_dev(None, None, 1, None, 4, 16, 0, -1.0, None) == mdx._lib.MDX_EINVAL
    assert L.mdx_bg_image_dev(None, None, None) == mdx._lib.MDX_EINVAL


# ---------------------------------------------------------------- GPU

class Model:
    """A device model of `streams` streams with the test's own 0xAA-prefilled frame, mask and image buffers."""

    def __init__(self, ctx, streams, w, h, cn, p, pitch=0, tmax=12):
        self.ctx, self.streams, self.w, self.h, self.cn, self.p = ctx, streams, w, h, cn, p
        self.stride = w * cn + pitch
        self.fbytes = self.stride * h                  # frames and streams lie back to back, pitch bytes included
        self.tmax = tmax
        self.bg = ctx.bg_create(streams, w, h, cn, **p)
        self.dev = []
        self.d_frames = self._alloc(streams * tmax * self.fbytes)
        self.d_mask = self._alloc(streams * tmax * w * h)
        self.d_image = self._alloc(streams * w * h * cn)

    def _alloc(self, n):
        self.dev.append(self.ctx.dev_alloc(n))
        return self.dev[-1]

    def close(self):
        self.ctx.sync()
        if self.bg:
            self.ctx.bg_destroy(self.bg)
        for d in self.dev:
            self.ctx.dev_free(d)
        self.bg, self.dev = 0, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def apply(self, frames, lr=-1.0, want_mask=True):
        """frames (streams, T, h, w, cn) -> masks (streams, T, h, w), in one call of T frames."""
        S, T = frames.shape[:2]
        assert S == self.streams and T <= self.tmax
        host = np.full((S, T, self.h, self.stride), 0xAA, np.uint8)       # the pitch bytes are 0xAA: never data
        host[:, :, :, :self.w * self.cn] = frames.reshape(S, T, self.h, self.w * self.cn)
        self.ctx.h2d(self.d_frames, host)
        masks = np.full((S, T, self.h, self.w), 0xAA, np.uint8)
        self.ctx.h2d(self.d_mask, masks)
        self.ctx.bg_apply_dev(self.bg, T, self.d_frames, self.stride, self.fbytes, T * self.fbytes, lr,
                              self.d_mask if want_mask else 0)
        self.ctx.d2h(masks, self.d_mask)
        self.ctx.sync()
        return masks

    def image(self):
        out = np.full((self.streams, self.h, self.w, self.cn), 0xAA, np.uint8)
        self.ctx.h2d(self.d_image, out)
        self.ctx.bg_image_dev(self.bg, self.d_image)
        self.ctx.d2h(out, self.d_image)
        self.ctx.sync()
        return out

    def state(self, stream=0):
        return canonical(self.ctx.bg_get_state(self.bg, stream, self.h, self.w, self.cn, self.p["nmixtures"]))


def model_for(ctx, name, streams=1, tmax=12):
    c = cases()[name]
    T, h, w, cn = c["frames"].shape
    m = Model(ctx, streams, w, h, cn, c["p"], c["pitch"], tmax)
    if c["state"]:
        for s in range(streams):
            ctx.bg_set_state(m.bg, s, c["state"])
    return m


@pytest.mark.gpu
@needs_gxx
@pytest.mark.parametrize("name", CASE_NAMES)
def test_gpu_equals_oracle_one_launch(ctx, name):
    """All of a case's frames in one launch: masks, the final image, the final state."""
    c, ref = cases()[name], reference(name)
    with model_for(ctx, name) as m:
        if c["state"]:                                   # set_state round-trips
            assert_same(dict(state=m.state()), dict(state=canonical(c["state"])), name + " set/get", ("state",))
        masks = m.apply(c["frames"][None], c["lr"])
        got = dict(masks=masks[0], images=m.image(), state=m.state())
        assert ctx.bg_frames(m.bg) == ref["state"]["nframes"]
    assert_same(got, dict(masks=ref["masks"], images=ref["images"][-1:], state=ref["state"]), name)


@pytest.mark.gpu
@needs_gxx
@pytest.mark.parametrize("name", ["moving_67x35_rgb", "bimodal_64x8_gray_h4", "moving_67x35_gray_lr1_nm3", "darken_64x8_rgb_pitch5"])
def test_gpu_frame_by_frame_and_T_split(ctx, name):
    """Twelve T = 1 calls (mask and image after each), and one launch of 7 then one of 5, against the oracle."""
    c, ref = cases()[name], reference(name)
    fr = c["frames"]
    with model_for(ctx, name) as m:
        for t in range(len(fr)):
            got = dict(masks=m.apply(fr[None, t:t + 1], c["lr"])[0], images=m.image())
            assert_same(got, dict(masks=ref["masks"][t:t + 1], images=ref["images"][t:t + 1]), f"{name} frame {t}",
                        ("masks", "images"))
        assert_same(dict(state=m.state()), ref, name + " T=1", ("state",))
    with model_for(ctx, name) as m:
        masks = np.concatenate([m.apply(fr[None, :7], c["lr"])[0], m.apply(fr[None, 7:], c["lr"])[0]])
        assert_same(dict(masks=masks, images=m.image(), state=m.state()),
                    dict(masks=ref["masks"], images=ref["images"][-1:], state=ref["state"]), name + " T=7+5")


@pytest.mark.gpu
@needs_gxx
def test_gpu_T_above_the_launch_cap(ctx, mdx):
    T, p = 40, params_of(history=8)
    assert T > mdx._lib.BG_MAX_FRAMES_PER_LAUNCH
    frames = seq_moving(31, 16, 16, 3, T=T)
    ref = cpp_run(frames, p)
    with Model(ctx, 1, 16, 16, 3, p, tmax=T) as m:
        got = dict(masks=m.apply(frames[None])[0], images=m.image(), state=m.state())
    assert_same(got, dict(masks=ref["masks"], images=ref["images"][-1:], state=ref["state"]), "T=40")


@pytest.mark.gpu
@needs_gxx
def test_gpu_streams_are_independent(ctx):
    """Three streams in one call equal three single-stream models; the constant middle stream stays one mode."""
    w, h, cn, p = 67, 35, 3, params_of(history=8)
    fr = np.stack([seq_moving(41, w, h, cn, amp=30), np.full((12, h, w, cn), 77, np.uint8), seq_moving(42, w, h, cn, amp=30)])
    refs = [cpp_run(f, p) for f in fr]
    with Model(ctx, 3, w, h, cn, p, pitch=1) as m:
        masks = np.concatenate([m.apply(fr[:, :5]), m.apply(fr[:, 5:])], axis=1)
        images = m.image()
        for s in range(3):
            assert_same(dict(masks=masks[s], images=images[s:s + 1], state=m.state(s)),
                        dict(masks=refs[s]["masks"], images=refs[s]["images"][-1:], state=refs[s]["state"]), f"stream {s}")
        mid = m.state(1)
    assert (mid["modes"] == 1).all() and (mid["weight"][..., 0].view(f32) == 1.0).all()
    assert (masks[1, 1:] == 0).all() and (images[1] == 77).all()


@pytest.mark.gpu
@needs_gxx
def test_gpu_reset_destroy_and_sizes(ctx):
    """Reset then the same frames gives the same outputs; a small model after a large one; destroy, create again."""
    big, small = "moving_67x35_rgb", "moving_1x1_rgb_h4"
    c, ref = cases()[big], reference(big)
    want = dict(masks=ref["masks"], images=ref["images"][-1:], state=ref["state"])
    with model_for(ctx, big) as m:
        for round_ in range(2):
            got = dict(masks=m.apply(c["frames"][None], c["lr"])[0], images=m.image(), state=m.state())
            assert_same(got, want, f"{big} round {round_}")
            ctx.bg_reset(m.bg)
            assert ctx.bg_frames(m.bg) == 0 and (m.state()["modes"] == 0).all()
        cs, rs = cases()[small], reference(small)
        with model_for(ctx, small) as m2:                # both alive on one context
            got = dict(masks=m2.apply(cs["frames"][None], cs["lr"])[0], images=m2.image(), state=m2.state())
            assert_same(got, dict(masks=rs["masks"], images=rs["images"][-1:], state=rs["state"]), small)
    with model_for(ctx, big) as m:                       # destroyed above, created again
        got = dict(masks=m.apply(c["frames"][None], c["lr"])[0], images=m.image(), state=m.state())
        assert_same(got, want, big + " again")


@pytest.mark.gpu
@needs_gxx
def test_gpu_host_conveniences(ctx):
    name = "moving_67x35_gray_pitch3"
    c, ref = cases()[name], reference(name)
    T, h, w, cn = c["frames"].shape
    bg = ctx.bg_create(1, w, h, cn, **c["p"])
    try:
        wide = np.full((h, w + 3), 0xAA, np.uint8)
        for t in range(T):
            wide[:, :w] = c["frames"][t, :, :, 0]
            assert np.array_equal(ctx.bg_apply(bg, wide[:, :w], c["lr"]), ref["masks"][t])     # a pitched view
            assert np.array_equal(ctx.bg_image(bg, h, w, cn), ref["images"][t, :, :, 0])
    finally:
        ctx.bg_destroy(bg)


@pytest.mark.gpu
def test_gpu_einval_leaves_everything_untouched(ctx, mdx):
    L, E = mdx.lib(), mdx._lib.MDX_EINVAL
    w, h, cn = 16, 8, 3
    out = C.c_void_p(0)

    def create(streams=1, w=w, h=h, cn=cn, **kw):
        p = mdx._lib.bg_default_params(**kw)
        return L.mdx_bg_create(ctx._h, streams, w, h, cn, C.byref(p), C.byref(out))
    bad = [dict(streams=0), dict(w=0), dict(h=0), dict(cn=2), dict(cn=4), dict(nmixtures=0), dict(nmixtures=9), dict(history=0),
           dict(var_threshold=-1.0), dict(var_threshold_gen=float("inf")), dict(var_init=float("nan")), dict(ct=-0.1),
           dict(var_min=80.0), dict(background_ratio=0.0), dict(background_ratio=1.5), dict(tau=-0.1), dict(tau=1.5),
           dict(shadow_value=256)]
    for kw in bad:
        assert create(**kw) == E and not out.value, kw
    assert L.mdx_bg_create(ctx._h, 1, w, h, cn, None, None) == E
    frames = seq_moving(51, w, h, cn, T=3)
    with Model(ctx, 2, w, h, cn, params_of(), tmax=3) as m, mdx.Context(0, 64, 64, 1) as other:
        m.apply(np.stack([frames, frames[::-1]]))
        before = [m.state(0), m.state(1)]
        fill = np.full((2, 3, h, w), 0xAA, np.uint8)
        ctx.h2d(m.d_mask, fill)
        ctx.h2d(m.d_image, np.full((2, h, w, cn), 0xAA, np.uint8))
        v, fb = C.c_void_p, m.fbytes
        calls = [
            lambda: L.mdx_bg_apply_dev(ctx._h, None, 1, v(m.d_frames), m.stride, fb, 3 * fb, -1.0, v(m.d_mask)),
            lambda: L.mdx_bg_apply_dev(other._h, v(m.bg), 1, v(m.d_frames), m.stride, fb, 3 * fb, -1.0, v(m.d_mask)),
            lambda: L.mdx_bg_apply_dev(ctx._h, v(m.bg), 0, v(m.d_frames), m.stride, fb, 3 * fb, -1.0, v(m.d_mask)),
            lambda: L.mdx_bg_apply_dev(ctx._h, v(m.bg), 1, None, m.stride, fb, 3 * fb, -1.0, v(m.d_mask)),
            lambda: L.mdx_bg_apply_dev(ctx._h, v(m.bg), 1, v(m.d_frames), w * cn - 1, fb, 3 * fb, -1.0, v(m.d_mask)),
            lambda: L.mdx_bg_apply_dev(ctx._h, v(m.bg), 3, v(m.d_frames), m.stride, fb - 1, 3 * fb, -1.0, v(m.d_mask)),
            lambda: L.mdx_bg_apply_dev(ctx._h, v(m.bg), 3, v(m.d_frames), m.stride, fb, 3 * fb - 1, -1.0, v(m.d_mask)),
            lambda: L.mdx_bg_apply_dev(ctx._h, v(m.bg), 1, v(m.d_frames), m.stride, fb, 0, -1.0, v(m.d_mask)),
            lambda: L.mdx_bg_apply_dev(ctx._h, v(m.bg), 1, v(m.d_frames), m.stride, fb, 3 * fb, float("nan"), v(m.d_mask)),
            lambda: L.mdx_bg_image_dev(ctx._h, None, v(m.d_image)),
            lambda: L.mdx_bg_image_dev(other._h, v(m.bg), v(m.d_image)),
            lambda: L.mdx_bg_image_dev(ctx._h, v(m.bg), None),
            lambda: L.mdx_bg_apply(ctx._h, v(m.bg), frames.ctypes.data_as(v), w * cn, -1.0, None),     # two streams
            lambda: L.mdx_bg_image(ctx._h, v(m.bg), fill.ctypes.data_as(v)),
            lambda: L.mdx_bg_reset(other._h, v(m.bg)),
            lambda: L.mdx_bg_destroy(other._h, v(m.bg)),
            lambda: L.mdx_bg_frames(other._h, v(m.bg)),
            lambda: L.mdx_bg_get_state(ctx._h, v(m.bg), 2, None, None, None, None, None),
            lambda: L.mdx_bg_get_state(ctx._h, v(m.bg), -1, None, None, None, None, None),
        ]
        for i, call in enumerate(calls):
            assert call() == E, i
        st = ctx.bg_get_state(m.bg, 0, h, w, cn, 5)
        too_many = dict(st, modes=np.full((h, w), 6, np.uint8))
        p = lambda a: a.ctypes.data_as(v)
        assert L.mdx_bg_set_state(ctx._h, v(m.bg), 0, p(st["weight"]), p(st["variance"]), p(st["mean"]), p(too_many["modes"]), 3) == E
        assert L.mdx_bg_set_state(ctx._h, v(m.bg), 0, p(st["weight"]), p(st["variance"]), p(st["mean"]), p(st["modes"]), -1) == E
        assert L.mdx_bg_set_state(ctx._h, v(m.bg), 0, None, p(st["variance"]), p(st["mean"]), p(st["modes"]), 3) == E
        assert L.mdx_bg_set_state(ctx._h, v(m.bg), 2, p(st["weight"]), p(st["variance"]), p(st["mean"]), p(st["modes"]), 3) == E
        ctx.sync()
        got_mask, got_img = np.zeros_like(fill), np.zeros((2, h, w, cn), np.uint8)
        ctx.d2h(got_mask, m.d_mask)
        ctx.d2h(got_img, m.d_image)
        ctx.sync()
        assert (got_mask == 0xAA).all() and (got_img == 0xAA).all() and (fill == 0xAA).all()
        assert ctx.bg_frames(m.bg) == 3
        for s in range(2):
            assert_same(dict(state=m.state(s)), dict(state=before[s]), f"stream {s} after the refused calls", ("state",))


def square_stream(w=160, h=120, T=8):
    rng = np.random.default_rng(77)
    base = rng.integers(60, 180, (h, w, 3))
    out = []
    for t in range(T):
        f = base.copy()
        f[30 + 3 * t:58 + 3 * t, 20 + 9 * t:52 + 9 * t] = 255
        f[80:100, 100 + 4 * t:124 + 4 * t] = 10
        out.append(_noisy(rng, f, 2))
    return np.stack(out)


@pytest.mark.gpu
@needs_gxx
def test_gpu_chain_to_external_outlines(ctx, mdx):
    """mdx_bg_apply_dev -> mdx_mask_regions_dev(OPEN3) -> parents -> outlines on the device equals the oracle's mask
    fed to the existing host entry, and BackgroundSubtractor.getMotionContours returns the same outlines."""
    frames = square_stream()
    T, h, w, cn = frames.shape
    ref = cpp_run(frames, params_of())
    bs = mdx.BackgroundSubtractor(context=ctx)
    seen = 0
    try:
        for t in range(T):
            contours, rects = bs.getMotionContours(frames[t])
            want = ctx.mask_regions(ref["masks"][t], open3=True, min_area=1, want_parents=True, want_outlines=True)
            assert len(contours) == len(want.external) == len(want.outlines) == len(rects), t
            for j, o in enumerate(want.outlines):
                assert np.array_equal(contours[j], o), (t, j)
            assert rects == want.external_rectangles, t
            seen += len(contours)
        assert np.array_equal(bs.background(), ref["images"][-1]) and bs.frames() == T
        assert np.array_equal(bs.apply(frames[0]), cpp_run(np.concatenate([frames, frames[:1]]), params_of())["masks"][-1])
    finally:
        bs.close()
    assert seen >= T - 1          # the squares are found from the second frame on


@pytest.mark.gpu
@needs_gxx
def test_gpu_outline_buffer_regrows(ctx, mdx):
    """A first guess of 8 outline points is short on every frame: getMotionContours grows the buffer by what
    num_points reports, outlines again, and returns what the roomy default returns."""
    frames = square_stream(T=3)
    ref = cpp_run(frames, params_of())
    bs = mdx.BackgroundSubtractor(context=ctx, max_points=8)
    try:
        for t in range(len(frames)):
            contours, rects = bs.getMotionContours(frames[t])
            want = ctx.mask_regions(ref["masks"][t], open3=True, min_area=1, want_parents=True, want_outlines=True)
            assert sum(len(o) for o in want.outlines) > 8 and bs._maxp >= sum(len(o) for o in want.outlines)
            assert len(contours) == len(want.outlines) and all(np.array_equal(a, b) for a, b in zip(contours, want.outlines))
            assert rects == want.external_rectangles
    finally:
        bs.close()


@pytest.mark.gpu
@needs_gxx
def test_gpu_context_frees_models_never_destroyed(mdx):
    """mdx_destroy with two live models, one of them mid-stream; a context made afterwards works as usual."""
    name = "bimodal_64x8_gray_h4"
    c, ref = cases()[name], reference(name)
    T, h, w, cn = c["frames"].shape
    other = mdx.Context(0, 64, 64, 1)
    a, b = other.bg_create(2, w, h, cn, **c["p"]), other.bg_create(1, 33, 7, 3)
    assert np.array_equal(other.bg_apply(b, np.full((7, 33, 3), 50, np.uint8)), np.full((7, 33), 127, np.uint8))
    assert other.bg_frames(a) == 0 and other.bg_frames(b) == 1
    other.close()                                        # neither model was destroyed
    with mdx.Context(0, 64, 64, 1) as again, model_for(again, name) as m:
        got = dict(masks=m.apply(c["frames"][None], c["lr"])[0], images=m.image(), state=m.state())
    assert_same(got, dict(masks=ref["masks"], images=ref["images"][-1:], state=ref["state"]), name)
