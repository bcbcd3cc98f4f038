"""Deterministic frames that drive Lucas-Kanade out of its comfortable regime (helper module).

The suite's ordinary inputs (mdx_synth_pair, tests/traj_seq.py) are a textured scene under a small
similarity: every LK point converges, oscillates, runs into the iteration cap or is rejected by
minEig.  The generators here make points *leave the frame* (smooth low-frequency frames with a
brightness offset), never converge (unrelated textures, a texture against its inverse), sit on
saturated gradients (8-px checkerboard) or fail minEig at every level (1-px checkerboard, flat
half, low contrast).  tests/test_lk_exits.py checks with the oracle that they do.

Everything is integer arithmetic or float64 numpy on index grids: no random generator state, the
same frames for any (w, h) on every run.
"""
import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _hash_noise(w, h, seed):
    """(h, w) uint8 white noise: splitmix64 of (seed, y, x)."""
    y, x = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), indexing="ij")
    with np.errstate(over="ignore"):
        z = (np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15) + (y << np.uint64(32)) + x) & _M64
        z = (z + np.uint64(0x9E3779B97F4A7C15)) & _M64
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(56)).astype(np.uint8)


def _box(img, r):
    """Separable (2r+1) box mean, reflected borders, integer arithmetic."""
    a = img.astype(np.int64)
    k = 2 * r + 1
    for axis in (0, 1):
        pad = [(r, r) if ax == axis else (0, 0) for ax in (0, 1)]
        p = np.pad(a, pad, mode="reflect")
        n = a.shape[axis]
        a = sum(np.take(p, np.arange(i, i + n), axis=axis) for i in range(k)) // k
    return a


def texture(w, h, seed):
    """Blurred noise stretched to the full 0..255 range: corners everywhere, like a textured scene."""
    a = _box(_box(_hash_noise(w, h, seed), 2), 1)
    lo, hi = int(a.min()), int(a.max())
    return ((a - lo) * 255 // max(hi - lo, 1)).astype(np.uint8)


def smooth(w, h, phi=0.0, off=0.0):
    """clip(128 + 50 sin(x/23 + phi) + 50 sin(y/19 + 0.7 phi) + off): gradients of about 2 grey
    levels per pixel and no corner, so a brightness offset sends LK's steps tens of pixels long."""
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    v = 128.0 + 50.0 * np.sin(x / 23.0 + phi) + 50.0 * np.sin(y / 19.0 + 0.7 * phi) + off
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def checker(w, h, cell, dx=0, dy=0):
    y, x = np.meshgrid(np.arange(h) + dy, np.arange(w) + dx, indexing="ij")
    return np.where(((x // cell) + (y // cell)) % 2 == 0, 0, 255).astype(np.uint8)


def _pair_smooth(phi, off):
    return lambda w, h: (smooth(w, h, 0.0, 0.0), smooth(w, h, phi, off))


def _pair_noise2(w, h):
    return texture(w, h, 11), texture(w, h, 12)


def _pair_inverse(w, h):
    t = texture(w, h, 13)
    return t, (255 - t).astype(np.uint8)


def _pair_checker8(w, h):
    return checker(w, h, 8), checker(w, h, 8, 5, 3)


def _pair_checker1(w, h):
    return checker(w, h, 1), checker(w, h, 1, 1, 0)


def _pair_halfflat(w, h):
    """A texture shifted by (3, 2) whose right half is one grey level in both frames."""
    big = texture(w + 8, h + 8, 14)
    a, b = big[4:4 + h, 4:4 + w].copy(), big[2:2 + h, 1:1 + w].copy()
    a[:, w // 2:] = 90
    b[:, w // 2:] = 90
    return a, b


def _pair_lowcontrast(w, h):
    """A texture shifted by (2, 1), squeezed into 125..131."""
    big = texture(w + 8, h + 8, 15)
    sq = lambda t: (128 + (t.astype(np.int32) - 128) * 3 // 128).astype(np.uint8)  # noqa: E731
    return sq(big[4:4 + h, 4:4 + w]), sq(big[3:3 + h, 2:2 + w])


# name -> (w, h) -> (frame1, frame2), gray
PAIRS = {
    "bright+30": _pair_smooth(0.0, 30.0),
    "bright-30": _pair_smooth(0.0, -30.0),
    "bright+60": _pair_smooth(0.0, 60.0),
    "bright-40": _pair_smooth(0.0, -40.0),
    "phase1.5": _pair_smooth(1.5, 0.0),
    "noise2": _pair_noise2,
    "inverse": _pair_inverse,
    "checker8": _pair_checker8,
    "checker1": _pair_checker1,
    "halfflat": _pair_halfflat,
    "lowcontrast": _pair_lowcontrast,
}


def to_rgb(gray):
    """(h, w, 3) frame whose channels differ (so rgb and bgr give different greys)."""
    g = gray.astype(np.int32)
    return np.stack([g, np.clip(g + 9, 0, 255), np.clip(g * 7 // 8, 0, 255)], axis=2).astype(np.uint8)


def pair(name, w, h, channels=1):
    a, b = PAIRS[name](w, h)
    if channels == 3:
        a, b = to_rgb(a), to_rgb(b)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def traj_frames(w, h, nimg, channels=1):
    """The smooth pattern drifting and brightening: frame k has off = 12 k, phi = 0.4 k."""
    fr = [smooth(w, h, 0.4 * k, 12.0 * k) for k in range(nimg)]
    return [np.ascontiguousarray(to_rgb(f) if channels == 3 else f) for f in fr]
