"""The 200 x 160 gray scenes of the k_lk_iter tests (helper module; test_lk_fma_gpu.py, test_lk_jbias_gpu.py):
at pixel_step 10 the smallest frame that puts level 1 on k_lk_iter<4, 56> and level 0 on k_lk_iter<8, 112>;
two pyramid levels, 320 grid points."""
import numpy as np

W, H, PS = 200, 160, 10
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


def smooth_base(seed):
    """Blurred noise, 128 +- 30: neighbouring pixels differ by a few grey levels."""
    r = np.random.default_rng(seed).random((H + 17, W + 17))
    b = _blur(r, 2)
    return 128 + 60 * (b - b.min()) / (b.max() - b.min()) - 30


def smooth_pair(seed):
    base = smooth_base(seed)
    return _shifted(base, 0, 0), _shifted(base, 0.4, 0.3)


def board():
    """0/255 blocks of 8 px, 3 px larger than the frame either way."""
    yy, xx = np.mgrid[0:H + 3, 0:W + 3]
    return ((((xx // 8) + (yy // 8)) & 1) * 255).astype(np.uint8)


def edges_pair(axis):
    """The board, the second frame moved by 3 px along `axis`."""
    b = board()
    return np.ascontiguousarray(b[:H, :W]), np.ascontiguousarray(b[3:3 + H, :W] if axis == 0 else b[:H, 3:3 + W])


def mixed_pair(seed):
    """The smooth scene with one 0/255 rectangle (a 255 block inside a 0 frame), moving with it."""
    base = smooth_base(seed)
    base[8 + 60:8 + 100, 8 + 70:8 + 120] = 0
    base[8 + 68:8 + 92, 8 + 78:8 + 112] = 255
    return _shifted(base, 0, 0), _shifted(base, 0.4, 0.3)
