"""Mirror of the reference's BackgroundSubtractor (common/include/motion_detection/background_subtractor.h:14-26,
common/src/background_subtractor.cpp:20-36): a cv::BackgroundSubtractorMOG2 with OpenCV 2.4's default
parameters, whose mask is opened (erode, dilate) and whose external contours are found
(findContours(RETR_EXTERNAL, CHAIN_APPROX_NONE)).

    bs = BackgroundSubtractor()
    contours, rectangles = bs.getMotionContours(frame)      # what the reference computes before it draws
    mask = bs.apply(frame)                                   # operator(): 0 / 127 (shadow) / 255
    background = bs.background()                             # getBackgroundImage

Everything runs on the MI355X through libmdx.so and stays there between the stages: the frame goes up, the
mixture model is updated (mdx_bg_apply_dev), the mask is opened and labelled (mdx_mask_regions_dev with
MDX_REGIONS_OPEN3), the external records are picked (mdx_region_parents_dev) and outlined
(mdx_region_outlines_dev); only the outlines and their records come back.  drawContours (:36) is not built
(DESIGN.md §8): the contours are returned, not painted.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .context import Context, _frame_view


class BackgroundSubtractor:
    def __init__(self, device: int = 0, context: Context | None = None, learning_rate: float = -1.0, min_area: int = 1,
                 max_points: int | None = None, **params):
        """params: mdx_bg_params fields (history, nmixtures, var_threshold, ...; include/mdx.h).  learning_rate < 0
        is the automatic rate the reference uses.  context: an existing Context to run on (not closed by this
        object); else one is created on `device` at the first frame.  min_area: regions below it are dropped
        (1 keeps every contour, as the reference does).  max_points: the first guess of a frame's outline points
        (default max(4096, w * h / 4)); a frame that needs more grows the buffer and outlines again."""
        self._device = device
        self._ctx = context
        self._own = context is None
        self._params = dict(params)
        self.learning_rate = float(learning_rate)
        self.min_area = int(min_area)
        self._guess = max_points
        self._bg = 0
        self._shape = None
        self._dev = {}

    # -- lifetime
    def close(self):
        if self._ctx is not None and getattr(self._ctx, "_h", None):
            self._release()
            if self._own:
                self._ctx.close()
        self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _release(self):
        self._ctx.sync()
        for p in self._dev.values():
            self._ctx.dev_free(p)
        self._dev = {}
        if self._bg:
            self._ctx.bg_destroy(self._bg)
            self._bg = 0

    def _prepare(self, frame) -> np.ndarray:
        frame = _frame_view(frame)
        if frame.ndim not in (2, 3) or (frame.ndim == 3 and frame.shape[2] not in (1, 3)):
            raise ValueError("frame must be (h, w) or (h, w, 3) uint8")
        h, w = frame.shape[:2]
        cn = 1 if frame.ndim == 2 else frame.shape[2]
        if self._ctx is None:
            self._ctx = Context(self._device, max(w, 64), max(h, 64), 1)
        if self._shape != (h, w, cn):       # a new frame size starts a new model, as MOG2's initialize does
            self._release()
            ctx, n, cap = self._ctx, w * h, ((w + 1) // 2) * ((h + 1) // 2)
            self._bg = ctx.bg_create(1, w, h, cn, **self._params)
            self._shape, self._cap, self._maxp = (h, w, cn), cap, max(4096, n // 4) if self._guess is None else max(1, int(self._guess))
            self._dev = {"frame": ctx.dev_alloc(frame.strides[0] * h), "mask": ctx.dev_alloc(n), "image": ctx.dev_alloc(n * cn),
                         "labels": ctx.dev_alloc(4 * n), "regions": ctx.dev_alloc(32 * cap), "external": ctx.dev_alloc(32 * cap),
                         "counts": ctx.dev_alloc(16), "offsets": ctx.dev_alloc(4 * (cap + 1)), "xy": ctx.dev_alloc(8 * self._maxp)}
            self._pitch = frame.strides[0]
        if frame.strides[0] != self._pitch:
            frame = np.ascontiguousarray(frame)
            if frame.strides[0] != self._pitch:
                self._ctx.sync()
                self._ctx.dev_free(self._dev["frame"])
                self._dev["frame"], self._pitch = self._ctx.dev_alloc(frame.strides[0] * h), frame.strides[0]
        return frame

    def _apply_dev(self, frame: np.ndarray):
        h, w, cn = self._shape
        nbytes = self._pitch * (h - 1) + w * cn
        flat = np.lib.stride_tricks.as_strided(frame, shape=(nbytes,), strides=(1,)) if frame.size else frame
        self._ctx.h2d(self._dev["frame"], flat)
        self._ctx.bg_apply_dev(self._bg, 1, self._dev["frame"], self._pitch, self._pitch * h, 0, self.learning_rate,
                               self._dev["mask"])

    # -- the reference's interface
    def apply(self, frame, want_mask: bool = True):
        """cv::BackgroundSubtractorMOG2::operator(): update the model with `frame`, return the (h, w) mask
        (want_mask False: nothing comes back, and the call does not wait for the device)."""
        frame = self._prepare(frame)
        self._apply_dev(frame)
        if not want_mask:
            return None
        h, w, _ = self._shape
        mask = np.empty((h, w), np.uint8)
        self._ctx.d2h(mask, self._dev["mask"])
        self._ctx.sync()
        return mask

    def background(self) -> np.ndarray:
        """getBackgroundImage: (h, w) or (h, w, 3) uint8."""
        if not self._bg:
            raise _lib.MdxError("no frame seen yet")
        h, w, cn = self._shape
        out = np.empty((h, w) if cn == 1 else (h, w, cn), np.uint8)
        self._ctx.bg_image_dev(self._bg, self._dev["image"])
        self._ctx.d2h(out, self._dev["image"])
        self._ctx.sync()
        return out

    def frames(self) -> int:
        return self._ctx.bg_frames(self._bg) if self._bg else 0

    def getMotionContours(self, frame):
        """Update the model with `frame`; return (contours, rectangles): one (n_j, 2) int32 array of x, y per
        external region of the opened mask, in findContours' point order, and each one's (x, y, width, height)."""
        frame = self._prepare(frame)
        self._apply_dev(frame)
        ctx, d = self._ctx, self._dev
        h, w, _ = self._shape
        cap = self._cap
        cnt = d["counts"]            # num_all, num_kept, num_external, num_points
        ctx.mask_regions_dev(1, d["mask"], w, h, w, w * h, True, self.min_area, d["regions"], cap, cnt, cnt + 4, d["labels"])
        ctx.region_parents_dev(1, d["labels"], w, h, d["regions"], cap, cnt + 4, 0, d["external"], cnt + 8)
        counts = np.zeros(4, np.int32)
        while True:
            ctx.region_outlines_dev(1, d["labels"], w, h, d["external"], cap, cnt + 8, d["offsets"], d["xy"], self._maxp,
                                    cnt + 12)
            ctx.d2h(counts, cnt)
            ctx.sync()
            if counts[3] <= self._maxp:
                break
            ctx.dev_free(d["xy"])           # the guess was short: num_points says by how much
            self._maxp = int(counts[3])
            d["xy"] = ctx.dev_alloc(8 * self._maxp)
        next_ = min(int(counts[2]), cap)
        offsets = np.zeros(next_ + 1, np.int32)
        ctx.d2h(offsets, d["offsets"])
        regs = np.zeros((next_, 8), np.int32)
        xy = np.zeros((int(counts[3]), 2), np.int32)
        if next_:
            ctx.d2h(regs, d["external"])
        if len(xy):
            ctx.d2h(xy, d["xy"])
        ctx.sync()
        contours = [xy[offsets[j]:offsets[j + 1]].copy() for j in range(next_)]
        return contours, [tuple(int(v) for v in r[:4]) for r in regs]
