"""Python host over the C-ABI: a device context per camera stream / GPU.

Thin ownership wrapper around ``mdx_ctx`` (include/mdx.h).  Numpy arrays on the host
side, raw device pointers (ints) for the zero-copy batched entry; no torch types.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import MdxError, lib


def _ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _v(p: int):
    """A device pointer given as an int (0: none) for a C-ABI argument."""
    return C.c_void_p(p) if p else None


def _cluster_buffers(n: int, min_size: int, max_kept: int | None = None):
    """Outputs of a clustering entry for n members: cap (max_kept, default every cluster that can be
    kept: one has more than min_size members), labels, kept ids and rectangles."""
    cap = n // (max(int(min_size), 0) + 1) if max_kept is None else int(max_kept)
    return cap, np.zeros(n, np.int32), np.zeros(max(cap, 0), np.int32), np.zeros((max(cap, 0), 4), np.int32)


def _trim_kept(nkept: int, cap: int, kept: np.ndarray, rects: np.ndarray):
    m = min(nkept, cap)
    return kept[:m].copy(), rects[:m].copy()


def _frame_view(img) -> np.ndarray:
    """A uint8 frame as the C-ABI reads it.  A row-pitched view (pixels and channels adjacent, a
    positive row stride of at least one row's bytes, e.g. a crop of a larger image) is kept as it is
    and goes down with its pitch; anything else is copied to a packed array."""
    a = np.asarray(img)
    if a.dtype != np.uint8:
        a = a.astype(np.uint8)
    if a.ndim not in (2, 3) or a.shape[0] == 0 or a.shape[1] == 0:
        return np.ascontiguousarray(a)
    ch = 1 if a.ndim == 2 else a.shape[2]
    inner = a.strides[1] == ch and (a.ndim == 2 or a.strides[2] == 1)
    if inner and a.strides[0] >= a.shape[1] * ch:
        return a
    return np.ascontiguousarray(a)


def _frame_views(images) -> list:
    """_frame_view of each frame; frames of different pitches are all packed (the entries take one)."""
    views = [_frame_view(im) for im in images]
    if any(v.strides[0] != views[0].strides[0] for v in views if v.shape == views[0].shape):
        views = [np.ascontiguousarray(v) for v in views]
    return views


def grid_count(w: int, h: int, pixel_step: int) -> int:
    return lib().mdx_grid_count(w, h, pixel_step)


def half_size(w: int, h: int) -> tuple:
    """(dw, dh) of the reference's cv::resize(src, dst, Size(), 0.5, 0.5) (include/mdx.h mdx_half_size):
    cvRound(side * 0.5), half to even.  ValueError when a side is below 1 or rounds to 0."""
    dw, dh = C.c_int(0), C.c_int(0)
    if lib().mdx_half_size(int(w), int(h), C.byref(dw), C.byref(dh)) != _lib.MDX_OK:
        raise ValueError(f"a {w} x {h} frame has no half size")
    return dw.value, dh.value


def grid_points(w: int, h: int, pixel_step: int) -> np.ndarray:
    """Grid of the reference (optical_flow_calculator.cpp:56-64): x-major, float32 (n, 2)."""
    xs = np.arange(0, w, pixel_step, dtype=np.float32)
    ys = np.arange(0, h, pixel_step, dtype=np.float32)
    gx, gy = np.meshgrid(xs, ys, indexing="ij")
    return np.stack([gx.ravel(), gy.ravel()], 1)


@dataclass
class FlowResult:
    num_vectors: int        # reference return value
    next_pts: np.ndarray    # (npts, 2) float32, LK output positions, x-major grid order
    status: np.ndarray      # (npts,) uint8
    vectors: np.ndarray     # (npts, 4) float64: (x, y, dx, dy) / (x, y, 0, 0) / (-1, -1, 0, 0)
    mask: np.ndarray | None  # (h, w) uint8 or None
    H: np.ndarray           # (3, 3) float64 (zeros when no fit)
    code: int               # MDX_OK or MDX_EDEGENERATE
    regions: "RegionResult | None" = None   # the mask labelled into regions (the node's region_min_area)
    # the node's detect_outliers (findOutliers -> getOutlierVectors -> getClusters on `vectors`' image):
    outlier_flags: np.ndarray | None = None  # (npts,) uint8 per grid vector, image rows outer (mdx_find_outliers)
    vector_clusters: list = field(default_factory=list)   # getClusters' kept clusters, (n_k, 4) float64 each
    clusters: list = field(default_factory=list)          # their points, (n_k, 2) float32 each
    rectangles: list = field(default_factory=list)        # their (x, y, width, height), as cv::Rect
    contours: list = field(default_factory=list)          # their convex hulls, (v_k, 2) int32 each (cluster_contours)


@dataclass
class TrajectoryResult:
    num_vectors: int        # reference return value (last pass)
    traj: np.ndarray        # (npts, nimg, 2) float32: grid point, then each accepted move
    traj_len: np.ndarray    # (npts,) int32: entries of traj in use (complete iff == nimg)
    start_pts: np.ndarray   # (npts, 2) float32: points entering the last pass
    vectors: np.ndarray     # (npts, 4) float64: the last pass's Vec4d per point

    @property
    def trajectories(self) -> list:
        """The reference's output list (optical_flow_calculator.cpp:244-249): the complete ones,
        in grid order, each (nimg, 2)."""
        nimg = self.traj.shape[1]
        return [self.traj[i] for i in np.nonzero(self.traj_len == nimg)[0]]


@dataclass
class SubspaceResult:
    columns: np.ndarray         # (4*num_motions,) int32: the winning sample (-1: no hypothesis had an inlier)
    is_outlier: np.ndarray      # (ntraj,) uint8
    residuals: np.ndarray       # (ntraj,) float64, the winner's
    outlier_points: np.ndarray  # (n_outliers, 2) float32: each outlier's second-to-last point


@dataclass
class ClusterResult:
    labels: np.ndarray          # (npoints,) int32: the point's cluster among all clusters, creation order
    num_all: int                # number of all clusters
    kept: np.ndarray            # (num_kept,) int32: ids of the clusters with size > min_size, ascending
    rects: np.ndarray           # (num_kept, 4) int32: x, y, width, height of each kept cluster (cv::Rect)
    num_kept: int = 0           # all kept clusters, also when max_kept cut kept / rects short


@dataclass
class VectorClusterResult:
    """Flow vectors clustered by distance and angle (include/mdx.h mdx_cluster_vectors)."""
    labels: np.ndarray          # (n,) int32: the vector's cluster among all clusters, creation order; -1 inactive
    num_active: int             # vectors with a non-zero flow
    num_all: int                # number of all clusters
    kept: np.ndarray            # (num_kept,) int32: ids of the clusters with size > min_size, ascending
    rects: np.ndarray           # (num_kept, 4) int32: x, y, width, height of each kept cluster (cv::Rect)
    num_kept: int = 0           # all kept clusters, also when max_kept cut kept / rects short


@dataclass
class OutlierResult:
    """Flow-vector outliers by median / MAD (include/mdx.h mdx_find_outliers).  Shapes are
    those of the input: (n, ...) for one field, (batch, n, ...) for a batch."""
    flags: np.ndarray            # (..., n) uint8: bit 0 flagged by the angle, bit 1 by the magnitude
    outlier_vectors: np.ndarray  # (..., n, 4) float64: getOutlierVectors, non-outliers zeroed
    stats: np.ndarray            # (batch,) records of _lib.MdxOutlierStats' fields (one record for one field)

    @property
    def is_outlier(self) -> np.ndarray:
        return self.flags != 0


@dataclass
class RegionResult:
    """The motion mask labelled into regions (include/mdx.h mdx_mask_regions)."""
    regions: np.ndarray         # (min(num_kept, max_regions), 8) int32: x, y, width, height, area, seed_x, seed_y, id
    num_all: int                # every 8-connected component of the (opened) mask
    num_kept: int               # those with area >= min_area, also when max_regions cut `regions` short
    labels: np.ndarray | None = None    # (h, w) int32: id among all components, -1 background (want_labels)
    mask_out: np.ndarray | None = None  # (h, w) uint8: the opened mask as 0 / 255 (want_mask)
    outlines: list | None = None        # one (n_j, 2) int32 array per returned record: its outer border (want_outlines, §7m)
    hulls: list | None = None           # one (v_j, 2) int32 array per returned record: its convex hull (want_hulls, §7k)

    @property
    def rectangles(self) -> list:
        """(x, y, width, height) of each kept region, as cv::Rect."""
        return [tuple(int(v) for v in r[:4]) for r in self.regions]


@dataclass
class RegionTreeResult(RegionResult):
    """RegionResult with each record's parent blob (include/mdx.h mdx_mask_regions_tree).
    `regions` holds every kept record, nested or not; `hulls` (want_hulls) and `outlines` (want_outlines) hold
    those of the external records only, hulls[i] and outlines[i] belonging to regions[external[i]]."""
    parent: np.ndarray | None = None    # (len(regions),) int32: a component id, -1 external, -2 unknown
    external: np.ndarray | None = None  # (num_external,) int32: positions in `regions` of the external records

    @property
    def external_rectangles(self) -> list:
        """(x, y, width, height) of each external region: what findContours' RETR_EXTERNAL keeps."""
        return [tuple(int(v) for v in self.regions[i, :4]) for i in self.external]


class Context:
    """One device context (mdx_ctx): workspace sized at creation, one HIP stream."""

    def __init__(self, device: int = 0, max_w: int = 1920, max_h: int = 1080, max_batch: int = 1, **params):
        self._p = _lib.default_params(**params)
        h = lib().mdx_create(device, max_w, max_h, max_batch, C.byref(self._p))
        if not h:
            raise MdxError("mdx_create failed: " + lib().mdx_create_error().decode())
        self._h = C.c_void_p(h)
        self._ring_hold = []    # frames whose asynchronous ring push may still be reading them

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None):
            lib().mdx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device(self) -> int:
        return lib().mdx_device(self._h)

    def device_pci(self) -> str:
        """PCI bus id of the context's device (distinct per physical GPU)."""
        buf = C.create_string_buffer(64)
        self._check(lib().mdx_device_pci(self._h, buf, 64))
        return buf.value.decode()

    def _check(self, rc: int) -> int:
        if rc < 0:
            raise MdxError(f"mdx error {rc}: {lib().mdx_last_error(self._h).decode()}")
        return rc

    # -- params
    @property
    def params(self) -> _lib.MdxParams:
        p = _lib.MdxParams()
        self._check(lib().mdx_get_params(self._h, C.byref(p)))
        return p

    def set_params(self, **kw):
        p = self.params
        for k, v in kw.items():
            setattr(p, k, v)
        self._check(lib().mdx_set_params(self._h, C.byref(p)))

    # -- host entry (drop-in for calculateOpticalFlow)
    def flow_warp_diff(self, img1: np.ndarray, img2: np.ndarray, fmt: int | None = None, want_mask: bool = True,
                       H_external: np.ndarray | None = None) -> FlowResult:
        img1, img2 = _frame_views([img1, img2])
        if img1.shape != img2.shape:
            raise ValueError("frames must have the same shape")
        h, w = img1.shape[:2]
        if fmt is None:
            fmt = _lib.FMT_GRAY8 if img1.ndim == 2 else _lib.FMT_RGB8
        p = self.params
        n = grid_count(w, h, p.pixel_step)
        nextp = np.zeros((n, 2), np.float32)
        status = np.zeros(n, np.uint8)
        vec = np.zeros((n, 4), np.float64)
        mask = np.zeros((h, w), np.uint8) if want_mask else None
        H = np.zeros(9, np.float64)
        Hx = None if H_external is None else np.ascontiguousarray(H_external, dtype=np.float64).ravel()
        num = C.c_int(0)
        rc = self._check(lib().mdx_flow_warp_diff(self._h, _ptr(img1), _ptr(img2), w, h, img1.strides[0], fmt,
                                                  _ptr(nextp), _ptr(status), _ptr(vec), _ptr(mask), _ptr(H), _ptr(Hx),
                                                  C.byref(num)))
        return FlowResult(num.value, nextp, status, vec, mask, H.reshape(3, 3), rc)

    # -- trajectory tracking (drop-in for calculateOpticalFlowTrajectory)
    def flow_trajectory(self, images, fmt: int | None = None) -> "TrajectoryResult":
        imgs = _frame_views(images)
        if len(imgs) < 2 or any(im.shape != imgs[0].shape for im in imgs):
            raise ValueError("need >= 2 frames of one shape")
        h, w = imgs[0].shape[:2]
        if fmt is None:
            fmt = _lib.FMT_GRAY8 if imgs[0].ndim == 2 else _lib.FMT_RGB8
        nimg = len(imgs)
        n = grid_count(w, h, self.params.pixel_step)
        traj = np.zeros((n, nimg, 2), np.float32)
        tlen = np.zeros(n, np.int32)
        start = np.zeros((n, 2), np.float32)
        vec = np.zeros((n, 4), np.float64)
        arr = (C.c_void_p * nimg)(*[im.ctypes.data for im in imgs])
        num = C.c_int(0)
        self._check(lib().mdx_flow_trajectory(self._h, arr, nimg, w, h, imgs[0].strides[0], fmt, _ptr(traj),
                                              _ptr(tlen), _ptr(start), _ptr(vec), C.byref(num)))
        return TrajectoryResult(num.value, traj, tlen, start, vec)

    # -- resident frame ring (the node's raw_images_ deque kept in HBM: mdx_ring_*)
    def ring_push(self, image: np.ndarray, keep: int, fmt: int | None = None, half: bool = False) -> int:
        """Append one frame (pyramided once, on the device) and keep at most `keep` frames.
        Returns the number of frames held.  half: the frame is halved on the device on its way in
        (mdx_ring_push_half); the ring then holds half_size(w, h) frames."""
        im = _frame_view(image)
        h, w = im.shape[:2]
        if fmt is None:
            fmt = _lib.FMT_GRAY8 if im.ndim == 2 else _lib.FMT_RGB8
        push = lib().mdx_ring_push_half if half else lib().mdx_ring_push
        n = self._check(push(self._h, _ptr(im), w, h, im.strides[0], fmt, int(keep)))
        # the upload is queued, not done (include/mdx.h): hold the frame until the next
        # ring_trajectory / sync returns
        self._ring_hold.append(im)
        return n

    def ring_trajectory(self, w: int, h: int, nimg: int, out: "TrajectoryResult | None" = None) -> "TrajectoryResult":
        """calculateOpticalFlowTrajectory over the ring's `nimg` frames (w x h).  `out`: arrays to
        fill (e.g. from trajectory_buffers(pinned=True)), reused across callbacks."""
        n = grid_count(w, h, self.params.pixel_step)
        if out is None:
            out = self.trajectory_buffers(w, h, nimg)
        traj, tlen, start, vec = out.traj, out.traj_len, out.start_pts, out.vectors
        num = C.c_int(0)
        assert traj.shape == (n, nimg, 2) and tlen.shape == (n,) and start.shape == (n, 2) and vec.shape == (n, 4)
        rc = lib().mdx_ring_trajectory(self._h, _ptr(traj), _ptr(tlen), _ptr(start), _ptr(vec), C.byref(num))
        if rc < 0:
            # the uploads queued by earlier ring_push calls may still read the held frames: release
            # them only once the stream has drained
            lib().mdx_sync(self._h)
        self._ring_hold.clear()
        self._check(rc)
        out.num_vectors = num.value
        return out

    def trajectory_buffers(self, w: int, h: int, nimg: int, pinned: bool = False) -> "TrajectoryResult":
        """Output arrays of a trajectory call; pinned=True puts them in one page-locked block laid
        out as mdx_trajectory_layout says, so the call reads them back with one copy."""
        n = grid_count(w, h, self.params.pixel_step)
        if not pinned:
            return TrajectoryResult(0, np.zeros((n, nimg, 2), np.float32), np.zeros((n,), np.int32),
                                    np.zeros((n, 2), np.float32), np.zeros((n, 4), np.float64))
        if not hasattr(lib(), "mdx_trajectory_layout"):
            return TrajectoryResult(0, host_empty((n, nimg, 2), np.float32), host_empty((n,), np.int32),
                                    host_empty((n, 2), np.float32), host_empty((n, 4), np.float64))
        off = (C.c_size_t * 4)()
        total = int(lib().mdx_trajectory_layout(n, nimg, off))
        blk = host_empty((total,), np.uint8)

        def part(o, shape, dt):
            cnt = int(np.prod(shape))
            return blk[o:o + cnt * np.dtype(dt).itemsize].view(dt).reshape(shape)
        return TrajectoryResult(0, part(off[0], (n, nimg, 2), np.float32), part(off[3], (n,), np.int32),
                                part(off[1], (n, 2), np.float32), part(off[2], (n, 4), np.float64))

    def ring_reset(self) -> None:
        self._check(lib().mdx_ring_reset(self._h))

    # -- trajectory subspace RANSAC (drop-in for OutlierDetector::fitSubspace)
    def fit_subspace(self, traj: np.ndarray, num_motions: int, sigma: float, rng: "_lib.MdxRandState") -> "SubspaceResult":
        traj = np.ascontiguousarray(traj, dtype=np.float32)
        if traj.ndim != 3 or traj.shape[2] != 2:
            raise ValueError("traj must be (ntraj, traj_len, 2)")
        N, T = traj.shape[:2]
        d = 4 * num_motions
        cols = np.full(d, -1, np.int32)
        out = np.zeros(N, np.uint8)
        res = np.zeros(N, np.float64)
        pts = np.zeros((N, 2), np.float32)
        nout = C.c_int(0)
        self._check(lib().mdx_fit_subspace(self._h, _ptr(traj), N, T, int(num_motions), float(sigma), C.byref(rng),
                                           _ptr(cols), _ptr(out), _ptr(res), _ptr(pts), C.byref(nout)))
        return SubspaceResult(cols, out, res, pts[:nout.value].copy())

    # -- greedy Euclidean clustering (drop-in for FlowClusterer::clusterEuclidean + boundingRect)
    def cluster_euclidean(self, points: np.ndarray, distance_threshold: float, min_size: int = 5,
                          max_kept: int | None = None) -> "ClusterResult":
        """max_kept (default: every kept cluster) caps how many kept ids / rectangles are returned."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
        n = pts.shape[0]
        cap, labels, kept, rects = _cluster_buffers(n, min_size, max_kept)
        nall, nkept = C.c_int(0), C.c_int(0)
        self._check(lib().mdx_cluster_euclidean(self._h, _ptr(pts), n, float(distance_threshold), int(min_size),
                                                _ptr(labels), C.byref(nall), _ptr(kept), _ptr(rects), cap,
                                                C.byref(nkept)))
        return ClusterResult(labels, nall.value, *_trim_kept(nkept.value, cap, kept, rects), nkept.value)

    # -- first-fit clustering by distance and angle (drop-in for FlowClusterer::getClusters + boundingRect)
    def cluster_vectors(self, vectors: np.ndarray, distance_threshold: float, angular_threshold: float,
                        min_size: int = 5, abs_int: bool = False) -> "VectorClusterResult":
        """vectors: (n, 4) float64 (x, y, dx, dy) in the reference's visiting order (image rows outer).
        abs_int: MDX_VCLUSTER_ABS_INT, the angular distance truncated as the reference's int abs does."""
        vec = np.ascontiguousarray(vectors, dtype=np.float64).reshape(-1, 4)
        n = vec.shape[0]
        cap, labels, kept, rects = _cluster_buffers(n, min_size)
        nact, nall, nkept = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(lib().mdx_cluster_vectors(self._h, _ptr(vec), n, float(distance_threshold), float(angular_threshold),
                                              int(min_size), _lib.VCLUSTER_ABS_INT if abs_int else 0, _ptr(labels),
                                              C.byref(nact), C.byref(nall), _ptr(kept), _ptr(rects), cap,
                                              C.byref(nkept)))
        return VectorClusterResult(labels, nact.value, nall.value, *_trim_kept(nkept.value, cap, kept, rects), nkept.value)

    # -- convex hulls of clusters (drop-in for showClusterContours' cv::convexHull of every kept cluster)
    def cluster_hulls(self, points: np.ndarray, labels: np.ndarray, ids) -> list:
        """points (n, 2) float32 and labels (n,): the members and each one's cluster, as cluster_euclidean
        returns `labels` (for cluster_vectors' clusters: every vector's (x, y) and its `labels`); ids: the
        clusters wanted, strictly ascending (`kept`, or a subset).  Returns one (v_k, 2) int32 array per
        id: the hull's vertices in cv::convexHull(.., clockwise=false)'s order (include/mdx.h)."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
        lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        want = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        n, k = pts.shape[0], want.shape[0]
        if lab.shape[0] != n:
            raise ValueError("labels must hold one entry per point")
        offsets = np.zeros(k + 1, np.int32)
        xy = np.zeros((n, 2), np.int32)               # a hull has at most as many vertices as members
        total = C.c_int(0)
        self._check(lib().mdx_cluster_hulls(self._h, _ptr(pts), _ptr(lab), n, _ptr(want), k, _ptr(offsets),
                                            _ptr(xy) if n else None, n, C.byref(total)))
        return [xy[offsets[j]:offsets[j + 1]].copy() for j in range(k)]

    # -- median / MAD outliers of the flow vectors (drop-in for OutlierDetector::findOutliers + getOutlierVectors)
    def find_outliers(self, vectors: np.ndarray, include_zeros: bool = False) -> "OutlierResult":
        """vectors: (n, 4) or (batch, n, 4) float64 (x, y, dx, dy); a batch is one launch."""
        vec = np.ascontiguousarray(vectors, dtype=np.float64)
        if vec.ndim not in (2, 3) or vec.shape[-1] != 4:
            raise ValueError("vectors must be (n, 4) or (batch, n, 4)")
        batch, n = (1, vec.shape[0]) if vec.ndim == 2 else vec.shape[:2]
        flags = np.zeros(vec.shape[:-1], np.uint8)
        out = np.zeros(vec.shape, np.float64)
        stats = np.zeros(batch, np.dtype(_lib.MdxOutlierStats))
        self._check(lib().mdx_find_outliers(self._h, _ptr(vec), batch, n,
                                            _lib.OUTLIERS_INCLUDE_ZEROS if include_zeros else 0, _ptr(flags),
                                            _ptr(out), _ptr(stats)))
        return OutlierResult(flags, out, stats)

    # -- the motion mask labelled into regions (getMotionContours' recipe: opening, 8-connected blobs, boundingRect)
    def mask_regions(self, mask: np.ndarray, open3: bool = True, min_area: int = 1, max_regions: int | None = None,
                     want_labels: bool = False, want_mask: bool = False, want_hulls: bool = False,
                     want_parents: bool = False, want_outlines: bool = False) -> "RegionResult":
        """max_regions (default: every component the frame can hold) caps how many records are returned.
        want_hulls: the records and each one's convex hull in one call (mdx_mask_region_hulls: the label
        image stays on the device); labels or the mask asked for next to the hulls cost a second call.
        want_parents: a RegionTreeResult -- every record's parent blob and the external records
        (mdx_mask_regions_tree); with want_hulls the hulls are those of the external records.
        want_outlines: each record's outer border polyline, findContours' point list (mdx_mask_region_outlines:
        the label image stays on the device); with want_parents those of the external records.  It is a call
        of its own next to any of the others, and a second one when the points outgrow the first guess."""
        mask = np.asarray(mask, dtype=np.uint8)
        if mask.ndim != 2 or mask.strides[1] != 1 or mask.strides[0] < mask.shape[1]:
            mask = np.ascontiguousarray(mask)
        if mask.ndim != 2:
            raise ValueError("mask must be (h, w)")
        h, w = mask.shape
        cap = ((w + 1) // 2) * ((h + 1) // 2) if max_regions is None else int(max_regions)
        if max_regions is None and min_area > 1:
            cap = min(cap, (w * h) // int(min_area))      # a kept component has at least min_area pixels
        regs = np.zeros((max(cap, 0), 8), np.int32)
        labels = np.empty((h, w), np.int32) if want_labels else None
        mout = np.empty((h, w), np.uint8) if want_mask else None
        nall, nkept = C.c_int(0), C.c_int(0)
        flags = _lib.REGIONS_OPEN3 if open3 else 0
        outlines = None
        if want_outlines:
            maxp = max(4096, (w * h) // 4)                    # a guess: num_points tells when it was short
            ooff = np.zeros(max(cap, 0) + 1, np.int32)
            opar, oext, onext, npts = np.zeros(max(cap, 0), np.int32), np.zeros(max(cap, 0), np.int32), C.c_int(0), C.c_int(0)
            while True:
                oxy = np.empty((maxp, 2), np.int32)
                self._check(lib().mdx_mask_region_outlines(
                    self._h, _ptr(mask), w, h, mask.strides[0], flags, int(min_area), _ptr(regs) if cap > 0 else None, cap,
                    C.byref(nall), C.byref(nkept), _ptr(opar) if want_parents else None,
                    _ptr(oext) if want_parents else None, C.byref(onext) if want_parents else None, _ptr(ooff), _ptr(oxy),
                    maxp, C.byref(npts)))
                if npts.value <= maxp:
                    break
                maxp = npts.value
            nout = onext.value if want_parents else min(nkept.value, max(cap, 0))
            outlines = [oxy[ooff[j]:ooff[j + 1]].copy() for j in range(nout)]
        if not (want_hulls or want_parents or want_outlines) or want_labels or want_mask:
            self._check(lib().mdx_mask_regions(self._h, _ptr(mask), w, h, mask.strides[0], flags, int(min_area),
                                               _ptr(regs) if cap > 0 else None, cap, C.byref(nall), C.byref(nkept),
                                               _ptr(labels), _ptr(mout)))
        hulls = None
        if want_hulls:
            maxv = min(w * h, 2 * min(w, h) * max(cap, 0))    # what the hulls of `cap` regions can hold (include/mdx.h)
            offsets = np.zeros(max(cap, 0) + 1, np.int32)
            xy = np.empty((maxv, 2), np.int32)
            nv = C.c_int(0)
        if want_parents:
            parent = np.zeros(max(cap, 0), np.int32)
            ext = np.zeros(max(cap, 0), np.int32)
            next_ = C.c_int(0)
            self._check(lib().mdx_mask_regions_tree(
                self._h, _ptr(mask), w, h, mask.strides[0], flags, int(min_area), _ptr(regs) if cap > 0 else None, cap,
                C.byref(nall), C.byref(nkept), _ptr(parent), _ptr(ext), C.byref(next_),
                _ptr(offsets) if want_hulls else None, _ptr(xy) if want_hulls and maxv > 0 else None,
                maxv if want_hulls else 0, C.byref(nv) if want_hulls else None))
            n = min(nkept.value, max(cap, 0))
            if want_hulls:
                hulls = [xy[offsets[j]:offsets[j + 1]].copy() for j in range(next_.value)]
            return RegionTreeResult(regs[:n].copy(), nall.value, nkept.value, labels, mout, outlines, hulls,
                                    parent[:n].copy(), ext[:next_.value].copy())
        if want_hulls:
            self._check(lib().mdx_mask_region_hulls(self._h, _ptr(mask), w, h, mask.strides[0], flags, int(min_area),
                                                    _ptr(regs) if cap > 0 else None, cap, C.byref(nall), C.byref(nkept),
                                                    _ptr(offsets), _ptr(xy) if maxv > 0 else None, maxv, C.byref(nv)))
            hulls = [xy[offsets[j]:offsets[j + 1]].copy() for j in range(min(nkept.value, max(cap, 0)))]
        return RegionResult(regs[:min(nkept.value, max(cap, 0))].copy(), nall.value, nkept.value, labels, mout,
                            outlines, hulls)

    def region_outlines_dev(self, batch: int, d_labels: int, w: int, h: int, d_regions: int, max_regions: int,
                            d_num_kept: int, d_offsets: int, d_xy: int = 0, max_points: int = 0,
                            d_num_points: int = 0) -> int:
        """Asynchronous on the context stream (include/mdx.h mdx_region_outlines_dev); pointers are ints.
        Takes what mask_regions_dev wrote: d_labels, d_regions, d_num_kept -- or region_parents_dev's
        d_external / d_num_external for the outlines of the external records only."""
        return self._check(lib().mdx_region_outlines_dev(
            self._h, batch, _v(d_labels), w, h, _v(d_regions), max_regions, _v(d_num_kept), _v(d_offsets), _v(d_xy),
            max_points, _v(d_num_points)))

    def region_hulls_dev(self, batch: int, d_labels: int, w: int, h: int, d_regions: int, max_regions: int,
                         d_num_kept: int, d_offsets: int, d_xy: int = 0, max_vertices: int = 0,
                         d_num_vertices: int = 0) -> int:
        """Asynchronous on the context stream (include/mdx.h mdx_region_hulls_dev); pointers are ints.
        Takes what mask_regions_dev wrote: d_labels, d_regions, d_num_kept."""
        return self._check(lib().mdx_region_hulls_dev(
            self._h, batch, _v(d_labels), w, h, _v(d_regions), max_regions, _v(d_num_kept), _v(d_offsets), _v(d_xy),
            max_vertices, _v(d_num_vertices)))

    def region_parents_dev(self, batch: int, d_labels: int, w: int, h: int, d_regions: int, max_regions: int,
                           d_num_kept: int, d_parent: int = 0, d_external: int = 0, d_num_external: int = 0) -> int:
        """Asynchronous on the context stream (include/mdx.h mdx_region_parents_dev); pointers are ints.
        Takes what mask_regions_dev wrote; region_hulls_dev takes d_external / d_num_external in place of
        d_regions / d_num_kept for the hulls of the external records only."""
        return self._check(lib().mdx_region_parents_dev(
            self._h, batch, _v(d_labels), w, h, _v(d_regions), max_regions, _v(d_num_kept), _v(d_parent), _v(d_external),
            _v(d_num_external)))

    def mask_regions_dev(self, batch: int, d_mask: int, w: int, h: int, stride: int, frame_stride: int,
                         open3: bool = True, min_area: int = 1, d_regions: int = 0, max_regions: int = 0,
                         d_num_all: int = 0, d_num_kept: int = 0, d_labels: int = 0, d_mask_out: int = 0) -> int:
        """Asynchronous on the context stream (include/mdx.h mdx_mask_regions_dev); pointers are ints."""
        return self._check(lib().mdx_mask_regions_dev(
            self._h, batch, _v(d_mask), w, h, stride, frame_stride, _lib.REGIONS_OPEN3 if open3 else 0, int(min_area),
            _v(d_regions), max_regions, _v(d_num_all), _v(d_num_kept), _v(d_labels), _v(d_mask_out)))

    # -- background subtraction (include/mdx.h mdx_bg_*); a model is an int handle
    def bg_create(self, streams: int, w: int, h: int, channels: int, **params) -> int:
        """A background model of `streams` independent w x h streams; params: mdx_bg_params fields."""
        p = _lib.bg_default_params(**params)
        out = C.c_void_p(0)
        self._check(lib().mdx_bg_create(self._h, streams, w, h, channels, C.byref(p), C.byref(out)))
        return out.value

    def bg_destroy(self, bg: int):
        self._check(lib().mdx_bg_destroy(self._h, _v(bg)))

    def bg_reset(self, bg: int):
        self._check(lib().mdx_bg_reset(self._h, _v(bg)))

    def bg_frames(self, bg: int) -> int:
        return self._check(lib().mdx_bg_frames(self._h, _v(bg)))

    def bg_apply_dev(self, bg: int, T: int, d_frames: int, stride: int, frame_stride: int, stream_stride: int = 0,
                     learning_rate: float = -1.0, d_fgmask: int = 0) -> int:
        """Asynchronous on the context stream (include/mdx.h mdx_bg_apply_dev); pointers are ints."""
        return self._check(lib().mdx_bg_apply_dev(self._h, _v(bg), T, _v(d_frames), stride, frame_stride, stream_stride,
                                                  float(learning_rate), _v(d_fgmask)))

    def bg_image_dev(self, bg: int, d_out: int) -> int:
        """Asynchronous on the context stream (include/mdx.h mdx_bg_image_dev); pointers are ints."""
        return self._check(lib().mdx_bg_image_dev(self._h, _v(bg), _v(d_out)))

    def bg_apply(self, bg: int, frame: np.ndarray, learning_rate: float = -1.0, want_mask: bool = True):
        """One frame (h, w) or (h, w, 3) of a one-stream model, synchronous; returns the (h, w) mask."""
        frame = _frame_view(frame)
        mask = np.empty(frame.shape[:2], np.uint8) if want_mask else None
        self._check(lib().mdx_bg_apply(self._h, _v(bg), _ptr(frame), frame.strides[0], float(learning_rate), _ptr(mask)))
        return mask

    def bg_image(self, bg: int, h: int, w: int, channels: int) -> np.ndarray:
        out = np.empty((h, w) if channels == 1 else (h, w, channels), np.uint8)
        self._check(lib().mdx_bg_image(self._h, _v(bg), _ptr(out)))
        return out

    def bg_get_state(self, bg: int, stream: int, h: int, w: int, channels: int, nmixtures: int) -> dict:
        """One stream's model in the canonical host layout (include/mdx.h mdx_bg_get_state)."""
        st = {"weight": np.empty((h, w, nmixtures), np.float32), "variance": np.empty((h, w, nmixtures), np.float32),
              "mean": np.empty((h, w, nmixtures, channels), np.float32), "modes": np.empty((h, w), np.uint8)}
        nf = C.c_int(0)
        self._check(lib().mdx_bg_get_state(self._h, _v(bg), stream, _ptr(st["weight"]), _ptr(st["variance"]),
                                           _ptr(st["mean"]), _ptr(st["modes"]), C.byref(nf)))
        st["nframes"] = nf.value
        return st

    def bg_set_state(self, bg: int, stream: int, state: dict):
        a = {k: np.ascontiguousarray(state[k], np.uint8 if k == "modes" else np.float32)
             for k in ("weight", "variance", "mean", "modes")}
        self._check(lib().mdx_bg_set_state(self._h, _v(bg), stream, _ptr(a["weight"]), _ptr(a["variance"]), _ptr(a["mean"]),
                                           _ptr(a["modes"]), int(state.get("nframes", 0))))

    # -- half-size ingest (the node's cv::resize(img, out, Size(), 0.5, 0.5), node.cpp:470-474)
    def resize_half(self, image: np.ndarray) -> np.ndarray:
        """image: (h, w) or (h, w, 3) uint8, a row-pitched view allowed.  Returns a new packed array of
        half_size(w, h)."""
        im = _frame_view(image)
        if im.ndim not in (2, 3) or (im.ndim == 3 and im.shape[2] != 3):
            raise ValueError("image must be (h, w) or (h, w, 3)")
        h, w = im.shape[:2]
        cn = 1 if im.ndim == 2 else 3
        dw, dh = half_size(w, h)
        out = np.empty((dh, dw) if cn == 1 else (dh, dw, 3), np.uint8)
        self._check(lib().mdx_resize_half(self._h, _ptr(im), w, h, im.strides[0], cn, _ptr(out), dw * cn))
        return out

    def resize_half_dev(self, batch: int, d_src: int, w: int, h: int, stride: int, frame_stride: int, channels: int,
                        d_dst: int, dst_stride: int, dst_frame_stride: int) -> int:
        """Asynchronous on the context stream (include/mdx.h mdx_resize_half_dev); pointers are ints."""
        return self._check(lib().mdx_resize_half_dev(self._h, batch, _v(d_src), w, h, stride, frame_stride, channels,
                                                     _v(d_dst), dst_stride, dst_frame_stride))

    # -- device entries (pointers are ints, e.g. torch.Tensor.data_ptr())
    def flow_warp_diff_batch_dev(self, batch: int, d_img1: int, d_img2: int, w: int, h: int, stride: int,
                                 frame_stride: int, fmt: int = _lib.FMT_GRAY8, d_next_pts: int = 0, d_status: int = 0,
                                 d_vectors: int = 0, d_mask: int = 0, d_H: int = 0, d_H_external: int = 0,
                                 d_num_vectors: int = 0) -> int:
        return self._check(lib().mdx_flow_warp_diff_batch_dev(
            self._h, batch, _v(d_img1), _v(d_img2), w, h, stride, frame_stride, fmt, _v(d_next_pts), _v(d_status),
            _v(d_vectors), _v(d_mask), _v(d_H), _v(d_H_external), _v(d_num_vectors)))

    def warp_diff_dev(self, batch: int, d_gray1: int, d_gray2: int, w: int, h: int, stride: int, frame_stride: int,
                      d_H: int, d_mask: int) -> int:
        return self._check(lib().mdx_warp_diff_dev(self._h, batch, C.c_void_p(d_gray1), C.c_void_p(d_gray2), w, h,
                                                   stride, frame_stride, C.c_void_p(d_H), C.c_void_p(d_mask)))

    def debug_warp_paths(self) -> np.ndarray:
        """Test hook (include/mdx.h mdx_debug_warp_paths): the k_warp_diff row path of every (pair,
        tile) of this context's last warp launch, after a sync, as a flat int32 array (pair-major,
        tile column fastest): 0 general, 1 fixed point, 2 affine FP64, 3 projective, -1 no fit."""
        n = self._check(lib().mdx_debug_warp_paths(self._h, None, 0))
        out = np.empty(n, np.int32)
        self._check(lib().mdx_debug_warp_paths(self._h, _ptr(out), n))
        return out

    def probe_stream3_dev(self, n: int, d_a: int, d_b: int, d_mask: int, thresh: int = 190) -> int:
        """Memory-ceiling probe of k_warp_diff's 3 B/px access mix (include/mdx.h)."""
        return self._check(lib().mdx_probe_stream3_dev(self._h, n, C.c_void_p(d_a), C.c_void_p(d_b),
                                                       C.c_void_p(d_mask), thresh))

    # -- row-tiled path (one pair split by rows over ranks; include/mdx.h mdx_band_*)
    def band_flow_dev(self, d_img1: int, d_img2: int, w: int, h: int, stride: int, fmt: int, y0: int, y1: int,
                      d_next_pts: int, d_status: int, d_cand: int, d_vectors: int = 0) -> int:
        return self._check(lib().mdx_band_flow_dev(self._h, _v(d_img1), _v(d_img2), w, h, stride, fmt, y0, y1,
                                                   _v(d_next_pts), _v(d_status), _v(d_vectors), _v(d_cand)))

    def band_fit_warp_dev(self, nrec: int, d_cands: int, y0: int, y1: int, d_mask_band: int, d_H: int = 0,
                          d_num_vectors: int = 0) -> int:
        return self._check(lib().mdx_band_fit_warp_dev(self._h, nrec, _v(d_cands), y0, y1, _v(d_mask_band), _v(d_H),
                                                       _v(d_num_vectors)))

    def input_ready(self, hip_event: int):
        """The next device-entry call waits for this hipEvent_t (an int handle) before reading its
        input frames (include/mdx.h mdx_input_ready; one-shot)."""
        self._check(lib().mdx_input_ready(self._h, C.c_void_p(hip_event) if hip_event else None))

    def sync(self):
        self._check(lib().mdx_sync(self._h))
        self._ring_hold.clear()

    def device_sync(self):
        self._check(lib().mdx_device_sync(self._h))

    def lk_fallbacks(self) -> dict:
        """LK level-dataflow fallbacks since creation, as of the last sync (include/mdx.h
        mdx_lk_fallbacks): waits that gave up and levels recomputed -- statistics, not errors."""
        if not hasattr(lib(), "mdx_lk_fallbacks"):     # (variant builds of older sources: A/B runs)
            return None
        v = (C.c_longlong * 3)()
        self._check(lib().mdx_lk_fallbacks(self._h, v))
        return {"group_giveups": v[0], "gate_giveups": v[1], "levels_recomputed": v[2]}

    @property
    def stream(self) -> int:
        return lib().mdx_stream(self._h) or 0

    def enable_timing(self, on: bool = True):
        self._check(lib().mdx_enable_timing(self._h, int(on)))

    def stage_ms(self) -> dict:
        """Per-stage device ms summed over the calls since enable_timing(); 'calls' = count."""
        names = ["gray_pad", "pyrdown", "scharr", "lk", "classify_fit", "warp_diff", "total"]
        out = {"calls": lib().mdx_timing_calls(self._h)}
        for i, nm in enumerate(names):
            ms = C.c_float(0)
            self._check(lib().mdx_stage_ms(self._h, i, C.byref(ms)))
            out[nm] = ms.value
        return out

    # -- device memory helpers (no torch needed)
    def dev_alloc(self, nbytes: int) -> int:
        p = lib().mdx_dev_alloc(self._h, nbytes)
        if not p:
            raise MdxError(lib().mdx_last_error(self._h).decode())
        return p

    def dev_free(self, ptr: int):
        self._check(lib().mdx_dev_free(self._h, C.c_void_p(ptr)))

    def h2d(self, dst: int, src: np.ndarray):
        src = np.ascontiguousarray(src)
        self._check(lib().mdx_memcpy_h2d(self._h, C.c_void_p(dst), _ptr(src), src.nbytes))

    def d2h(self, dst: np.ndarray, src: int):
        self._check(lib().mdx_memcpy_d2h(self._h, _ptr(dst), C.c_void_p(src), dst.nbytes))


class _HostBlock:
    """Owner of one mdx_host_alloc block; freed when the last array viewing it goes away."""

    def __init__(self, nbytes: int):
        self.nbytes = max(1, nbytes)
        self.ptr = lib().mdx_host_alloc(self.nbytes)
        if not self.ptr:
            raise MdxError(f"mdx_host_alloc({nbytes}) failed")

    def __del__(self):
        try:
            lib().mdx_host_free(C.c_void_p(self.ptr))
        except Exception:
            pass


class PinnedArray(np.ndarray):
    """numpy array over page-locked host memory; views keep the block alive through their base."""
    _blk = None


def host_empty(shape, dtype=np.uint8) -> np.ndarray:
    """A numpy array in page-locked host memory (include/mdx.h mdx_host_alloc): frames and outputs
    in it cross PCIe by DMA at full rate.  The block is freed with the array."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    blk = _HostBlock(n)
    raw = (C.c_uint8 * blk.nbytes).from_address(blk.ptr)
    # the block hangs off the lowest buffer object: numpy collapses a view's base chain down to
    # `raw` (np.asarray, .view(np.ndarray) and ascontiguousarray skip the PinnedArray), so every
    # view of the memory keeps it alive
    raw._blk = blk
    arr = np.frombuffer(raw, dtype=np.uint8, count=n).view(dtype).reshape(shape).view(PinnedArray)
    arr._blk = blk
    return arr


def synth_pair(seed: int, w: int, h: int, channels: int = 1, nthreads: int = 0):
    """Deterministic synthetic frame pair.  Returns (img1, img2, H_true)."""
    shape = (h, w) if channels == 1 else (h, w, channels)
    a = np.empty(shape, np.uint8)
    b = np.empty(shape, np.uint8)
    H = np.zeros(9, np.float64)
    rc = lib().mdx_synth_pair(seed, w, h, channels, _ptr(a), _ptr(b), _ptr(H), nthreads)
    if rc != 0:
        raise MdxError(f"mdx_synth_pair failed ({rc})")
    return a, b, H.reshape(3, 3)
