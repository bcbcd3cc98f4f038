"""Mirror of the reference's OutlierDetector: fitSubspace for the trajectory path, findOutliers /
getOutlierVectors for the pair path.

Reference: class OutlierDetector (common/include/motion_detection/outlier_detector.h:14-40),
constructor (common/src/outlier_detector.cpp:15-31: srand(time(NULL)) and the chi-square table),
fitSubspace (:236-331), called by the node on the complete trajectories
(ros/src/motion_detection_node.cpp:345-348):

    od = OutlierDetector()                     # seed=None: time(NULL), as the reference
    subspace = od.fitSubspace(trajectories, outlier_points, num_motions, sigma)

* trajectories: list of (T, 2) arrays (OpticalFlowCalculator.calculateOpticalFlowTrajectory's).
* outlier_points: a list, extended with each outlier trajectory's second-to-last point (:322).
* returns the winning sample's trajectories (4*num_motions of them, repeats possible; empty when
  no hypothesis found an inlier), like the reference's return value.

findOutliers / getOutlierVectors (:37-71) are the pair path's detector
(MotionDetectionNode::detectOutliers, node.cpp:112-160): the median and the median absolute
deviation of the grid vectors' angles and magnitudes, a vector flagged where either modified z-score
exceeds 3.5 (mdx_find_outliers):

    prob = od.findOutliers(optical_flow_vectors, include_zeros, pixel_step)      # (h, w) float64, 1.0 / 0.0
    outlier_vectors = od.getOutlierVectors(optical_flow_vectors, prob, pixel_step)   # (h, w, 4)

The generator is glibc's rand() restated (mdx_srand / mdx_rand), one stream per detector across
calls, like the reference's.  All arithmetic runs on the MI355X through libmdx.so.
"""
from __future__ import annotations

import ctypes as C
import time

import numpy as np

from . import _lib
from .context import Context, OutlierResult, SubspaceResult
from .flow_clusterer import grid_vectors


class OutlierDetector:
    def __init__(self, seed: int | None = None, device: int = 0, precision: int = _lib.SUBSPACE_F64,
                 context: Context | None = None):
        """precision: SUBSPACE_F64 (default, stable) or SUBSPACE_F32 (the reference's float
        arithmetic shape; see include/mdx.h mdx_fit_subspace).  context: an existing Context to run
        on (not closed by this object; its subspace_precision holds); else one is created on `device`
        at the first call."""
        self.precision = int(precision)
        self.rng = _lib.MdxRandState()
        self.seed = int(time.time()) & 0xFFFFFFFF if seed is None else int(seed) & 0xFFFFFFFF
        _lib.lib().mdx_srand(C.byref(self.rng), self.seed)
        self._device = device
        self._ctx: Context | None = context
        self._own = context is None
        self.last: SubspaceResult | None = None
        self.last_outliers: OutlierResult | None = None

    def fitSubspace(self, trajectories, outlier_points: list, num_motions: int, sigma: float) -> list:
        traj = np.ascontiguousarray(np.asarray(trajectories, dtype=np.float32))
        if self._ctx is None:
            self._ctx = Context(self._device, 64, 64, 1, subspace_precision=self.precision)
        res = self._ctx.fit_subspace(traj, num_motions, sigma, self.rng)
        self.last = res
        outlier_points.extend(tuple(p) for p in res.outlier_points)
        return [traj[i] for i in res.columns if i >= 0]

    def findOutliers(self, optical_flow_vectors, include_zeros: bool = False, pixel_step: int = 10) -> np.ndarray:
        """The reference's outlier_probabilities (:37-53): (h, w) float64, 1.0 at every flagged grid
        point, 0 elsewhere (off-grid pixels are never read)."""
        img = np.asarray(optical_flow_vectors, dtype=np.float64)
        vec = grid_vectors(img, pixel_step)
        if self._ctx is None:
            self._ctx = Context(self._device, 64, 64, 1, subspace_precision=self.precision)
        res = self._ctx.find_outliers(vec, bool(include_zeros))
        self.last_outliers = res
        ps = int(pixel_step)
        prob = np.zeros(img.shape[:2], np.float64)
        grid = prob[::ps, ::ps]
        grid[...] = (res.flags != 0).reshape(grid.shape)
        return prob

    def getOutlierVectors(self, optical_flow_vectors, outlier_probabilities, pixel_step: int = 10) -> np.ndarray:
        """(:55-71): (h, w, 4) float64, the Vec4d of every grid point whose probability exceeds 0.5,
        zero elsewhere."""
        img = np.asarray(optical_flow_vectors, dtype=np.float64)
        prob = np.asarray(outlier_probabilities, dtype=np.float64)
        if prob.shape != img.shape[:2]:
            raise ValueError("outlier_probabilities must be (h, w)")
        ps = int(pixel_step)
        vec = grid_vectors(img, ps)
        keep = prob[::ps, ::ps].reshape(-1) > 0.5
        out = np.zeros(img.shape, np.float64)
        grid = out[::ps, ::ps]
        grid[...] = np.where(keep[:, None], vec, 0.0).reshape(grid.shape)
        return out

    def close(self):
        if self._ctx is not None and self._own:
            self._ctx.close()
        self._ctx, self._own = None, True      # a later call creates a context of this object's own
