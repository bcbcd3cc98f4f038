"""Mirror of the reference's FlowClusterer::clusterEuclidean for the live chain's last stage.

Reference: class FlowClusterer (common/include/motion_detection/flow_clusterer.h),
clusterEuclidean (common/src/flow_clusterer.cpp:231-269), called by the node on fitSubspace's
outlier_points (ros/src/motion_detection_node.cpp:355); each returned cluster then becomes a
cv::Rect (optical_flow_visualizer.cpp:223-240) that MotionLogger::writeBoundingBox logs
(node.cpp:431-434):

    fc = FlowClusterer()
    clusters = fc.clusterEuclidean(outlier_points, distance_threshold)
    for k, rect in enumerate(bounding_rects(clusters)):
        logger.writeBoundingBox(rect, frame, k)

* points: (n, 2) float32 (or a list of (x, y)), visited in input order.
* returns the clusters with more than 5 points (:263) as (n_k, 2) float32 arrays, in creation
  order, members in input order, like the reference's vector<vector<Point2f>>.

All pair distances run on the MI355X through libmdx.so (mdx_cluster_euclidean); there is no CPU
fallback.  Restated from the source; unpinned against a real build (no OpenCV 2.4 to compare with):
the copyTo conversion (cvRound) and boundingRect in particular.
"""
from __future__ import annotations

import numpy as np

from .context import ClusterResult, Context

MIN_SIZE = 5          # clusters.at(i).size() > 5 (flow_clusterer.cpp:263)


def clusters_from_labels(points: np.ndarray, labels: np.ndarray, kept) -> list:
    """The kept clusters' member lists from a labelling: cluster id k's points in input order, for
    each k of `kept` in order."""
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 2)
    labels = np.asarray(labels)
    return [pts[labels == int(k)] for k in kept]


def bounding_rects(clusters) -> list:
    """cv::boundingRect of each cluster after cv::Mat(cluster).copyTo(vector<cv::Point>)
    (optical_flow_visualizer.cpp:230-236): the points converted with cvRound (round half to even),
    then (x, y, width, height) = (xmin, ymin, xmax - xmin + 1, ymax - ymin + 1).  Tuples that
    formats.MotionLogger.writeBoundingBox accepts.  O(points) on the host; the rectangles of
    Context.cluster_euclidean are the same numbers."""
    out = []
    for c in clusters:
        p = np.rint(np.asarray(c, dtype=np.float32).reshape(-1, 2).astype(np.float64)).astype(np.int64)
        x0, y0 = p.min(axis=0)
        x1, y1 = p.max(axis=0)
        out.append((int(x0), int(y0), int(x1 - x0 + 1), int(y1 - y0 + 1)))
    return out


class FlowClusterer:
    def __init__(self, device: int = 0, context: Context | None = None):
        """context: an existing Context to run on (not closed by this object); else one is created
        on `device` at the first call."""
        self._device = device
        self._ctx = context
        self._own = context is None
        self.last: ClusterResult | None = None

    def clusterEuclidean(self, points, distance_threshold: float) -> list:
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float32)).reshape(-1, 2)
        if self._ctx is None:
            self._ctx = Context(self._device, 64, 64, 1)
        res = self._ctx.cluster_euclidean(pts, float(distance_threshold), MIN_SIZE)
        self.last = res
        return clusters_from_labels(pts, res.labels, res.kept)

    def close(self):
        if self._ctx is not None and self._own:
            self._ctx.close()
        self._ctx = None
