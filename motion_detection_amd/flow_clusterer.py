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

With egomotion off the node clusters the last trajectory pass's Vec4d image instead
(getClusters, flow_clusterer.cpp:178-227, node.cpp:375): first fit by distance and angle.

    clusters = fc.getClusters(optical_flow_vectors, pixel_step, distance_threshold, angular_threshold)

* flow_vectors: the (h, w, 4) float64 Vec4d image; its grid is visited in the reference's order,
  image rows outer (y-major), and only vectors with a non-zero flow take part.
* returns the clusters with more than 5 vectors (:213) as (n_k, 4) float64 arrays, in creation
  order, members in visiting order, like the reference's vector<vector<Vec4d>>.

All pair tests run on the MI355X through libmdx.so (mdx_cluster_euclidean, mdx_cluster_vectors); there is no CPU
fallback.  Restated from the source; unpinned against a real build (no OpenCV 2.4 to compare with):
the copyTo conversion (cvRound) and boundingRect in particular.
"""
from __future__ import annotations

import numpy as np

from .context import ClusterResult, Context, VectorClusterResult

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


def hulls_of(clusters, context: Context) -> list:
    """cv::convexHull of each cluster after cv::Mat(cluster).copyTo(vector<cv::Point>), as
    showClusterContours takes it (optical_flow_visualizer.cpp:204-221): one (v_k, 2) int32 array per
    cluster, in cv::convexHull(.., clockwise=false)'s order (include/mdx.h mdx_cluster_hulls).  For
    callers that hold member lists, next to bounding_rects; every hull is computed on the device, in one
    call on `context`.  An empty cluster has no hull and raises."""
    members = [np.asarray(c, dtype=np.float32).reshape(-1, 2) for c in clusters]
    if not members:
        return []
    labels = np.repeat(np.arange(len(members), dtype=np.int32), [len(m) for m in members])
    return context.cluster_hulls(np.concatenate(members), labels, np.arange(len(members), dtype=np.int32))


def grid_vectors(flow_vectors, pixel_step: int) -> np.ndarray:
    """The Vec4d image's grid as getClusters visits it (flow_clusterer.cpp:180-184): rows i = 0,
    pixel_step, .. outer, columns j inner -- y-major, unlike the x-major grid of the flow entries.
    (n, 4) float64."""
    img = np.asarray(flow_vectors, dtype=np.float64)
    if img.ndim != 3 or img.shape[2] != 4:
        raise ValueError("flow_vectors must be (h, w, 4)")
    ps = int(pixel_step)
    return np.ascontiguousarray(img[::ps, ::ps]).reshape(-1, 4)


class FlowClusterer:
    def __init__(self, device: int = 0, context: Context | None = None):
        """context: an existing Context to run on (not closed by this object); else one is created
        on `device` at the first call."""
        self._device = device
        self._ctx = context
        self._own = context is None
        self.last: ClusterResult | VectorClusterResult | None = None
        self._last_points = None      # (n, 2) float32: the last call's members, one per entry of last.labels

    def clusterEuclidean(self, points, distance_threshold: float) -> list:
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float32)).reshape(-1, 2)
        if self._ctx is None:
            self._ctx = Context(self._device, 64, 64, 1)
        res = self._ctx.cluster_euclidean(pts, float(distance_threshold), MIN_SIZE)
        self.last, self._last_points = res, pts
        return clusters_from_labels(pts, res.labels, res.kept)

    def getClusters(self, flow_vectors, pixel_step: int, distance_threshold: float, angular_threshold: float,
                    abs_int: bool = False) -> list:
        """abs_int: the reference's int abs on the angular distance (include/mdx.h MDX_VCLUSTER_ABS_INT)."""
        vec = grid_vectors(flow_vectors, pixel_step)
        if self._ctx is None:
            self._ctx = Context(self._device, 64, 64, 1)
        res = self._ctx.cluster_vectors(vec, float(distance_threshold), float(angular_threshold), MIN_SIZE, abs_int)
        self.last, self._last_points = res, vec[:, :2].astype(np.float32)   # cv::Point2f(vec[0], vec[1]) (node.cpp:382)
        return [vec[res.labels == int(k)] for k in res.kept]

    def hulls(self) -> list:
        """The convex hulls of the last call's kept clusters (showClusterContours' cv::convexHull,
        optical_flow_visualizer.cpp:204-221): one (v_k, 2) int32 array per cluster of `last.kept`, computed
        on the device (Context.cluster_hulls)."""
        if self.last is None:
            raise ValueError("hulls() follows clusterEuclidean or getClusters")
        return self._ctx.cluster_hulls(self._last_points, self.last.labels, self.last.kept)

    def close(self):
        if self._ctx is not None and self._own:
            self._ctx.close()
        self._ctx = None
