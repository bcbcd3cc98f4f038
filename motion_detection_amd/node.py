"""ROS-free core of MotionDetectionNode for the hot path (the drop-in boundary's caller).

Reproduces the ingest semantics of MotionDetectionNode::imageCallback
(ros/src/motion_detection_node.cpp:235-287) and the runOpticalFlow caller (:76-92), without
ROS: frames arrive as ``Image`` records shaped like sensor_msgs/Image (height, width,
encoding, step, data).  Parameters mirror the node's ROS params (:29-44, :237-245):

* skip_frames (default 1) and num_motions (default 2) are re-read on every frame;
  trajectory_size = 2*num_motions + 1, or 2 when egomotion is false (:241-245).
* a frame is dropped unless global_frame_count % skip_frames == 0 (:247).  The counter
  advances on every call: on a dropped frame at :247, on a kept one at :454 (:315 when no
  trajectory survives), so skip_frames = k keeps frames 0, k, 2k, ...
* raw frames go into a ring of trajectory_size (:248-261); once full, the last two
  frames are converted to rgb8 (cv_bridge toCvCopy, :271) and handed to the calculator.

Publishing is a callback: ``on_result(result)`` receives the FlowResult (vectors + mask),
standing in for publishImage on ~optical_flow_image (:83-85).

By default (``live_chain=True``, as the reference's imageCallback and host/mdx_host.h) the callback
follows the reference's live branch (:266-348): every ring frame goes to
calculateOpticalFlowTrajectory (:295, runOpticalFlowTrajectory :94-110); with egomotion and at
least one complete trajectory, fitSubspace(trajectories, outlier_points, num_motions, sigma) follows
(:341-348), and, when the ``distance_threshold`` parameter is set, clusterEuclidean on its outlier
points (:355) and each kept cluster's bounding rectangle (optical_flow_visualizer.cpp:223-240), the
rectangles MotionLogger::writeBoundingBox logs under ``log_contours`` (:431-434).  Without egomotion
the ring holds 2 frames and, when ``distance_threshold`` and ``angular_threshold`` are both set,
FlowClusterer::getClusters runs on the trajectory pass's Vec4d image (:375, first fit by distance and
angle; ``abs_int`` selects the reference's truncating abs); each kept cluster's points
(:376-386) and rectangle follow the same way.  ``on_result`` then receives a LiveResult.
``live_chain=False`` drives the pair path the north star names (runOpticalFlow, :76-92) on the ring's last two frames, the only one that
produces the motion mask.  With ``region_min_area`` set, that mask is labelled into regions on the
device (BackgroundSubtractor::getMotionContours' recipe: ``region_open`` is its 3x3 opening) and the
FlowResult carries them as ``regions``; under ``log_contours`` each kept region's rectangle is logged
like a cluster's.  With ``detect_outliers`` (off by default: the reference's call at :405 is commented
out) and both thresholds set, the pair callback also runs MotionDetectionNode::detectOutliers
(:112-160) on the pair's Vec4d image: findOutliers (``include_zeros`` is its parameter) ->
getOutlierVectors -> getClusters; the FlowResult then carries ``outlier_flags``, ``vector_clusters``,
``clusters`` and ``rectangles``, and under ``log_contours`` the rectangles are logged.

With ``cluster_contours`` (off by default) every clustering stage above is followed by
showClusterContours' convex hull of each kept cluster (:393, :510; optical_flow_visualizer.cpp:204-221),
computed on the device (mdx_cluster_hulls): the result carries them as ``contours``, and
under ``log_contours`` each is written with MotionLogger::writeContour behind the frame's rectangle
lines (the reference's loop at :426-429 is commented out, hence the opt-in).  Drawing them
(drawContours, the published cluster_image) is out of scope.  With ``region_contours`` (off by default)
and ``region_min_area`` set, the regions come with the convex hull of each (mdx_mask_region_hulls,
DESIGN.md §7k: the label image stays on the device) as ``regions.hulls``, logged the same way behind
the frame's region rectangles.  With ``region_external`` (off by default) and ``region_min_area`` set,
``regions`` is a RegionTreeResult: every kept record still, plus each one's ``parent`` blob and the
``external`` ones' indices (findContours' RETR_EXTERNAL, mdx_mask_regions_tree); the logged
rectangles and, with ``region_contours``, ``regions.hulls`` and the logged contours cover the external
records only.  With ``region_outlines`` (off by default) and ``region_min_area`` set, the regions come with the
outer border polyline of each -- the point list findContours itself returns (mdx_mask_region_outlines,
DESIGN.md §7m) -- as ``regions.outlines``, each logged with writeContour behind the frame's hull lines; it
combines with ``region_external`` as ``region_contours`` does.

With ``use_all_frames=False`` the callback only fills the ring (:262) and the reference's polling caller
run() (:457-553) does the work: ``run_once()`` is one pass of its body (:464-529) and ``run()`` the loop.
Every ring frame wider than 320 px is halved (cv::resize(img, out, Size(), 0.5, 0.5), :470-474) -- here
on the device, on its way into the context's resident ring, which each message enters once --, then the
trajectories, fitSubspace(trajectories, outlier_points, 2, residual_threshold) (:494: the 2 is hard-coded
there, whatever ``num_motions`` says, which still sizes the ring) and clusterEuclidean (:497).  run() has
no egomotion branch and writes no motion.log.  Two passes without a new frame see the same ring and a
further-advanced rand() stream, as the reference's spinning loop does.
"""
from __future__ import annotations

import os
from collections import deque
from dataclasses import dataclass, field
from typing import Callable

import numpy as np

from . import _lib
from .background_subtractor import BackgroundSubtractor
from .context import grid_points, half_size
from .flow_clusterer import FlowClusterer, bounding_rects
from .formats import MotionLogger
from .optical_flow_calculator import OpticalFlowCalculator
from .outlier_detector import OutlierDetector

ENCODINGS = {"mono8": (1, _lib.FMT_GRAY8), "rgb8": (3, _lib.FMT_RGB8), "bgr8": (3, _lib.FMT_BGR8)}


@dataclass
class Image:
    """Minimal sensor_msgs/Image."""
    height: int
    width: int
    encoding: str
    step: int
    data: bytes | np.ndarray

    @staticmethod
    def from_array(a: np.ndarray, encoding: str | None = None) -> "Image":
        a = np.ascontiguousarray(a, dtype=np.uint8)
        enc = encoding or ("mono8" if a.ndim == 2 else "rgb8")
        return Image(a.shape[0], a.shape[1], enc, a.strides[0], a.tobytes())


def to_rgb8(msg: Image) -> np.ndarray:
    """cv_bridge::toCvCopy(msg, "rgb8"): mono8 is replicated, bgr8 is reordered."""
    if msg.encoding not in ENCODINGS:
        raise ValueError(f"unsupported encoding {msg.encoding!r}")
    cn, _ = ENCODINGS[msg.encoding]
    buf = np.frombuffer(bytes(msg.data) if not isinstance(msg.data, np.ndarray) else msg.data.tobytes(), np.uint8)
    rows = buf[: msg.step * msg.height].reshape(msg.height, msg.step)[:, : msg.width * cn]
    if cn == 1:
        return np.repeat(rows[:, :, None], 3, axis=2)
    px = rows.reshape(msg.height, msg.width, 3)
    return px[:, :, ::-1].copy() if msg.encoding == "bgr8" else px.copy()


@dataclass
class LiveResult:
    """Outputs of the live branch (node.cpp:266-355, :431-434): trajectories, fitSubspace's outliers
    and, when clustering is on (egomotion and a distance_threshold), their clusters and rectangles;
    without egomotion and with both thresholds, getClusters' clusters of the flow vectors instead."""
    num_vectors: int
    optical_flow_vectors: np.ndarray     # (h, w, 4) Vec4d image (runOpticalFlowTrajectory :97-99)
    trajectories: list                   # complete trajectories, (T, 2) each
    outlier_points: list                 # fitSubspace's (egomotion only)
    subspace: list                       # fitSubspace's return value (egomotion only)
    clusters: list = field(default_factory=list)     # clusterEuclidean's kept clusters, (n_k, 2) float32 each
    rectangles: list = field(default_factory=list)   # their (x, y, width, height), as cv::Rect
    frame_number: int = 0                # global_frame_count_ of this callback (the log's frame column)
    vector_clusters: list = field(default_factory=list)   # getClusters' kept clusters, (n_k, 4) float64 each (no egomotion)
    contours: list = field(default_factory=list)     # the clusters' convex hulls, (v_k, 2) int32 each (cluster_contours)


class MotionDetectionNode:
    def __init__(self, params: dict | None = None, on_result: Callable | None = None, device: int = 0):
        # the reference's defaults (node.cpp:29-44, :237-240, :346); egomotion true (:40) sets a
        # ring of 2*num_motions+1 frames, and imageCallback always runs the live branch on it
        # (live_chain True; False selects the pair path on the ring's last two frames)
        self.params = {"pixel_step": 10, "min_vector_size": 1.0, "skip_frames": 1, "num_motions": 2,
                       "egomotion": True, "use_all_frames": True, "sigma": 0.5, "live_chain": True,
                       # run()'s fitSubspace threshold (:491); only run_once() reads it
                       "residual_threshold": 0.2,
                       # clustering: distance_threshold has no default in the reference (node.cpp:34;
                       # the launch files set it) -- None leaves the stage off; log_contours false (:39), log_path "" (:42)
                       "distance_threshold": None, "log_contours": False, "log_path": "",
                       # getClusters (no egomotion, :375): angular_threshold has no default either -- None
                       # leaves the stage off; abs_int: the angular distance truncated (int abs)
                       "angular_threshold": None, "abs_int": False,
                       # the pair path's mask labelled into regions (getMotionContours' recipe):
                       # region_min_area None leaves the stage off; region_open is the 3x3 opening
                       "region_min_area": None, "region_open": True,
                       # the pair path's detector (detectOutliers, :112-160): off by default, the
                       # reference's call (:405) is commented out; include_zeros is findOutliers' argument
                       "detect_outliers": False, "include_zeros": False,
                       # showClusterContours' convex hull of every kept cluster (node.cpp:393, :510):
                       # off by default, the reference's writeContour loop (:426-429) is commented out
                       "cluster_contours": False,
                       # the convex hull of every kept mask region (region_min_area set): off by
                       # default; logged with writeContour behind the frame's region rectangles
                       "region_contours": False,
                       # findContours' RETR_EXTERNAL (region_min_area set): regions keeps every
                       # kept record and gains parent / external; what is logged covers the external records only
                       "region_external": False,
                       # the outer border polyline of every kept mask region, findContours' own point list
                       # (region_min_area set): off by default; logged with writeContour behind the hulls
                       "region_outlines": False,
                       # the reference's BackgroundSubtractor bs_ (motion_detection_node.h:93): every
                       # frame that enters the ring also updates a MOG2 model of its size on the device; with
                       # region_min_area and a log_path set, the external regions of its opened mask go to
                       # motion_bg.log beside the log_path.  Off by default
                       "background_subtraction": False}
        if params:
            self.params.update(params)
        self.on_result = on_result
        self.raw_images: deque = deque()
        self.global_frame_count = 0
        self.image_received = False
        self.frames_processed = 0
        self.ofc = OpticalFlowCalculator(device=device)
        self.od = None                                    # the live path's OutlierDetector (own context, the
        self.fc = None                                    # rand() stream) and FlowClusterer, created on first use
        self.logger = None                                # MotionLogger (log_contours with a log_path)
        self._pair_tools = None                           # detect_outliers' (context, detector, clusterer)
        self._device = device
        self.bs = None                                    # background_subtraction's BackgroundSubtractor
        self.bg_logger = None                             # its MotionLogger (motion_bg.log)
        self.bg_rectangles: list = []                     # the newest frame's external regions of its mask
        self.bg_contours: list = []
        self._ring_msgs: list = []                        # run_once: the messages held by the device ring, oldest
        self._ring_ctx = None                             # first, and the context whose ring it is

    def _detector(self):
        if self.od is None:
            self.od = OutlierDetector(seed=self.params.get("seed"), device=self._device)
        return self.od

    def _clusterer(self):
        if self.fc is None:
            self.fc = FlowClusterer(device=self._device)
        return self.fc

    def _pair_detector_and_clusterer(self):
        # on the calculator's context, kept across frames (made again only when the calculator has replaced
        # its context); not the live path's od / fc, which own contexts and, od, the live rand() stream
        ctx = self.ofc.context
        if self._pair_tools is None or self._pair_tools[0] is not ctx:
            self._pair_tools = (ctx, OutlierDetector(context=ctx), FlowClusterer(context=ctx))
        return self._pair_tools[1:]

    def _log_rectangles(self, rects):
        """MotionLogger::writeBoundingBox of each rectangle (node.cpp:431-434) when log_contours and a
        log_path are set; the logger is created by the first stage that logs, rectangles or not."""
        if not (self.params.get("log_contours") and self.params.get("log_path")):
            return
        if self.logger is None:
            self.logger = MotionLogger(self.params["log_path"])
        for k, rect in enumerate(rects):
            self.logger.writeBoundingBox(rect, self.global_frame_count, k)

    def _contours(self, fc, log: bool = True) -> list:
        """showClusterContours' cv::convexHull of every kept cluster of fc's last call (node.cpp:393, :510)
        under ``cluster_contours``, on the device; each is logged with MotionLogger::writeContour(hull,
        frame, i) (:426-429) behind the rectangles' lines when log_contours and a log_path are set (log False:
        run(), which writes no motion.log)."""
        if not self.params.get("cluster_contours"):
            return []
        hulls = fc.hulls()
        if log:
            self._log_contours(hulls)
        return hulls

    def _log_contours(self, hulls):
        """MotionLogger::writeContour(hull, frame, i) of each hull when log_contours and a log_path are set."""
        if not (self.params.get("log_contours") and self.params.get("log_path")):
            return
        if self.logger is None:
            self.logger = MotionLogger(self.params["log_path"])
        for k, hull in enumerate(hulls):
            self.logger.writeContour(hull, self.global_frame_count, k)

    def _update_background(self, frame: np.ndarray):
        """BackgroundSubtractor::getMotionContours on the frame that just entered the ring: the model update and,
        with region_min_area set, the external regions of its opened mask, one writeBoundingBox line each in
        motion_bg.log (beside log_path) when a log_path is set."""
        min_area = self.params.get("region_min_area")
        if self.bs is None:
            self.bs = BackgroundSubtractor(device=self._device, min_area=int(min_area or 1))
        if min_area is None:
            self.bs.apply(frame, want_mask=False)
            return
        self.bs.min_area = int(min_area)
        self.bg_contours, self.bg_rectangles = self.bs.getMotionContours(frame)
        if not self.params.get("log_path"):
            return
        if self.bg_logger is None:
            self.bg_logger = MotionLogger(os.path.join(os.path.dirname(self.params["log_path"]), "motion_bg.log"))
        for k, rect in enumerate(self.bg_rectangles):
            self.bg_logger.writeBoundingBox(rect, self.global_frame_count, k)

    @property
    def trajectory_size(self) -> int:
        # node.cpp:241-245
        return 2 if not self.params["egomotion"] else 2 * int(self.params["num_motions"]) + 1

    def image_callback(self, msg: Image):
        skip = int(self.params.get("skip_frames", 1))
        if self.global_frame_count % skip != 0:          # :247
            self.global_frame_count += 1
            return None
        ts = self.trajectory_size
        if len(self.raw_images) < ts:                     # :248-261
            self.raw_images.append(msg)
            if len(self.raw_images) == ts:
                self.image_received = True
        else:
            self.raw_images.append(msg)
            self.raw_images.popleft()
            self.image_received = True
        if self.params.get("background_subtraction"):
            self._update_background(to_rgb8(msg))
        out = None
        if self.params.get("use_all_frames", True) and self.image_received:
            if self.params.get("live_chain", True):
                out = self.run_live_chain([to_rgb8(m) for m in self.raw_images])   # :266-295
            else:
                frames = [to_rgb8(m) for m in list(self.raw_images)[-2:]]   # :266-287
                out = self.run_optical_flow(frames[0], frames[1])
        self.global_frame_count += 1                          # :454
        return out

    def run_live_chain(self, images: list):
        """runOpticalFlowTrajectory (node.cpp:94-110), then fitSubspace (:341-348, egomotion), then one
        of the two clustering stages, then the kept clusters' rectangles and their log lines."""
        h, w = images[0].shape[:2]
        vec = np.zeros((h, w, 4))                         # cv::Mat::zeros(rows, cols, CV_32FC4) (:97)
        trajectories: list = []
        num = self.ofc.calculateOpticalFlowTrajectory(images, vec, trajectories, int(self.params["pixel_step"]),
                                                      None, float(self.params["min_vector_size"]))
        ego = bool(self.params["egomotion"])
        thr, athr = self.params.get("distance_threshold"), self.params.get("angular_threshold")
        outliers, subspace, vector_clusters, rectangles, contours = [], [], [], [], []
        if trajectories and ego:                                                                      # :341-348
            subspace = self._detector().fitSubspace(trajectories, outliers, int(self.params["num_motions"]),
                                                    float(self.params["sigma"]))
        clusters = None                                   # None: no clustering stage ran
        if trajectories and ego and thr is not None:
            clusters = self._clusterer().clusterEuclidean(np.asarray(outliers, np.float32).reshape(-1, 2), float(thr))   # :355
        elif trajectories and not ego and thr is not None and athr is not None:
            vector_clusters = self._clusterer().getClusters(vec, int(self.params["pixel_step"]), float(thr), float(athr),
                                                            bool(self.params.get("abs_int", False)))   # :375
            clusters = [c[:, :2].astype(np.float32) for c in vector_clusters]                         # :376-386
        if clusters is not None:
            rectangles = bounding_rects(clusters)                                                     # :395
            self._log_rectangles(rectangles)                                                          # :431-434
            contours = self._contours(self._clusterer())                                              # :393
        self.frames_processed += 1
        res = LiveResult(num, vec, trajectories, outliers, subspace, clusters or [], rectangles, self.global_frame_count,
                         vector_clusters, contours)
        if self.on_result is not None:
            self.on_result(res)
        return res

    def _sync_ring(self, msgs: list) -> bool:
        """Bring the device ring up to date with `msgs` (raw_images, oldest first): every message that has
        entered since the last pass is converted (toCvCopy "rgb8", :469) and pushed once, halved when
        wider than 320 px (:470-474).  False: the ring could not take them all (frames of several sizes)."""
        ps, mvs = int(self.params["pixel_step"]), float(self.params["min_vector_size"])
        held, keep = self._ring_msgs, len(msgs)
        # the messages to keep: the longest tail of the ring's that heads msgs
        k = min(len(held), keep)
        while k > 0 and not all(a is b for a, b in zip(held[-k:], msgs[:k])):
            k -= 1
        if k == 0:
            held = []
            if self._ring_ctx is not None:
                self._ring_ctx.ring_reset()
        for m in msgs[k:]:
            n, ctx = self.ofc.ring_push(to_rgb8(m), keep, m.width > 320, ps, mvs)
            if ctx is not self._ring_ctx or n != min(len(held) + 1, keep):
                # a new context (the frame outgrew the old one) or a frame of another size: the ring was
                # empty when this frame entered
                held = []
                self._ring_ctx = ctx
            held = (held + [m])[-keep:]
        self._ring_msgs = held
        return len(held) == keep

    def run_once(self):
        """One pass of run()'s body (node.cpp:464-529); None until image_received.  With no complete
        trajectory (the reference indexes trajectories[0] there, undefined) the fit and the clustering are
        skipped and the result carries empty lists."""
        if not self.image_received:                                                                  # :459
            return None
        msgs = list(self.raw_images)
        if not self._sync_ring(msgs):
            raise ValueError("the ring's frames differ in size")
        w, h = msgs[-1].width, msgs[-1].height
        if w > 320:
            w, h = half_size(w, h)
        vec = np.zeros((h, w, 4))
        trajectories: list = []
        num = self.ofc.ring_trajectory(w, h, len(msgs), vec, trajectories, int(self.params["pixel_step"]),
                                       float(self.params["min_vector_size"]))                        # :488
        outliers, subspace, clusters, rectangles, contours = [], [], [], [], []
        thr = self.params.get("distance_threshold")
        if trajectories:
            subspace = self._detector().fitSubspace(trajectories, outliers, 2,
                                                    float(self.params["residual_threshold"]))        # :494
            if thr is not None:
                clusters = self._clusterer().clusterEuclidean(np.asarray(outliers, np.float32).reshape(-1, 2),
                                                              float(thr))                            # :497
                rectangles = bounding_rects(clusters)
                contours = self._contours(self._clusterer(), log=False)                              # :510
        self.frames_processed += 1
        res = LiveResult(num, vec, trajectories, outliers, subspace, clusters, rectangles, self.global_frame_count,
                         contours=contours)
        if self.on_result is not None:
            self.on_result(res)
        return res

    def run(self, max_runs: int | None = None, spin_once: Callable | None = None) -> list:
        """main()'s polling loop over run() (node.cpp:579-582), for callers that want it.  spin_once, the
        stand-in for ros::spinOnce, is called before every pass to deliver pending frames through
        image_callback; the loop ends when it returns False, after max_runs passes that processed, or,
        without a spin_once, at a pass that finds no full ring.  Returns the results.  The reference's loop
        never ends, so one of the two arguments is required."""
        if max_runs is None and spin_once is None:
            raise ValueError("run() needs max_runs or spin_once: nothing else ends the loop")
        out = []
        while max_runs is None or len(out) < max_runs:
            if spin_once is not None and spin_once() is False:
                break
            res = self.run_once()
            if res is not None:
                out.append(res)
            elif spin_once is None:
                break
        return out

    def detect_outliers(self, h: int, w: int, res, thr: float, athr: float):
        """detectOutliers (node.cpp:112-160) on the pair's Vec4d field: findOutliers, getOutlierVectors,
        getClusters and each kept cluster's rectangle, all on the calculator's context."""
        ps = int(self.params["pixel_step"])
        od, fc = self._pair_detector_and_clusterer()
        vec = np.zeros((h, w, 4))                         # cv::Mat::zeros(rows, cols, CV_32FC4) (:81)
        pts = grid_points(w, h, ps).astype(np.int64)
        vec[pts[:, 1], pts[:, 0], :] = res.vectors
        prob = od.findOutliers(vec, bool(self.params.get("include_zeros", False)), ps)             # :114
        outlier_vectors = od.getOutlierVectors(vec, prob, ps)                                      # :121
        res.outlier_flags = od.last_outliers.flags        # per grid vector, image rows outer
        res.vector_clusters = fc.getClusters(outlier_vectors, ps, thr, athr, bool(self.params.get("abs_int", False)))   # :127
        res.clusters = [c[:, :2].astype(np.float32) for c in res.vector_clusters]
        res.rectangles = bounding_rects(res.clusters)
        self._log_rectangles(res.rectangles)
        res.contours = self._contours(fc)

    def run_optical_flow(self, image1: np.ndarray, image2: np.ndarray):
        """runOpticalFlow (node.cpp:76-92)."""
        res = self.ofc.compute(image1, image2, int(self.params["pixel_step"]), float(self.params["min_vector_size"]),
                               fmt=_lib.FMT_RGB8)
        min_area = self.params.get("region_min_area")
        if min_area is not None and res.mask is not None:
            # the mask is labelled on the device; what comes back is the records
            # (region_contours: and each record's convex hull; the labels stay on the device)
            # (region_external: and each record's parent blob; rectangles and hulls of the external ones)
            # (region_outlines: and each record's outer border polyline; of the external ones likewise)
            want_hulls, external = bool(self.params.get("region_contours")), bool(self.params.get("region_external"))
            want_outlines = bool(self.params.get("region_outlines"))
            res.regions = self.ofc.context.mask_regions(res.mask, open3=bool(self.params.get("region_open", True)),
                                                        min_area=int(min_area), want_hulls=want_hulls,
                                                        **({"want_parents": True} if external else {}),
                                                        **({"want_outlines": True} if want_outlines else {}))
            self._log_rectangles(res.regions.external_rectangles if external else res.regions.rectangles)
            if want_hulls:
                self._log_contours(res.regions.hulls)
            if want_outlines:
                self._log_contours(res.regions.outlines)
        thr, athr = self.params.get("distance_threshold"), self.params.get("angular_threshold")
        if self.params.get("detect_outliers") and thr is not None and athr is not None:
            self.detect_outliers(image1.shape[0], image1.shape[1], res, float(thr), float(athr))
        self.frames_processed += 1
        if self.on_result is not None:
            self.on_result(res)
        return res
