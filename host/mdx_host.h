// mdx_host.h -- ROS-free C++ node core over the C-ABI (include/mdx.h).
//
// The reference's caller of the hot path is MotionDetectionNode (ros/src/motion_detection_node.cpp):
// it subscribes sensor_msgs/Image on ~input_image (:63), keeps a ring of the last
// trajectory_size frames (:237-261), converts them with cv_bridge::toCvCopy(msg, "rgb8") (:271) and
// runs either runOpticalFlow (:76-92, the pair path with the motion mask -- compiled but only
// reachable from commented-out code) or runOpticalFlowTrajectory + fitSubspace + clusterEuclidean
// (:94-110, :341-355, the live path), then publishes RGB8 images (publishImage, :217-223).  This header restates that
// caller without ROS or OpenCV: messages are plain structs, publishing is a callback, and every
// per-pixel step goes through libmdx.so.  No Python anywhere on this path.
#ifndef MDX_HOST_H_
#define MDX_HOST_H_

#include <cstdint>
#include <deque>
#include <fstream>
#include <functional>
#include <string>
#include <vector>

#include "mdx.h"

namespace mdx_host {

// sensor_msgs/Image, the fields the node reads
struct Image {
    uint32_t height = 0, width = 0;
    std::string encoding;          // "mono8", "rgb8" or "bgr8"
    uint32_t step = 0;             // row pitch in bytes
    std::vector<uint8_t> data;
};

// cv_bridge::toCvCopy(msg, "rgb8") (node.cpp:271): mono8 replicated to three channels, bgr8
// reordered, rows made contiguous (step = 3 * width).  Throws std::invalid_argument otherwise.
Image to_rgb8(const Image& msg);

// ROS parameters of the node that the path reads (node.cpp:29-44, :237-240, :346); defaults are the
// reference's own (egomotion true :40, min_vector_size 1.0 :44, skip_frames 1 and num_motions 2
// :238-240, sigma 0.5 :346) except pixel_step, which has no default there (:29; 10 in the launch
// files) and use_all_frames, whose constructor default (false, :37) disagrees with main()'s (true,
// :568) -- every launch file sets it true.
struct Params {
    int pixel_step = 10;
    double min_vector_size = 1.0;
    int skip_frames = 1;
    int num_motions = 2;
    bool egomotion = true;
    bool use_all_frames = true;
    double sigma = 0.5;
    // the polling caller's fitSubspace threshold (run(), node.cpp:491); run_once() reads it, nothing else does
    double residual_threshold = 0.2;
    // which caller body to run per frame: true = the live path (trajectories + fitSubspace,
    // node.cpp:266-348), false = runOpticalFlow on the ring's last two frames (:76-92), the only
    // caller that produces the motion mask
    bool live_path = true;
    uint32_t seed = 1;             // the reference seeds rand() with time(NULL) (outlier_detector.cpp:17)
    int subspace_precision = MDX_SUBSPACE_F64;   // or MDX_SUBSPACE_F32 (the reference's float shape)
    // clusterEuclidean's threshold (node.cpp:320-321, :355; no default there, the launch files set
    // it).  0: the clustering stage is off
    double distance_threshold = 0;
    // getClusters' second threshold (node.cpp:35, :375; no default there, the launch files set it):
    // with egomotion false and both thresholds > 0 the live path clusters the trajectory pass's flow
    // vectors by distance and angle (mdx_cluster_vectors).  0: that stage is off.  abs_int: the
    // angular distance truncated, the reference's int abs (MDX_VCLUSTER_ABS_INT)
    double angular_threshold = 0;
    bool abs_int = false;
    bool log_contours = false;     // node.cpp:39: log each kept cluster's rectangle (mdx_node: motion.log)
    // the pair path's mask labelled into regions on the device (mdx_mask_regions: getMotionContours'
    // recipe, background_subtractor.cpp:31-35).  region_min_area 0: the stage is off; region_open: its
    // 3x3 opening
    int region_min_area = 0;
    bool region_open = true;
    // the pair path's detector (MotionDetectionNode::detectOutliers, node.cpp:112-160; off: the reference's
    // call at :405 is commented out): with live_path false and both thresholds > 0, findOutliers ->
    // getOutlierVectors -> getClusters on the pair's Vec4d field (mdx_find_outliers, mdx_cluster_vectors;
    // DESIGN.md §7h).  include_zeros: findOutliers' argument
    bool detect_outliers = false;
    bool include_zeros = false;
    // showClusterContours' convex hull of every kept cluster (node.cpp:393 live, :510 run();
    // optical_flow_visualizer.cpp:204-221) behind each clustering stage that ran (mdx_cluster_hulls,
    // DESIGN.md §7j).  Off by default: the reference's writeContour loop (:426-429) is commented out, and
    // drawing the hulls (drawContours, the published cluster_image) is out of scope
    bool cluster_contours = false;
    // the convex hull of every kept mask region (regions_on(); mdx_mask_region_hulls): the
    // records and the hulls in one call, the label image staying on the device.  Off by default
    bool region_contours = false;
    // findContours' RETR_EXTERNAL (regions_on(); mdx_mask_regions_tree): `regions` keeps every kept
    // record and gains each one's parent blob and the external ones' indices; with region_contours the hulls are
    // those of the external records.  Off by default
    bool region_external = false;
    // the outer border polyline of every kept mask region, the point list findContours itself returns
    // (regions_on(); mdx_mask_region_outlines), the label image staying on the device; with
    // region_external those of the external records, as region_contours.  Off by default
    bool region_outlines = false;
    // background subtraction (the reference's BackgroundSubtractor bs_, motion_detection_node.h:93; mdx_bg_*,
    // DESIGN.md §7n): every frame that enters the ring also updates a mixture model of its size on the device;
    // with region_min_area > 0 the frame's external regions of the model's opened mask are kept
    // (background_regions(); mdx_node: motion_bg.log).  Whichever path runs.  Off by default
    bool background_subtraction = false;

    // Whether each optional stage runs on a processed frame (the conditions documented above, written
    // once: the node's stages and mdx_node's output files both ask here)
    bool both_thresholds() const { return distance_threshold > 0 && angular_threshold > 0; }
    bool regions_on() const { return !live_path && region_min_area > 0; }
    bool detect_outliers_on() const { return !live_path && detect_outliers && both_thresholds(); }
    bool vector_clusters_on() const { return live_path && !egomotion && both_thresholds(); }
    bool subspace_on() const { return live_path && egomotion; }
    bool point_clusters_on() const { return subspace_on() && distance_threshold > 0; }
    // the polling caller (run_once): which frames enter the device ring, and its clusterEuclidean (:497)
    bool ring_on() const { return live_path || !use_all_frames; }
    bool run_clusters_on() const { return distance_threshold > 0; }
};

// What the optional stages behind the flow write.  A stage that is off or did not run leaves its fields
// as they are here; reset_stages() puts them all back, so a field added here is reset with the rest.
struct StageOutputs {
    std::vector<double> grid;                  // n x 4: grid_vectors(vector_image), when a stage ran on it
                                               // (detect_outliers, getClusters)
    // pair path
    int num_regions_all = 0;                   // region_min_area > 0: every component of the (opened) mask
    std::vector<int32_t> regions;              // x, y, width, height, area, seed_x, seed_y, id of each kept one
    // region_contours: region i's convex hull is region_contours[2 * region_contour_offsets[i] ..
    // 2 * region_contour_offsets[i + 1]), (x, y) pairs in mdx_region_hulls_dev's order (include/mdx.h)
    // (region_external: hull i belongs to regions[region_external_index[i]])
    std::vector<int32_t> region_contour_offsets;    // regions.size() / 8 + 1 entries (region_external: one per external + 1)
    std::vector<int32_t> region_contours;
    // region_outlines: region i's outer border is region_outlines[2 * region_outline_offsets[i] ..
    // 2 * region_outline_offsets[i + 1]), (x, y) pairs in mdx_region_outlines_dev's order (include/mdx.h)
    // (region_external: outline i belongs to regions[region_external_index[i]])
    std::vector<int32_t> region_outline_offsets;    // as region_contour_offsets
    std::vector<int32_t> region_outlines;
    // region_external: each kept region's parent (a component id, MDX_REGION_NO_PARENT, MDX_REGION_PARENT_UNKNOWN)
    // and the positions in `regions` of the external ones
    std::vector<int32_t> region_parent;
    std::vector<int32_t> region_external_index;
    // detect_outliers: the grid vectors' flags (bit 0 angle, bit 1 magnitude; image rows outer) and their
    // statistics; the clusters of the outlier vectors fill num_clusters, cluster_labels (per grid vector,
    // -1 for a vector that is no outlier or has no flow), kept_clusters, rectangles and
    // num_active_vectors below, as getClusters does on the live path
    std::vector<uint8_t> outlier_flags;
    mdx_outlier_stats outlier_stats{};
    // live path
    std::vector<float> outlier_points;              // fitSubspace's outlier_points, (x, y) each
    std::vector<int> subspace_columns;              // indices (into trajectories) of the winning sample
    // clusterEuclidean on outlier_points (:355), when egomotion and distance_threshold > 0
    int num_clusters = 0;                           // all clusters, kept or not
    std::vector<int32_t> cluster_labels;            // per outlier point: its cluster among all, creation order
    std::vector<int32_t> kept_clusters;             // ids of the clusters with more than 5 points
    std::vector<int32_t> rectangles;                // x, y, w, h of each kept cluster's boundingRect
    // getClusters on the vector image's grid (:375), when egomotion is off and both thresholds are > 0:
    // the four fields above are filled the same way, cluster_labels per grid vector in the reference's
    // visiting order (image rows outer), -1 for a vector without flow
    int num_active_vectors = 0;                     // grid vectors with a non-zero flow
    // cluster_contours: the convex hull of each kept cluster, in kept_clusters' order, whichever clustering
    // stage filled the fields above; hull i's vertices (x, y) are contours[2 * contour_offsets[i] ..
    // 2 * contour_offsets[i + 1]), in cv::convexHull(.., clockwise=false)'s order (include/mdx.h)
    std::vector<int32_t> contour_offsets;           // kept_clusters.size() + 1 entries
    std::vector<int32_t> contours;
};

// One processed frame's outputs (what the node hands to its publishers / logs).
struct FrameResult : StageOutputs {
    int num_vectors = 0;                       // the calculator's return value
    int w = 0, h = 0, npts = 0;
    std::vector<double> vector_image;          // h * w * 4: the node's optical_flow_vectors Mat, Vec4d per
                                               // pixel, zero where no store landed (node.cpp:81 / :98)
    // pair path
    std::vector<float> next_pts;               // 2 * npts
    std::vector<uint8_t> status;               // npts
    std::vector<uint8_t> mask;                 // h * w, thresholded |warp(gray1) - gray2|
    double H[9] = {0};
    int rc = 0;                                // MDX_OK or MDX_EDEGENERATE
    // live path
    std::vector<std::vector<float>> trajectories;   // complete ones, (x, y) * traj_size each
};

// Both paths call this before any stage runs: a FrameResult reused across frames and paths never
// carries a previous frame's stage outputs.
inline void reset_stages(FrameResult* r) { static_cast<StageOutputs&>(*r) = StageOutputs{}; }

// The Vec4d image's grid in getClusters' visiting order (flow_clusterer.cpp:180-184): rows y = 0,
// pixel_step, .. outer, columns inner, as a flat n x 4 array.
std::vector<double> grid_vectors(const std::vector<double>& vector_image, int w, int h, int pixel_step);

using Publisher = std::function<void(const std::string& topic, const Image& msg)>;

class MotionDetectionNode {
public:
    // device: HIP device of this camera stream's context (one context per stream / GPU)
    MotionDetectionNode(const Params& p, int device, int max_w, int max_h, Publisher pub);
    ~MotionDetectionNode();
    MotionDetectionNode(const MotionDetectionNode&) = delete;
    MotionDetectionNode& operator=(const MotionDetectionNode&) = delete;

    // imageCallback (node.cpp:235-455): returns true and fills *out when the frame was processed.
    bool image_callback(const Image& msg, FrameResult* out);

    // One pass of the polling caller run()'s body (node.cpp:464-529), for use_all_frames = false, where
    // imageCallback only fills the ring: returns false until image_received_; then the trajectories over the
    // ring's frames, fitSubspace(trajectories, outlier_points, 2, residual_threshold) (:494: the 2 is
    // hard-coded there, whatever num_motions says; num_motions still sizes the ring) and, with
    // distance_threshold > 0, clusterEuclidean (:497) and the kept clusters' rectangles.  With
    // use_all_frames false every frame wider than 320 px enters the device ring halved
    // (cv::resize(.., 0.5, 0.5), :470-474; mdx_ring_push_half), once, from image_callback; *out then has
    // the halved size.  With no complete trajectory (the reference indexes trajectories[0], undefined)
    // the fit and the clustering are skipped and *out carries empty lists.  There is no egomotion branch,
    // nothing is published (the markers would need the halved frame back on the host) and nothing is
    // logged.  Two passes without a new frame see the same ring and a further-advanced rand() stream, as
    // the reference's spinning loop does.
    bool run_once(FrameResult* out);

    // background_subtraction: the frame (global_frame_count() at its callback) the model last took, -1 before
    // the first; with region_min_area > 0 that frame's external regions, x, y, width, height each
    long background_frame() const { return bg_frame_; }
    const std::vector<int32_t>& background_regions() const { return bg_rects_; }

    Params& params() { return p_; }
    long global_frame_count() const { return global_frame_count_; }
    int trajectory_size() const { return p_.egomotion ? 2 * p_.num_motions + 1 : 2; }   // :241-245

private:
    void run_pair(const Image& a, const Image& b, FrameResult* r);
    void run_live(int nimg, FrameResult* r);
    void set_flow_params();
    void ring_flow(int w, int h, int nimg, FrameResult* r);
    void fit_subspace(int nimg, int num_motions, double sigma, FrameResult* r);
    void cluster_points(FrameResult* r);
    // the optional stages behind the flow; each returns at once unless its Params::*_on() holds
    void stage_detect_outliers(FrameResult* r);
    void stage_regions(FrameResult* r);
    void stage_region_records(FrameResult* r);     // the records, (region_external) parents, (region_contours) hulls
    void stage_region_outlines(FrameResult* r);    // region_outlines
    void stage_vector_clusters(FrameResult* r);
    void stage_subspace(int nimg, FrameResult* r);
    void stage_point_clusters(FrameResult* r);
    void cluster_vectors(const std::vector<double>& vectors, FrameResult* r);
    void cluster_hulls(const std::vector<float>& points, FrameResult* r);
    template <class Entry> void cluster_and_trim(const char* name, int n, FrameResult* r, Entry entry);
    void publish(const std::string& topic, const Image& img) const;
    void update_background(const Image& rgb);

    Params p_;
    Publisher pub_;
    mdx_ctx* ctx_ = nullptr;
    mdx_rand_state rng_{};
    std::deque<Image> raw_images_;
    Image last_rgb_;                          // the newest frame as rgb8 (also in the device ring)
    int ring_w_ = 0, ring_h_ = 0;             // the size the newest frame has in the device ring (halved or not)
    bool image_received_ = false;
    long global_frame_count_ = 0;
    // background_subtraction: the model, its frame size, and the device buffers of its chain (freed with ctx_)
    mdx_bg* bg_ = nullptr;
    int bg_w_ = 0, bg_h_ = 0;
    void* bg_dev_[6] = {};                    // frame, mask, labels, records, external records, counts
    long bg_frame_ = -1;
    std::vector<int32_t> bg_rects_;
};

// RGB8 renderings the node publishes, both under topic names of this build's own (kTopicMask,
// kTopicFlowMarkers), never under the reference's: the motion mask replicated to three channels
// (the new, optional mask topic of SURVEY.md §8b), and the frame with a CV_RGB(0, 0, 255) mark at
// each vector showOpticalFlowVectors would draw.  The reference's ~optical_flow_image carries
// anti-aliased arrows (optical_flow_visualizer.cpp:23-71, published at node.cpp:83-85, :101-103);
// its rendering is out of scope, so that topic is not published here ("Topics").
constexpr const char* kTopicMask = "motion_mask_image";
constexpr const char* kTopicFlowMarkers = "mdx_flow_markers_image";
Image mask_image(const std::vector<uint8_t>& mask, int w, int h);
Image flow_image(const Image& rgb, const std::vector<double>& vector_image, int pixel_step, double min_vector_size);

// On-disk formats: OpticalFlowCalculator::writeFlow / writeTrajectories
// (optical_flow_calculator.cpp:509-562) and MotionLogger (motion_logger.cpp:31-47), written with
// std::ofstream so the numbers format exactly as the reference's.
void write_flow(const std::vector<double>& vector_image, int w, int h, int pixel_step, const std::string& filename);
void write_trajectories(const std::vector<std::vector<float>>& trajectories, const std::string& filename);

class MotionLogger {
public:
    explicit MotionLogger(const std::string& path) : out_(path) {}
    void write_contour(const std::vector<int>& xy, int frame_number, int contour_id);
    void write_bounding_box(int x, int y, int width, int height, int frame_number, int contour_id);

private:
    std::ofstream out_;
};

}  // namespace mdx_host

#endif  // MDX_HOST_H_
