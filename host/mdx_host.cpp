// mdx_host.cpp -- see mdx_host.h.  Reference sites cited per function.
#include "mdx_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <stdexcept>

namespace mdx_host {

Image to_rgb8(const Image& msg)
{
    int cn;
    if (msg.encoding == "mono8") cn = 1;
    else if (msg.encoding == "rgb8" || msg.encoding == "bgr8") cn = 3;
    else throw std::invalid_argument("unsupported encoding " + msg.encoding);
    if (msg.step < msg.width * (uint32_t)cn || msg.data.size() < (size_t)msg.step * msg.height)
        throw std::invalid_argument("image buffer smaller than step * height");
    Image out;
    out.height = msg.height;
    out.width = msg.width;
    out.encoding = "rgb8";
    out.step = 3 * msg.width;
    out.data.resize((size_t)out.step * out.height);
    for (uint32_t y = 0; y < msg.height; y++) {
        const uint8_t* s = msg.data.data() + (size_t)y * msg.step;
        uint8_t* d = out.data.data() + (size_t)y * out.step;
        for (uint32_t x = 0; x < msg.width; x++) {
            if (cn == 1) {
                d[3 * x] = d[3 * x + 1] = d[3 * x + 2] = s[x];
            } else if (msg.encoding == "bgr8") {
                d[3 * x] = s[3 * x + 2];
                d[3 * x + 1] = s[3 * x + 1];
                d[3 * x + 2] = s[3 * x];
            } else {
                d[3 * x] = s[3 * x];
                d[3 * x + 1] = s[3 * x + 1];
                d[3 * x + 2] = s[3 * x + 2];
            }
        }
    }
    return out;
}

MotionDetectionNode::MotionDetectionNode(const Params& p, int device, int max_w, int max_h, Publisher pub)
    : p_(p), pub_(std::move(pub))
{
    // the library must match the header this node was built against (ABI 4)
    if (mdx_abi_version() != MDX_ABI_VERSION || mdx_params_size() != sizeof(mdx_params))
        throw std::runtime_error("libmdx.so does not match include/mdx.h (ABI / mdx_params size)");
    mdx_params mp;
    mdx_default_params(&mp);
    mp.pixel_step = p_.pixel_step;
    mp.min_vector_size = p_.min_vector_size;
    mp.subspace_precision = p_.subspace_precision;
    ctx_ = mdx_create(device, max_w, max_h, 1, &mp);
    if (!ctx_) throw std::runtime_error(std::string("mdx_create: ") + mdx_create_error());
    mdx_srand(&rng_, p_.seed);
}

MotionDetectionNode::~MotionDetectionNode()
{
    if (ctx_) mdx_destroy(ctx_);
}

void MotionDetectionNode::publish(const std::string& topic, const Image& img) const
{
    if (pub_) pub_(topic, img);
}

// imageCallback (node.cpp:235-455): the frame counter advances on every call -- on a skipped
// frame at :247, on a kept one at :454 (or :315 when no trajectory survives).
bool MotionDetectionNode::image_callback(const Image& msg, FrameResult* out)
{
    const int skip = p_.skip_frames > 0 ? p_.skip_frames : 1;
    if (global_frame_count_ % skip != 0) {
        global_frame_count_++;
        return false;
    }
    const size_t ts = (size_t)trajectory_size();
    if (raw_images_.size() < ts) {                               // :248-261
        raw_images_.push_back(msg);
        if (raw_images_.size() == ts) image_received_ = true;
    } else {
        raw_images_.push_back(msg);
        raw_images_.pop_front();
        image_received_ = true;
    }
    if (p_.ring_on()) {
        // the device ring mirrors raw_images_: this frame is converted, uploaded and pyramided once
        // (the reference re-converts every ring frame on every callback, :266-287, and on every pass
        // of run(), :464-480); the polling caller's frames wider than 320 px enter halved (:470-474)
        last_rgb_ = to_rgb8(msg);
        const bool half = !p_.use_all_frames && last_rgb_.width > 320;
        ring_w_ = (int)last_rgb_.width;
        ring_h_ = (int)last_rgb_.height;
        if (half && mdx_half_size(ring_w_, ring_h_, &ring_w_, &ring_h_) != MDX_OK)
            throw std::invalid_argument("frame too small to halve");
        const int rc = (half ? mdx_ring_push_half : mdx_ring_push)(ctx_, last_rgb_.data.data(), (int)last_rgb_.width,
                                                                   (int)last_rgb_.height, (int)last_rgb_.step,
                                                                   MDX_FMT_RGB8, (int)raw_images_.size());
        if (rc < 0) throw std::runtime_error(std::string("mdx_ring_push: ") + mdx_last_error(ctx_));
    }
    if (p_.background_subtraction) update_background(p_.ring_on() ? last_rgb_ : to_rgb8(msg));
    bool done = false;
    if (p_.use_all_frames && image_received_) {                  // :262
        set_flow_params();
        FrameResult local;
        FrameResult* r = out ? out : &local;
        if (p_.live_path) {
            run_live((int)raw_images_.size(), r);
        } else {
            // toCvCopy(*iter, "rgb8") (:271) of the two frames the pair path reads
            run_pair(to_rgb8(raw_images_[raw_images_.size() - 2]), to_rgb8(raw_images_.back()), r);
        }
        done = true;
    }
    global_frame_count_++;
    return done;
}

// background_subtraction: the frame updates the mixture model (BackgroundSubtractor::getMotionContours,
// background_subtractor.cpp:27); with region_min_area > 0 its mask is opened and labelled and the external
// records picked (:31-35), all on the device: the frame goes up, the records come back.
void MotionDetectionNode::update_background(const Image& rgb)
{
    const int w = (int)rgb.width, h = (int)rgb.height;
    auto check = [&](int rc, const char* what) {
        if (rc < 0) throw std::runtime_error(std::string(what) + ": " + mdx_last_error(ctx_));
    };
    const size_t n = (size_t)w * h, cap = (size_t)((w + 1) / 2) * ((h + 1) / 2);
    if (!bg_ || w != bg_w_ || h != bg_h_) {          // a new frame size starts a new model
        check(mdx_sync(ctx_), "mdx_sync");
        if (bg_) check(mdx_bg_destroy(ctx_, bg_), "mdx_bg_destroy");
        bg_ = nullptr;
        for (void*& d : bg_dev_) {
            if (d) mdx_dev_free(ctx_, d);
            d = nullptr;
        }
        check(mdx_bg_create(ctx_, 1, w, h, 3, nullptr, &bg_), "mdx_bg_create");
        const size_t bytes[6] = {n * 3, n, n * 4, cap * sizeof(mdx_region), cap * sizeof(mdx_region), 16};
        for (int i = 0; i < 6; i++)
            if (!(bg_dev_[i] = mdx_dev_alloc(ctx_, bytes[i]))) throw std::runtime_error("mdx_dev_alloc failed");
        bg_w_ = w, bg_h_ = h;
    }
    uint8_t* d_frame = static_cast<uint8_t*>(bg_dev_[0]);
    uint8_t* d_mask = static_cast<uint8_t*>(bg_dev_[1]);
    if (rgb.step == 3u * rgb.width) {
        check(mdx_memcpy_h2d(ctx_, d_frame, rgb.data.data(), n * 3), "mdx_memcpy_h2d");
    } else {
        for (int y = 0; y < h; y++)
            check(mdx_memcpy_h2d(ctx_, d_frame + (size_t)y * w * 3, rgb.data.data() + (size_t)y * rgb.step, (size_t)w * 3),
                  "mdx_memcpy_h2d");
    }
    check(mdx_bg_apply_dev(ctx_, bg_, 1, d_frame, w * 3, n * 3, 0, -1.0, d_mask), "mdx_bg_apply_dev");
    bg_frame_ = global_frame_count_;
    bg_rects_.clear();
    if (p_.region_min_area <= 0) return;
    int32_t* d_labels = static_cast<int32_t*>(bg_dev_[2]);
    mdx_region* d_rec = static_cast<mdx_region*>(bg_dev_[3]);
    mdx_region* d_ext = static_cast<mdx_region*>(bg_dev_[4]);
    int32_t* d_cnt = static_cast<int32_t*>(bg_dev_[5]);     // num_all, num_kept, num_external
    check(mdx_mask_regions_dev(ctx_, 1, d_mask, w, h, w, n, MDX_REGIONS_OPEN3, p_.region_min_area, d_rec, (int)cap, d_cnt,
                               d_cnt + 1, d_labels, nullptr),
          "mdx_mask_regions_dev");
    check(mdx_region_parents_dev(ctx_, 1, d_labels, w, h, d_rec, (int)cap, d_cnt + 1, nullptr, d_ext, d_cnt + 2),
          "mdx_region_parents_dev");
    int32_t cnt[3] = {0, 0, 0};
    check(mdx_memcpy_d2h(ctx_, cnt, d_cnt, sizeof cnt), "mdx_memcpy_d2h");
    check(mdx_sync(ctx_), "mdx_sync");
    const size_t next = std::min((size_t)std::max(cnt[2], 0), cap);
    std::vector<mdx_region> ext(next);
    if (next) {
        check(mdx_memcpy_d2h(ctx_, ext.data(), d_ext, next * sizeof(mdx_region)), "mdx_memcpy_d2h");
        check(mdx_sync(ctx_), "mdx_sync");
    }
    for (const mdx_region& e : ext) bg_rects_.insert(bg_rects_.end(), {e.x, e.y, e.width, e.height});
}

// pixel_step and min_vector_size are re-read on every frame (:264) and every pass of run()
void MotionDetectionNode::set_flow_params()
{
    mdx_params mp;
    mdx_get_params(ctx_, &mp);
    mp.pixel_step = p_.pixel_step;
    mp.min_vector_size = p_.min_vector_size;
    if (mdx_set_params(ctx_, &mp) != MDX_OK) throw std::runtime_error(mdx_last_error(ctx_));
}

// run() (node.cpp:457-553), one pass of its body
bool MotionDetectionNode::run_once(FrameResult* out)
{
    if (!image_received_) return false;                          // :459
    if (p_.use_all_frames || !p_.ring_on()) throw std::logic_error("run_once needs use_all_frames = false");
    set_flow_params();
    FrameResult local;
    FrameResult* r = out ? out : &local;
    reset_stages(r);
    ring_flow(ring_w_, ring_h_, (int)raw_images_.size(), r);     // :488
    if (r->trajectories.empty()) return true;                    // (the reference reads trajectories[0] here)
    fit_subspace((int)raw_images_.size(), 2, p_.residual_threshold, r);   // :494
    if (p_.run_clusters_on()) cluster_points(r);                 // :497
    return true;
}

// runOpticalFlow (node.cpp:76-92) -> calculateOpticalFlow (optical_flow_calculator.cpp:30-130)
void MotionDetectionNode::run_pair(const Image& a, const Image& b, FrameResult* r)
{
    const int w = (int)a.width, h = (int)a.height, ps = p_.pixel_step;
    if (b.width != a.width || b.height != a.height) throw std::invalid_argument("frame sizes differ");
    reset_stages(r);
    const int npts = mdx_grid_count(w, h, ps), ny = (h + ps - 1) / ps;
    r->w = w;
    r->h = h;
    r->npts = npts;
    r->next_pts.assign((size_t)2 * npts, 0.f);
    r->status.assign(npts, 0);
    r->mask.assign((size_t)w * h, 0);
    std::vector<double> vec((size_t)4 * npts);
    r->rc = mdx_flow_warp_diff(ctx_, a.data.data(), b.data.data(), w, h, (int)a.step, MDX_FMT_RGB8, r->next_pts.data(),
                               r->status.data(), vec.data(), r->mask.data(), r->H, nullptr, &r->num_vectors);
    if (r->rc < 0) throw std::runtime_error(std::string("mdx_flow_warp_diff: ") + mdx_last_error(ctx_));
    // optical_flow_vectors = zeros(rows, cols) (:81), the calculator's Vec4d at each grid point
    r->vector_image.assign((size_t)w * h * 4, 0.0);
    for (int k = 0; k < npts; k++) {
        const int x = (k / ny) * ps, y = (k % ny) * ps;          // x-major grid (:56-64)
        std::memcpy(&r->vector_image[((size_t)y * w + x) * 4], &vec[(size_t)4 * k], 32);
    }
    publish(kTopicFlowMarkers, flow_image(a, r->vector_image, ps, p_.min_vector_size));   // (not :83-85's arrows)
    publish(kTopicMask, mask_image(r->mask, w, h));
    stage_detect_outliers(r);
    stage_regions(r);
}

// detectOutliers (node.cpp:112-160): findOutliers (:114), getOutlierVectors (:121) and getClusters (:127)
// on the Vec4d image's grid
void MotionDetectionNode::stage_detect_outliers(FrameResult* r)
{
    if (!p_.detect_outliers_on()) return;
    r->grid = grid_vectors(r->vector_image, r->w, r->h, p_.pixel_step);
    const int n = (int)(r->grid.size() / 4);
    std::vector<double> outl(r->grid.size());
    r->outlier_flags.assign(n, 0);
    const int rc = mdx_find_outliers(ctx_, r->grid.data(), 1, n, p_.include_zeros ? MDX_OUTLIERS_INCLUDE_ZEROS : 0,
                                     r->outlier_flags.data(), outl.data(), &r->outlier_stats);
    if (rc < 0) throw std::runtime_error(std::string("mdx_find_outliers: ") + mdx_last_error(ctx_));
    cluster_vectors(outl, r);
}

// the mask labelled into regions (getMotionContours' recipe, background_subtractor.cpp:31-35)
void MotionDetectionNode::stage_regions(FrameResult* r)
{
    if (!p_.regions_on()) return;
    stage_region_records(r);
    if (p_.region_outlines) stage_region_outlines(r);
}

void MotionDetectionNode::stage_region_records(FrameResult* r)
{
    const int w = r->w, h = r->h;
    // a kept region has at least region_min_area pixels
    static_assert(sizeof(mdx_region) == 8 * sizeof(int32_t), "mdx_region is eight int32");
    const int cap = (int)std::min<long long>((long long)w * h / p_.region_min_area, (long long)((w + 1) / 2) * ((h + 1) / 2));
    int nkept = 0;
    r->regions.assign((size_t)8 * cap, 0);
    const int flags = p_.region_open ? MDX_REGIONS_OPEN3 : 0;
    mdx_region* recs = reinterpret_cast<mdx_region*>(r->regions.data());
    if (p_.region_external) {
        // the records, their parents and (region_contours) the hulls of the external ones in one call
        const int maxv = p_.region_contours ? (int)std::min<long long>((long long)w * h, 2ll * std::min(w, h) * cap) : 0;
        int total = 0, next = 0;
        r->region_parent.assign((size_t)cap, 0);
        r->region_external_index.assign((size_t)cap, 0);
        if (p_.region_contours) {
            r->region_contour_offsets.assign((size_t)cap + 1, 0);
            r->region_contours.resize((size_t)2 * maxv);
        }
        const int rc = mdx_mask_regions_tree(ctx_, r->mask.data(), w, h, w, flags, p_.region_min_area, recs, cap,
                                             &r->num_regions_all, &nkept, r->region_parent.data(),
                                             r->region_external_index.data(), &next,
                                             p_.region_contours ? r->region_contour_offsets.data() : nullptr,
                                             r->region_contours.data(), maxv, &total);
        if (rc < 0) throw std::runtime_error(std::string("mdx_mask_regions_tree: ") + mdx_last_error(ctx_));
        const int n = std::min(nkept, cap);
        r->regions.resize((size_t)8 * n);
        r->region_parent.resize((size_t)n);
        r->region_external_index.resize((size_t)next);
        if (p_.region_contours) {
            r->region_contour_offsets.resize((size_t)next + 1);
            r->region_contours.resize((size_t)2 * std::min(total, maxv));
        }
        return;
    }
    if (!p_.region_contours) {
        const int rc = mdx_mask_regions(ctx_, r->mask.data(), w, h, w, flags, p_.region_min_area, recs, cap,
                                        &r->num_regions_all, &nkept, nullptr, nullptr);
        if (rc < 0) throw std::runtime_error(std::string("mdx_mask_regions: ") + mdx_last_error(ctx_));
        r->regions.resize((size_t)8 * std::min(nkept, cap));
        return;
    }
    // the records and their convex hulls in one call; every hull of `cap` regions fits maxv vertices
    const int maxv = (int)std::min<long long>((long long)w * h, 2ll * std::min(w, h) * cap);
    int total = 0;
    r->region_contour_offsets.assign((size_t)cap + 1, 0);
    r->region_contours.resize((size_t)2 * maxv);
    const int rc = mdx_mask_region_hulls(ctx_, r->mask.data(), w, h, w, flags, p_.region_min_area, recs, cap,
                                         &r->num_regions_all, &nkept, r->region_contour_offsets.data(),
                                         r->region_contours.data(), maxv, &total);
    if (rc < 0) throw std::runtime_error(std::string("mdx_mask_region_hulls: ") + mdx_last_error(ctx_));
    const int n = std::min(nkept, cap);
    r->regions.resize((size_t)8 * n);
    r->region_contour_offsets.resize((size_t)n + 1);
    r->region_contours.resize((size_t)2 * std::min(total, maxv));
}

// region_outlines: the outer border polyline of every kept (region_external: external) record, a call of its
// own behind the records'; the points' number is the image's, so a first guess may need a second call
void MotionDetectionNode::stage_region_outlines(FrameResult* r)
{
    const int w = r->w, h = r->h;
    const int cap = (int)std::min<long long>((long long)w * h / p_.region_min_area, (long long)((w + 1) / 2) * ((h + 1) / 2));
    const int flags = p_.region_open ? MDX_REGIONS_OPEN3 : 0;
    std::vector<int32_t> recs((size_t)8 * cap), parent, index;
    if (p_.region_external) {
        parent.assign((size_t)cap, 0);
        index.assign((size_t)cap, 0);
    }
    int maxp = std::max(4096, w * h / 4), total = 0, nall = 0, nkept = 0, next = 0;
    for (;;) {
        r->region_outline_offsets.assign((size_t)cap + 1, 0);
        r->region_outlines.resize((size_t)2 * maxp);
        const int rc = mdx_mask_region_outlines(ctx_, r->mask.data(), w, h, w, flags, p_.region_min_area,
                                                reinterpret_cast<mdx_region*>(recs.data()), cap, &nall, &nkept,
                                                p_.region_external ? parent.data() : nullptr,
                                                p_.region_external ? index.data() : nullptr,
                                                p_.region_external ? &next : nullptr, r->region_outline_offsets.data(),
                                                r->region_outlines.data(), maxp, &total);
        if (rc < 0) throw std::runtime_error(std::string("mdx_mask_region_outlines: ") + mdx_last_error(ctx_));
        if (total <= maxp) break;
        maxp = total;
    }
    r->region_outline_offsets.resize((size_t)(p_.region_external ? next : std::min(nkept, cap)) + 1);
    r->region_outlines.resize((size_t)2 * total);
}

// One clustering entry's call and trim: the result vectors sized for n members and max_kept = n / 6 clusters (a
// kept one has more than 5 members), entry(max_kept, &nkept) called, its error thrown under `name`, then the trim
template <class Entry> void MotionDetectionNode::cluster_and_trim(const char* name, int n, FrameResult* r, Entry entry)
{
    const int max_kept = n / 6;
    int nkept = 0;
    r->cluster_labels.assign(n, 0);
    r->kept_clusters.assign(max_kept, 0);
    r->rectangles.assign((size_t)4 * max_kept, 0);
    if (entry(max_kept, &nkept) < 0) throw std::runtime_error(std::string(name) + ": " + mdx_last_error(ctx_));
    r->kept_clusters.resize(nkept);
    r->rectangles.resize((size_t)4 * nkept);
}

// getClusters (flow_clusterer.cpp:178-227) on n x 4 vectors in its visiting order
void MotionDetectionNode::cluster_vectors(const std::vector<double>& vectors, FrameResult* r)
{
    const int n = (int)(vectors.size() / 4);
    cluster_and_trim("mdx_cluster_vectors", n, r, [&](int max_kept, int* nkept) {
        return mdx_cluster_vectors(ctx_, vectors.data(), n, p_.distance_threshold, p_.angular_threshold, 5,
                                   p_.abs_int ? MDX_VCLUSTER_ABS_INT : 0, r->cluster_labels.data(),
                                   &r->num_active_vectors, &r->num_clusters, r->kept_clusters.data(),
                                   r->rectangles.data(), max_kept, nkept);
    });
    if (!p_.cluster_contours) return;
    std::vector<float> pts((size_t)2 * n);                      // cv::Point2f(vec[0], vec[1]) (node.cpp:382)
    for (int i = 0; i < n; i++) pts[2 * i] = (float)vectors[4 * (size_t)i], pts[2 * i + 1] = (float)vectors[4 * (size_t)i + 1];
    cluster_hulls(pts, r);
}

// showClusterContours' cv::convexHull of every kept cluster (optical_flow_visualizer.cpp:204-221) of the
// clustering that has just filled r's labels and kept ids; points: one (x, y) per label
void MotionDetectionNode::cluster_hulls(const std::vector<float>& points, FrameResult* r)
{
    const int n = (int)r->cluster_labels.size(), k = (int)r->kept_clusters.size();
    int total = 0;
    r->contour_offsets.assign((size_t)k + 1, 0);
    r->contours.assign((size_t)2 * n, 0);                       // a hull has at most as many vertices as members
    const int rc = mdx_cluster_hulls(ctx_, points.data(), r->cluster_labels.data(), n, r->kept_clusters.data(), k,
                                     r->contour_offsets.data(), r->contours.data(), n, &total);
    if (rc < 0) throw std::runtime_error(std::string("mdx_cluster_hulls: ") + mdx_last_error(ctx_));
    r->contours.resize((size_t)2 * total);
}

// runOpticalFlowTrajectory (node.cpp:94-110) over the nimg ring frames already on the device, and,
// with egomotion, fitSubspace (:341-348)
void MotionDetectionNode::run_live(int nimg, FrameResult* r)
{
    reset_stages(r);
    ring_flow((int)last_rgb_.width, (int)last_rgb_.height, nimg, r);
    publish(kTopicFlowMarkers, flow_image(last_rgb_, r->vector_image, p_.pixel_step, p_.min_vector_size));   // (not :101-103's arrows)
    if (r->trajectories.empty()) return;                        // :296-318
    stage_vector_clusters(r);
    stage_subspace(nimg, r);
    stage_point_clusters(r);
}

// calculateOpticalFlowTrajectory over the device ring's nimg frames of w x h: the vector image and the
// complete trajectories
void MotionDetectionNode::ring_flow(int w, int h, int nimg, FrameResult* r)
{
    const int ps = p_.pixel_step;
    for (const Image& m : raw_images_)
        if (m.width != last_rgb_.width || m.height != last_rgb_.height) throw std::invalid_argument("frame sizes differ");
    const int npts = mdx_grid_count(w, h, ps);
    r->w = w;
    r->h = h;
    r->npts = npts;
    std::vector<float> traj((size_t)npts * nimg * 2), start((size_t)npts * 2);
    std::vector<int32_t> tlen(npts);
    std::vector<double> vec((size_t)npts * 4);
    const int rc = mdx_ring_trajectory(ctx_, traj.data(), tlen.data(), start.data(), vec.data(), &r->num_vectors);
    if (rc < 0) throw std::runtime_error(std::string("mdx_ring_trajectory: ") + mdx_last_error(ctx_));
    // optical_flow_vectors = zeros (:98); the last pass stores each point's Vec4d at
    // ((int)y, (int)x) of its position entering that pass, in point order
    r->vector_image.assign((size_t)w * h * 4, 0.0);
    for (int k = 0; k < npts; k++) {
        const int x = (int)start[2 * k], y = (int)start[2 * k + 1];
        if (x >= 0 && x < w && y >= 0 && y < h) std::memcpy(&r->vector_image[((size_t)y * w + x) * 4], &vec[4 * k], 32);
    }
    r->trajectories.clear();
    for (int k = 0; k < npts; k++)                              // full-length ones only (:244-249)
        if (tlen[k] == nimg) r->trajectories.emplace_back(&traj[(size_t)k * nimg * 2], &traj[(size_t)(k + 1) * nimg * 2]);
}

// without egomotion (:357-389): getClusters(optical_flow_vectors, pixel_step, distance_threshold,
// angular_threshold) (:375) on the Vec4d image's grid
void MotionDetectionNode::stage_vector_clusters(FrameResult* r)
{
    if (!p_.vector_clusters_on()) return;
    r->grid = grid_vectors(r->vector_image, r->w, r->h, p_.pixel_step);
    cluster_vectors(r->grid, r);
}

// fitSubspace on the complete trajectories (:341-348), one rand() stream across frames
void MotionDetectionNode::stage_subspace(int nimg, FrameResult* r)
{
    if (p_.subspace_on()) fit_subspace(nimg, p_.num_motions, p_.sigma, r);
}

void MotionDetectionNode::fit_subspace(int nimg, int num_motions, double sigma, FrameResult* r)
{
    const int nt = (int)r->trajectories.size(), d = 4 * num_motions;
    std::vector<float> flat((size_t)nt * nimg * 2);
    for (int i = 0; i < nt; i++) std::memcpy(&flat[(size_t)i * nimg * 2], r->trajectories[i].data(), (size_t)nimg * 8);
    std::vector<int> cols(d);
    std::vector<float> outl((size_t)nt * 2);
    int nout = 0;
    const int rc = mdx_fit_subspace(ctx_, flat.data(), nt, nimg, num_motions, sigma, &rng_, cols.data(), nullptr,
                                    nullptr, outl.data(), &nout);
    if (rc < 0) throw std::runtime_error(std::string("mdx_fit_subspace: ") + mdx_last_error(ctx_));
    r->outlier_points.assign(outl.begin(), outl.begin() + 2 * nout);
    for (int c : cols)
        if (c >= 0) r->subspace_columns.push_back(c);
}

// clusterEuclidean(outlier_points, distance_threshold) (:355) and each kept cluster's boundingRect
// (optical_flow_visualizer.cpp:230-236)
void MotionDetectionNode::stage_point_clusters(FrameResult* r)
{
    if (p_.point_clusters_on()) cluster_points(r);
}

void MotionDetectionNode::cluster_points(FrameResult* r)
{
    const int nout = (int)(r->outlier_points.size() / 2);
    cluster_and_trim("mdx_cluster_euclidean", nout, r, [&](int max_kept, int* nkept) {
        return mdx_cluster_euclidean(ctx_, r->outlier_points.data(), nout, p_.distance_threshold, 5,
                                     r->cluster_labels.data(), &r->num_clusters, r->kept_clusters.data(),
                                     r->rectangles.data(), max_kept, nkept);
    });
    if (p_.cluster_contours) cluster_hulls(r->outlier_points, r);
}

std::vector<double> grid_vectors(const std::vector<double>& vi, int w, int h, int ps)
{
    std::vector<double> grid;
    for (int y = 0; y < h; y += ps)
        for (int x = 0; x < w; x += ps) {
            const double* e = &vi[((size_t)y * w + x) * 4];
            grid.insert(grid.end(), e, e + 4);
        }
    return grid;
}

Image mask_image(const std::vector<uint8_t>& mask, int w, int h)
{
    Image im;
    im.width = w;
    im.height = h;
    im.encoding = "rgb8";                                      // publishImage's encoding (:220)
    im.step = 3 * w;
    im.data.resize((size_t)3 * w * h);
    for (size_t i = 0; i < (size_t)w * h; i++) im.data[3 * i] = im.data[3 * i + 1] = im.data[3 * i + 2] = mask[i];
    return im;
}

Image flow_image(const Image& rgb, const std::vector<double>& vi, int pixel_step, double mvs)
{
    Image im = rgb;
    const int w = (int)rgb.width, h = (int)rgb.height;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const double* e = &vi[((size_t)y * w + x) * 4];
            // the vectors showOpticalFlowVectors draws (optical_flow_visualizer.cpp:37)
            if ((std::fabs(e[2]) > mvs || std::fabs(e[3]) > mvs) && std::fabs(e[2]) < pixel_step * 5 &&
                std::fabs(e[3]) < pixel_step * 5) {
                const int sx = (int)e[0], sy = (int)e[1];
                if (sx < 0 || sx >= w || sy < 0 || sy >= h) continue;
                uint8_t* p = &im.data[(size_t)sy * im.step + 3 * (size_t)sx];
                p[0] = 0;
                p[1] = 0;
                p[2] = 255;                                    // CV_RGB(0, 0, 255) in an rgb8 image
            }
        }
    return im;
}

// writeFlow (optical_flow_calculator.cpp:509-541): grid rows i = 0, ps, .. and columns j = 0, ps, ..
// of the Vec4d image; a lost point (x == -1) writes 0.0
void write_flow(const std::vector<double>& vi, int w, int h, int ps, const std::string& filename)
{
    std::ofstream hf(filename + "_h"), vf(filename + "_f");
    for (int i = 0; i < h; i += ps) {
        for (int j = 0; j < w; j += ps) {
            if (j) {
                hf << ", ";
                vf << ", ";
            }
            const double* e = &vi[((size_t)i * w + j) * 4];
            if (e[0] == -1.0) {
                hf << 0.0;
                vf << 0.0;
            } else {
                hf << e[2];
                vf << e[3];
            }
        }
        hf << std::endl;
        vf << std::endl;
    }
}

// writeTrajectories (:543-562): "x0, y0, x1, y1, ..." per trajectory, float32 values
void write_trajectories(const std::vector<std::vector<float>>& trajectories, const std::string& filename)
{
    std::ofstream tf(filename);
    for (const auto& t : trajectories) {
        for (size_t j = 0; j + 1 < t.size(); j += 2) {
            if (j) tf << ", ";
            tf << t[j] << ", " << t[j + 1];
        }
        tf << std::endl;
    }
}

// MotionLogger::writeContour / writeBoundingBox (motion_logger.cpp:31-47); cv::Rect br() = tl + size
void MotionLogger::write_contour(const std::vector<int>& xy, int frame_number, int contour_id)
{
    out_ << frame_number << ", " << contour_id;
    for (size_t i = 0; i + 1 < xy.size(); i += 2) out_ << ", " << xy[i] << ", " << xy[i + 1];
    out_ << std::endl;
}

void MotionLogger::write_bounding_box(int x, int y, int width, int height, int frame_number, int contour_id)
{
    out_ << frame_number << ", " << contour_id << ", " << x << ", " << y << ", " << x + width << ", " << y + height
         << std::endl;
}

}  // namespace mdx_host
