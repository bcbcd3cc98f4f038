// mdx_node -- drives mdx_host::MotionDetectionNode (C++, over libmdx.so) from a recorded frame stream,
// the way ros::spin delivers ~input_image to imageCallback (node.cpp:63, :575).
//
//   mdx_node <frames.bin> <outdir> [pixel_step=10] [min_vector_size=1.0] [skip_frames=1]
//            [num_motions=2] [egomotion=1] [live_path=1] [sigma=0.5] [seed=1] [device=0]
//            [subspace_precision=0]   (0 double, 1 the reference's float arithmetic shape)
//            [distance_threshold=0]   (clusterEuclidean's threshold; 0: no clustering)
//            [angular_threshold=0]    (egomotion=0: getClusters' angular threshold; with distance_threshold
//                                      > 0 too, the flow vectors are clustered by distance and angle; 0: off)
//            [abs_int=0]              (getClusters: truncate the angular distance, the reference's int abs)
//            [log_contours=0]
//            [region_min_area=0]      (pair path: label the mask into regions of at least this area; 0: off)
//            [region_open=1]          (the 3x3 opening in front of the labelling)
//            [detect_outliers=0]      (pair path with both thresholds > 0: flag the flow vectors' median / MAD
//                                      outliers and cluster them by distance and angle)
//            [include_zeros=0]        (findOutliers: vectors without flow take part in the statistics)
//            [use_all_frames=1]       (0: the polling caller run() (node.cpp:457-553) instead of imageCallback's
//                                      body: the callback only fills the ring, every frame wider than 320 px
//                                      entering it halved on the device (:470-474), and run_once() is called once
//                                      after every delivered frame, a deterministic stand-in for the polling loop)
//            [residual_threshold=0.2] (use_all_frames=0: fitSubspace's threshold (:491); its num_motions is 2 there)
//            [cluster_contours=0]     (the convex hull of every kept cluster, showClusterContours' (:393, :510),
//                                      behind each clustering stage that ran)
//            [region_contours=0]      (pair path with region_min_area > 0: the convex hull of every kept region)
//            [region_external=0]      (pair path with region_min_area > 0: findContours' RETR_EXTERNAL -- each kept
//                                      region's parent blob; rectangles and hulls of the external regions only)
//            [region_outlines=0]      (pair path with region_min_area > 0: the outer border polyline of every kept
//                                      region, findContours' own point list; with region_external=1 of the external ones)
//            [background_subtraction=0] (every frame that enters the ring also updates a MOG2 background model on the
//                                      device; with region_min_area > 0 the external regions of its opened mask go to
//                                      motion_bg.log, one MotionLogger::writeBoundingBox line each)
//
// frames.bin: "MDXF", u32 count, then per frame u32 height, u32 width, u32 step, u32 len, the
// encoding (len bytes) and step * height data bytes (a sensor_msgs/Image each).
// For the k-th processed frame (use_all_frames=0: the k-th run_once() that processed, which writes what a
// live frame writes -- res, flow, traj and, with distance_threshold > 0, clusters -- at the size the frames
// have in the ring, publishes nothing and logs nothing) it writes to <outdir>:
//   pub_<k>_<topic>.rgb8          every published image (raw RGB8, step 3 * width)
//   res_<k>.bin                   i32 num_vectors, rc, w, h, npts, ntraj, traj_len, nout; f64 H[9];
//                                 pair: f32 next_pts[2 npts], u8 status[npts], u8 mask[w h];
//                                 live: f32 trajectories[ntraj][traj_len][2], f32 outliers[nout][2],
//                                 i32 ncols, i32 columns[ncols]
//   flow_<k>_h, flow_<k>_f        writeFlow of the node's vector image (optical_flow_calculator.cpp:509)
//   traj_<k>                      writeTrajectories (live path, :543)
//   clusters_<k>.bin              live path with egomotion and distance_threshold > 0: i32 num_all,
//                                 num_kept; i32 labels[nout]; i32 kept[num_kept]; i32 rects[num_kept][4]
//                                 (x, y, width, height)
//   vclusters_<k>.bin             live path with egomotion=0 and both thresholds > 0: i32 n (grid vectors,
//                                 image rows outer), num_active, num_all, num_kept; f64 vectors[n][4] (the
//                                 grid of the node's vector image as getClusters visits it); i32 labels[n]
//                                 (-1: no flow); i32 kept[num_kept]; i32 rects[num_kept][4] (x, y, width,
//                                 height); with log_contours=1 each rectangle goes to motion.log too
//   outliers_<k>.bin              pair path with detect_outliers=1 and both thresholds > 0: i32 n (grid vectors,
//                                 image rows outer), selected, flagged_angle, flagged_magnitude, outliers,
//                                 num_active (outlier vectors with a flow), num_all, num_kept; f64
//                                 median_angle, mad_angle, median_magnitude, mad_magnitude; f64
//                                 vectors[n][4] (the grid of the node's vector image); u8 flags[n] (bit 0
//                                 angle, bit 1 magnitude); i32 labels[n] (getClusters on the outlier vectors;
//                                 -1: no outlier, or no flow); i32 kept[num_kept]; i32 rects[num_kept][4] (x,
//                                 y, width, height); with log_contours=1 each rectangle goes to motion.log too
//   regions_<k>.bin               pair path with region_min_area > 0: i32 num_all, num_kept; i32
//                                 records[num_kept][8] (x, y, width, height, area, seed_x, seed_y, id);
//                                 with log_contours=1 each record's rectangle goes to motion.log too
//   region_hulls_<k>.bin          the same with region_contours=1: i32 k (the records of regions_<k>.bin); i32
//                                 offsets[k + 1]; i32 xy[offsets[k]][2] -- record i's convex hull is
//                                 xy[offsets[i] .. offsets[i + 1]), in mdx_region_hulls_dev's order (include/mdx.h);
//                                 with log_contours=1 each hull goes to motion.log too (writeContour), behind
//                                 the frame's region rectangles.  With region_external=1 the hulls (and k)
//                                 are those of the external records, hull i belonging to record
//                                 external_index[i] of region_parents_<k>.bin, and so are the rectangles and
//                                 hulls that go to motion.log, numbered among the external records
//   region_outlines_<k>.bin       the same with region_outlines=1, in region_hulls_<k>.bin's layout: i32 k; i32
//                                 offsets[k + 1]; i32 xy[offsets[k]][2] -- record i's outer border is
//                                 xy[offsets[i] .. offsets[i + 1]), in mdx_region_outlines_dev's order
//                                 (include/mdx.h); with log_contours=1 each outline goes to motion.log too
//                                 (writeContour), behind the frame's hull lines.  With region_external=1 they
//                                 are those of the external records, as the hulls
//   region_parents_<k>.bin        the same with region_external=1: i32 k (the records of regions_<k>.bin); i32
//                                 parent[k] (a component id, -1: external, -2: unknown; include/mdx.h
//                                 mdx_region_parents_dev); i32 num_external; i32 external_index[num_external]
//                                 (positions in the records of the external ones)
//   motion.log                   log_contours=1: created at start; MotionLogger::writeBoundingBox of
//                                 every kept cluster's rectangle (node.cpp:431-434), "frame, id, tl.x,
//                                 tl.y, br.x, br.y" with frame = the node's global_frame_count_ during
//                                 that callback and id the index among the kept clusters; with
//                                 cluster_contours=1, behind a frame's rectangle lines,
//                                 MotionLogger::writeContour of every kept cluster's hull (:426-429), "frame,
//                                 id, x, y, x, y, ..."
// With cluster_contours=1 every cluster file (clusters, vclusters, outliers) ends in the hulls of its kept
// clusters, behind the rectangles: i32 offsets[num_kept + 1]; i32 xy[offsets[num_kept]][2] -- hull i's
// vertices are xy[offsets[i] .. offsets[i + 1]), in cv::convexHull(.., clockwise=false)'s order (include/mdx.h).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "mdx_host.h"

using namespace mdx_host;

static std::vector<Image> read_frames(const char* path)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    char magic[4];
    uint32_t n = 0;
    if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "MDXF", 4) != 0 || std::fread(&n, 4, 1, f) != 1)
        throw std::runtime_error("bad frames header");
    std::vector<Image> out(n);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t hdr[4];
        if (std::fread(hdr, 4, 4, f) != 4) throw std::runtime_error("truncated frame header");
        Image& im = out[i];
        im.height = hdr[0];
        im.width = hdr[1];
        im.step = hdr[2];
        im.encoding.resize(hdr[3]);
        im.data.resize((size_t)im.step * im.height);
        if (std::fread(&im.encoding[0], 1, hdr[3], f) != hdr[3] ||
            std::fread(im.data.data(), 1, im.data.size(), f) != im.data.size())
            throw std::runtime_error("truncated frame data");
    }
    std::fclose(f);
    return out;
}

static void write_bytes(const std::string& path, const void* p, size_t n)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, 1, n, f) != n) throw std::runtime_error("cannot write " + path);
    std::fclose(f);
}

// One output file's bytes: its i32 header, raw bytes appended, written to a path.
struct ByteBuffer {
    std::vector<uint8_t> bytes;
    ByteBuffer(std::initializer_list<int32_t> header) { put(header.begin(), header.size() * 4); }
    void put(const void* q, size_t n) { bytes.insert(bytes.end(), (const uint8_t*)q, (const uint8_t*)q + n); }
    template <class T> void put(const std::vector<T>& v) { put(v.data(), v.size() * sizeof(T)); }
    void write(const std::string& path) const { write_bytes(path, bytes.data(), bytes.size()); }
};

int main(int argc, char** argv)
{
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s <frames.bin> <outdir> [key=value ...]\n", argv[0]);
        return 2;
    }
    std::map<std::string, std::string> kv;
    for (int i = 3; i < argc; i++) {
        const char* eq = std::strchr(argv[i], '=');
        if (!eq) {
            std::fprintf(stderr, "bad argument %s\n", argv[i]);
            return 2;
        }
        kv[std::string(argv[i], eq - argv[i])] = eq + 1;
    }
    auto geti = [&](const char* k, int d) { return kv.count(k) ? std::atoi(kv[k].c_str()) : d; };
    auto getd = [&](const char* k, double d) { return kv.count(k) ? std::atof(kv[k].c_str()) : d; };
    auto getu = [&](const char* k, uint32_t d) { return kv.count(k) ? (uint32_t)std::strtoul(kv[k].c_str(), nullptr, 10) : d; };
    try {
        Params p;
        p.pixel_step = geti("pixel_step", 10);
        p.min_vector_size = getd("min_vector_size", 1.0);
        p.skip_frames = geti("skip_frames", 1);
        p.num_motions = geti("num_motions", 2);
        p.egomotion = geti("egomotion", 1) != 0;
        p.live_path = geti("live_path", 1) != 0;
        p.sigma = getd("sigma", 0.5);
        p.seed = getu("seed", 1);
        p.subspace_precision = geti("subspace_precision", 0);
        p.distance_threshold = getd("distance_threshold", 0);
        p.angular_threshold = getd("angular_threshold", 0);
        p.abs_int = geti("abs_int", 0) != 0;
        p.log_contours = geti("log_contours", 0) != 0;
        p.region_min_area = geti("region_min_area", 0);
        p.region_open = geti("region_open", 1) != 0;
        p.detect_outliers = geti("detect_outliers", 0) != 0;
        p.include_zeros = geti("include_zeros", 0) != 0;
        p.use_all_frames = geti("use_all_frames", 1) != 0;
        p.residual_threshold = getd("residual_threshold", 0.2);
        p.cluster_contours = geti("cluster_contours", 0) != 0;
        p.region_contours = geti("region_contours", 0) != 0;
        p.region_external = geti("region_external", 0) != 0;
        p.region_outlines = geti("region_outlines", 0) != 0;
        p.background_subtraction = geti("background_subtraction", 0) != 0;
        const bool polling = !p.use_all_frames;
        const int device = geti("device", 0);
        const std::string out = argv[2];
        const std::vector<Image> frames = read_frames(argv[1]);
        if (frames.empty()) throw std::runtime_error("no frames");

        int k = 0;
        Publisher pub = [&](const std::string& topic, const Image& im) {
            write_bytes(out + "/pub_" + std::to_string(k) + "_" + topic + ".rgb8", im.data.data(), im.data.size());
        };
        MotionDetectionNode node(p, device, (int)frames[0].width, (int)frames[0].height, pub);
        std::unique_ptr<MotionLogger> ml;
        if (p.log_contours) ml.reset(new MotionLogger(out + "/motion.log"));
        // MotionLogger::writeBoundingBox of `count` rectangles (x, y, width, height at the head of every
        // `stride` ints); the frame is the callback's global_frame_count_ (node.cpp:433), before its closing
        // increment (:454)
        auto log_rectangles = [&](const int32_t* rects, int stride, size_t count) {
            if (!ml || polling) return;   // run() logs nothing
            const int frame = (int)node.global_frame_count() - 1;
            for (size_t i = 0; i < count; i++) {
                const int32_t* q = rects + stride * i;
                ml->write_bounding_box(q[0], q[1], q[2], q[3], frame, (int)i);
            }
        };
        // MotionLogger::writeContour of every hull (xy[2 * offsets[i] .. 2 * offsets[i + 1])), same frame
        auto log_hulls = [&](const std::vector<int32_t>& offsets, const std::vector<int32_t>& xy) {
            if (!ml || polling) return;   // run() logs nothing
            for (size_t i = 0; i + 1 < offsets.size(); i++)
                ml->write_contour(std::vector<int>(xy.begin() + 2 * offsets[i], xy.begin() + 2 * offsets[i + 1]),
                                  (int)node.global_frame_count() - 1, (int)i);
        };
        // background_subtraction=1 with region_min_area > 0: every frame that entered the ring, processed or not
        std::unique_ptr<MotionLogger> bgl;
        if (p.background_subtraction && p.region_min_area > 0) bgl.reset(new MotionLogger(out + "/motion_bg.log"));
        auto log_background = [&]() {
            const long frame = node.global_frame_count() - 1;
            if (!bgl || node.background_frame() != frame) return;
            const std::vector<int32_t>& q = node.background_regions();
            for (size_t i = 0; i + 3 < q.size(); i += 4)
                bgl->write_bounding_box(q[i], q[i + 1], q[i + 2], q[i + 3], (int)frame, (int)(i / 4));
        };
        for (size_t fi = 0; fi < frames.size(); fi++) {
            FrameResult r;
            if (polling) {
                node.image_callback(frames[fi], nullptr);
                log_background();
                if (!node.run_once(&r)) continue;
            } else {
                const bool done = node.image_callback(frames[fi], &r);
                log_background();
                if (!done) continue;
            }
            const bool live = p.live_path || polling;
            const std::string sfx = "_" + std::to_string(k) + ".bin";
            const int32_t num_kept = (int32_t)r.kept_clusters.size();
            // labels, kept ids and rectangles (cluster_contours: and the hulls): the tail of every cluster file,
            // then the rectangles' and the hulls' log lines
            auto put_clusters = [&](ByteBuffer& b) {
                b.put(r.cluster_labels);
                b.put(r.kept_clusters);
                b.put(r.rectangles);
                log_rectangles(r.rectangles.data(), 4, r.kept_clusters.size());
                if (!p.cluster_contours) return;
                if (r.contour_offsets.empty()) r.contour_offsets.assign(1, 0);   // the stage did not run: no cluster
                b.put(r.contour_offsets);
                b.put(r.contours);
                log_hulls(r.contour_offsets, r.contours);
            };
            const int traj_len = r.trajectories.empty() ? 0 : (int)r.trajectories[0].size() / 2;
            ByteBuffer res{r.num_vectors, r.rc, r.w, r.h, r.npts, (int32_t)r.trajectories.size(), traj_len,
                           (int32_t)(r.outlier_points.size() / 2)};
            res.put(r.H, sizeof(r.H));
            if (!live) {
                res.put(r.next_pts);
                res.put(r.status);
                res.put(r.mask);
            } else {
                for (const auto& t : r.trajectories) res.put(t);
                res.put(r.outlier_points);
                const int32_t nc = (int32_t)r.subspace_columns.size();
                res.put(&nc, 4);
                res.put(r.subspace_columns);
                write_trajectories(r.trajectories, out + "/traj_" + std::to_string(k));
            }
            if (polling ? p.run_clusters_on() : p.point_clusters_on()) {
                ByteBuffer b{r.num_clusters, num_kept};
                put_clusters(b);
                b.write(out + "/clusters" + sfx);
            }
            if (!polling && p.vector_clusters_on()) {
                // (no trajectory survived: the stage did not run, no grid, n = 0)
                ByteBuffer b{(int32_t)r.cluster_labels.size(), r.num_active_vectors, r.num_clusters, num_kept};
                b.put(r.grid);
                put_clusters(b);
                b.write(out + "/vclusters" + sfx);
            }
            if (!polling && p.regions_on()) {
                ByteBuffer b{r.num_regions_all, (int32_t)(r.regions.size() / 8)};
                b.put(r.regions);
                b.write(out + "/regions" + sfx);
                if (p.region_external) {
                    ByteBuffer pb{(int32_t)(r.regions.size() / 8)};
                    pb.put(r.region_parent);
                    const int32_t next = (int32_t)r.region_external_index.size();
                    pb.put(&next, 4);
                    pb.put(r.region_external_index);
                    pb.write(out + "/region_parents" + sfx);
                    std::vector<int32_t> ext;     // the external records, in record order
                    for (const int32_t i : r.region_external_index)
                        ext.insert(ext.end(), r.regions.begin() + 8 * i, r.regions.begin() + 8 * (i + 1));
                    log_rectangles(ext.data(), 8, ext.size() / 8);
                } else {
                    log_rectangles(r.regions.data(), 8, r.regions.size() / 8);
                }
                if (p.region_contours) {
                    ByteBuffer hb{(int32_t)(p.region_external ? r.region_external_index.size() : r.regions.size() / 8)};
                    hb.put(r.region_contour_offsets);
                    hb.put(r.region_contours);
                    hb.write(out + "/region_hulls" + sfx);
                    log_hulls(r.region_contour_offsets, r.region_contours);
                }
                if (p.region_outlines) {
                    ByteBuffer ob{(int32_t)(p.region_external ? r.region_external_index.size() : r.regions.size() / 8)};
                    ob.put(r.region_outline_offsets);
                    ob.put(r.region_outlines);
                    ob.write(out + "/region_outlines" + sfx);
                    log_hulls(r.region_outline_offsets, r.region_outlines);
                }
            }
            if (!polling && p.detect_outliers_on()) {
                const mdx_outlier_stats& st = r.outlier_stats;
                const double osta[4] = {st.median_angle, st.mad_angle, st.median_magnitude, st.mad_magnitude};
                ByteBuffer b{(int32_t)r.outlier_flags.size(), st.selected, st.flagged_angle, st.flagged_magnitude,
                             st.outliers, r.num_active_vectors, r.num_clusters, num_kept};
                b.put(osta, sizeof(osta));
                b.put(r.grid);
                b.put(r.outlier_flags);
                put_clusters(b);
                b.write(out + "/outliers" + sfx);
            }
            res.write(out + "/res" + sfx);
            write_flow(r.vector_image, r.w, r.h, p.pixel_step, out + "/flow_" + std::to_string(k));
            std::printf("frame %zu -> processed %d: num_vectors %d%s\n", fi, k, r.num_vectors,
                        live ? (", trajectories " + std::to_string(r.trajectories.size()) + ", outliers " +
                                       std::to_string(r.outlier_points.size() / 2)).c_str()
                                    : "");
            k++;
        }
        std::printf("processed %d of %zu frames\n", k, frames.size());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "mdx_node: %s\n", e.what());
        return 1;
    }
    return 0;
}
