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
//
// frames.bin: "MDXF", u32 count, then per frame u32 height, u32 width, u32 step, u32 len, the
// encoding (len bytes) and step * height data bytes (a sensor_msgs/Image each).
// For the k-th processed frame it writes to <outdir>:
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
//   motion.log                    log_contours=1: created at start; MotionLogger::writeBoundingBox of
//                                 every kept cluster's rectangle (node.cpp:431-434), "frame, id, tl.x,
//                                 tl.y, br.x, br.y" with frame = the node's global_frame_count_ during
//                                 that callback and id the index among the kept clusters.  (writeContour,
//                                 :426-429, needs the convex hulls, which are out of scope.)
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
    auto get = [&](const char* k, const char* d) { return kv.count(k) ? kv[k] : std::string(d); };
    try {
        Params p;
        p.pixel_step = std::atoi(get("pixel_step", "10").c_str());
        p.min_vector_size = std::atof(get("min_vector_size", "1.0").c_str());
        p.skip_frames = std::atoi(get("skip_frames", "1").c_str());
        p.num_motions = std::atoi(get("num_motions", "2").c_str());
        p.egomotion = std::atoi(get("egomotion", "1").c_str()) != 0;
        p.live_path = std::atoi(get("live_path", "1").c_str()) != 0;
        p.sigma = std::atof(get("sigma", "0.5").c_str());
        p.seed = (uint32_t)std::strtoul(get("seed", "1").c_str(), nullptr, 10);
        p.subspace_precision = std::atoi(get("subspace_precision", "0").c_str());
        p.distance_threshold = std::atof(get("distance_threshold", "0").c_str());
        p.angular_threshold = std::atof(get("angular_threshold", "0").c_str());
        p.abs_int = std::atoi(get("abs_int", "0").c_str()) != 0;
        p.log_contours = std::atoi(get("log_contours", "0").c_str()) != 0;
        p.region_min_area = std::atoi(get("region_min_area", "0").c_str());
        p.region_open = std::atoi(get("region_open", "1").c_str()) != 0;
        p.detect_outliers = std::atoi(get("detect_outliers", "0").c_str()) != 0;
        p.include_zeros = std::atoi(get("include_zeros", "0").c_str()) != 0;
        const int device = std::atoi(get("device", "0").c_str());
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
        const bool clustering = p.live_path && p.egomotion && p.distance_threshold > 0;
        const bool vclustering = p.live_path && !p.egomotion && p.distance_threshold > 0 && p.angular_threshold > 0;
        const bool outliers = !p.live_path && p.detect_outliers && p.distance_threshold > 0 && p.angular_threshold > 0;
        for (size_t fi = 0; fi < frames.size(); fi++) {
            FrameResult r;
            if (!node.image_callback(frames[fi], &r)) continue;
            const int traj_len = r.trajectories.empty() ? 0 : (int)r.trajectories[0].size() / 2;
            int32_t hdr[8] = {r.num_vectors, r.rc, r.w, r.h, r.npts, (int32_t)r.trajectories.size(), traj_len,
                              (int32_t)(r.outlier_points.size() / 2)};
            std::vector<uint8_t> buf((uint8_t*)hdr, (uint8_t*)hdr + sizeof(hdr));
            auto put = [&](const void* q, size_t n) { buf.insert(buf.end(), (const uint8_t*)q, (const uint8_t*)q + n); };
            put(r.H, sizeof(r.H));
            if (!p.live_path) {
                put(r.next_pts.data(), r.next_pts.size() * 4);
                put(r.status.data(), r.status.size());
                put(r.mask.data(), r.mask.size());
            } else {
                for (const auto& t : r.trajectories) put(t.data(), t.size() * 4);
                put(r.outlier_points.data(), r.outlier_points.size() * 4);
                const int32_t nc = (int32_t)r.subspace_columns.size();
                put(&nc, 4);
                put(r.subspace_columns.data(), r.subspace_columns.size() * 4);
                write_trajectories(r.trajectories, out + "/traj_" + std::to_string(k));
            }
            if (clustering) {
                const int32_t chdr[2] = {r.num_clusters, (int32_t)r.kept_clusters.size()};
                std::vector<uint8_t> cb((const uint8_t*)chdr, (const uint8_t*)chdr + sizeof(chdr));
                auto cput = [&](const void* q, size_t n) { cb.insert(cb.end(), (const uint8_t*)q, (const uint8_t*)q + n); };
                cput(r.cluster_labels.data(), r.cluster_labels.size() * 4);
                cput(r.kept_clusters.data(), r.kept_clusters.size() * 4);
                cput(r.rectangles.data(), r.rectangles.size() * 4);
                write_bytes(out + "/clusters_" + std::to_string(k) + ".bin", cb.data(), cb.size());
                // the callback's global_frame_count_ (node.cpp:433), before its closing increment (:454)
                const int frame = (int)node.global_frame_count() - 1;
                if (ml)
                    for (size_t i = 0; i < r.kept_clusters.size(); i++)
                        ml->write_bounding_box(r.rectangles[4 * i], r.rectangles[4 * i + 1], r.rectangles[4 * i + 2],
                                               r.rectangles[4 * i + 3], frame, (int)i);
            }
            if (vclustering) {
                const int32_t n = (int32_t)r.cluster_labels.size();
                const int32_t vhdr[4] = {n, r.num_active_vectors, r.num_clusters, (int32_t)r.kept_clusters.size()};
                std::vector<uint8_t> vb((const uint8_t*)vhdr, (const uint8_t*)vhdr + sizeof(vhdr));
                auto vput = [&](const void* q, size_t len) { vb.insert(vb.end(), (const uint8_t*)q, (const uint8_t*)q + len); };
                if (n > 0)                                      // (no trajectory survived: no grid, n = 0)
                    for (int y = 0; y < r.h; y += p.pixel_step)
                        for (int x = 0; x < r.w; x += p.pixel_step) vput(&r.vector_image[((size_t)y * r.w + x) * 4], 32);
                vput(r.cluster_labels.data(), r.cluster_labels.size() * 4);
                vput(r.kept_clusters.data(), r.kept_clusters.size() * 4);
                vput(r.rectangles.data(), r.rectangles.size() * 4);
                write_bytes(out + "/vclusters_" + std::to_string(k) + ".bin", vb.data(), vb.size());
                const int frame = (int)node.global_frame_count() - 1;
                if (ml)
                    for (size_t i = 0; i < r.kept_clusters.size(); i++)
                        ml->write_bounding_box(r.rectangles[4 * i], r.rectangles[4 * i + 1], r.rectangles[4 * i + 2],
                                               r.rectangles[4 * i + 3], frame, (int)i);
            }
            if (!p.live_path && p.region_min_area > 0) {
                const int32_t ghdr[2] = {r.num_regions_all, (int32_t)(r.regions.size() / 8)};
                std::vector<uint8_t> gb((const uint8_t*)ghdr, (const uint8_t*)ghdr + sizeof(ghdr));
                gb.insert(gb.end(), (const uint8_t*)r.regions.data(), (const uint8_t*)(r.regions.data() + r.regions.size()));
                write_bytes(out + "/regions_" + std::to_string(k) + ".bin", gb.data(), gb.size());
                const int frame = (int)node.global_frame_count() - 1;
                if (ml)
                    for (size_t i = 0; i < r.regions.size() / 8; i++)
                        ml->write_bounding_box(r.regions[8 * i], r.regions[8 * i + 1], r.regions[8 * i + 2],
                                               r.regions[8 * i + 3], frame, (int)i);
            }
            if (outliers) {
                const int32_t n = (int32_t)r.outlier_flags.size();
                const mdx_outlier_stats& st = r.outlier_stats;
                const int32_t ohdr[8] = {n, st.selected, st.flagged_angle, st.flagged_magnitude, st.outliers,
                                         r.num_active_vectors, r.num_clusters, (int32_t)r.kept_clusters.size()};
                const double osta[4] = {st.median_angle, st.mad_angle, st.median_magnitude, st.mad_magnitude};
                std::vector<uint8_t> ob((const uint8_t*)ohdr, (const uint8_t*)ohdr + sizeof(ohdr));
                auto oput = [&](const void* q, size_t len) { ob.insert(ob.end(), (const uint8_t*)q, (const uint8_t*)q + len); };
                oput(osta, sizeof(osta));
                for (int y = 0; y < r.h; y += p.pixel_step)
                    for (int x = 0; x < r.w; x += p.pixel_step) oput(&r.vector_image[((size_t)y * r.w + x) * 4], 32);
                oput(r.outlier_flags.data(), r.outlier_flags.size());
                oput(r.cluster_labels.data(), r.cluster_labels.size() * 4);
                oput(r.kept_clusters.data(), r.kept_clusters.size() * 4);
                oput(r.rectangles.data(), r.rectangles.size() * 4);
                write_bytes(out + "/outliers_" + std::to_string(k) + ".bin", ob.data(), ob.size());
                const int frame = (int)node.global_frame_count() - 1;
                if (ml)
                    for (size_t i = 0; i < r.kept_clusters.size(); i++)
                        ml->write_bounding_box(r.rectangles[4 * i], r.rectangles[4 * i + 1], r.rectangles[4 * i + 2],
                                               r.rectangles[4 * i + 3], frame, (int)i);
            }
            write_bytes(out + "/res_" + std::to_string(k) + ".bin", buf.data(), buf.size());
            write_flow(r.vector_image, r.w, r.h, p.pixel_step, out + "/flow_" + std::to_string(k));
            std::printf("frame %zu -> processed %d: num_vectors %d%s\n", fi, k, r.num_vectors,
                        p.live_path ? (", trajectories " + std::to_string(r.trajectories.size()) + ", outliers " +
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
