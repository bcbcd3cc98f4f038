/*
 * mdx.h -- C-ABI of the MI355X-native motion-detection hot path.
 *
 * Drop-in boundary for the reference's in-process seam
 *   int OpticalFlowCalculator::calculateOpticalFlow(const cv::Mat& image1,
 *        const cv::Mat& image2, cv::Mat& optical_flow_vectors, int pixel_step,
 *        cv::Mat& comp, double min_vector_size)
 * declared at reference common/include/motion_detection/optical_flow_calculator.h:19 and
 * defined at common/src/optical_flow_calculator.cpp:30-130, called from
 * MotionDetectionNode::runOpticalFlow (ros/src/motion_detection_node.cpp:76-92, call :82).
 *
 * Plain C types only: pointers + sizes, no torch / OpenCV / HIP types in signatures.
 * Errors are integer codes; no C++ exception crosses this boundary.  A context owns one
 * HIP stream on one device; it is not thread-safe, but different contexts may be driven
 * concurrently from different host threads (one context per camera stream / GPU).
 */
#ifndef MDX_H_
#define MDX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDX_ABI_VERSION 11  /* 2: mdx_params.call_pipelining, mdx_input_ready.
                                3: mdx_lk_fallbacks; mdx_params grew ransac_iters, ransac_thresh and
                                   ransac_seed (16 more bytes: a caller built against ABI 2 passes a
                                   shorter struct); mdx_sync / mdx_device_sync return MDX_OK after an
                                   LK hand-off that gave up and was recomputed (ABI 2: MDX_EHIP).
                                4: mdx_abi_version and mdx_params_size: check both at start-up --
                                   a mismatch means the header and the library differ.
                                5: mdx_debug_warp_paths (a new entry, as 3 and 4 were: nothing existing
                                   changes, but a caller's header and library must be the same age).
                                6: mdx_cluster_euclidean (a new entry; mdx_params is unchanged, 80 bytes).
                                7: mdx_mask_regions_dev and mdx_mask_regions (new entries; mdx_params is
                                   unchanged, 80 bytes).
                                8: mdx_cluster_vectors (a new entry; mdx_params is unchanged, 80 bytes).
                                9: mdx_find_outliers and mdx_outlier_stats (a new entry; mdx_params is
                                   unchanged, 80 bytes).
                                10: mdx_half_size, mdx_resize_half_dev, mdx_resize_half and
                                   mdx_ring_push_half (new entries; mdx_params is unchanged, 80 bytes).
                                11: mdx_cluster_hulls (a new entry; mdx_params is unchanged, 80 bytes).
                                   mdx_region_hulls_dev and mdx_mask_region_hulls joined under 11: two
                                   more entries, nothing existing changes.  mdx_region_parents_dev and
                                   mdx_mask_regions_tree joined under 11 the same way, and so did
                                   mdx_region_outlines_dev and mdx_mask_region_outlines. */

/* Return codes */
#define MDX_OK           0
#define MDX_EINVAL      -1   /* bad argument (size, format, unsupported parameter) */
#define MDX_EHIP        -2   /* HIP runtime error (message in mdx_last_error) */
#define MDX_ENOMEM      -3   /* device allocation failed */
#define MDX_EDEGENERATE  1   /* success, but fewer than 4 accepted vectors: no fit, mask zeroed.
                                num_vectors == 0 is the reference's "no mask" branch
                                (optical_flow_calculator.cpp:118); 1..3 is reference UB (:120,
                                reads past src_points) and is defined here as "no fit". */

/* Pixel formats of the input frames (sensor_msgs/Image encodings the node accepts). */
#define MDX_FMT_GRAY8 0      /* mono8: cv_bridge rgb8 replication then BGR2GRAY == identity */
#define MDX_FMT_RGB8  1      /* rgb8 (node.cpp:271), BGR2GRAY weights land swapped (:50) */
#define MDX_FMT_BGR8  2      /* bgr8: cv_bridge converts to rgb8 first, same swapped weights */

/* Global-motion fit used for the back-warp. */
#define MDX_FIT_FIRST4   0   /* reference: getPerspectiveTransform on the first 4 accepted
                                vectors in x-major grid order (:120) */
#define MDX_FIT_EXTERNAL 1   /* caller supplies H (forward, frame1 -> frame2) per pair */
#define MDX_FIT_RANSAC   2   /* NOT in the reference (parity with it N/A): deterministic RANSAC over
                                all accepted vectors -- mdx_params.ransac_iters hypotheses, each the
                                reference's own 4-point getPerspectiveTransform on 4 accepted vectors
                                drawn by a counter-based generator (splitmix64 of ransac_seed,
                                hypothesis, draw); the hypothesis with the most inliers (reprojection
                                error <= ransac_thresh px; first on ties) is H, without a refit.
                                Restated in oracle/ and bit-exact there. */

/* mdx_fit_subspace arithmetic (see its comment below). */
#define MDX_SUBSPACE_F64 0   /* double Householder basis and residuals (stable; the default) */
#define MDX_SUBSPACE_F32 1   /* the reference's float arithmetic shape: Eigen::MatrixXf
                                (outlier_detector.cpp:243-290), Pnd formed explicitly in float */

typedef struct {
    int    win;              /* LK window side; reference hard-codes 40 (:41). Only 40 is supported. */
    int    max_level;        /* reference MAX_LEVEL = 5 (:40) */
    int    max_iters;        /* TermCriteria count = 10 (:44) */
    double eps;              /* TermCriteria epsilon = 0.03 (:44) */
    float  min_eig;          /* minEigThreshold = 1e-3 (:71) */
    int    thresh;           /* threshold(comp, comp, 190, 255, BINARY) (:127) */
    int    pixel_step;       /* ROS param pixel_step (node.cpp:29; 10 in bag.launch:27) */
    double min_vector_size;  /* ROS param min_vector_size, default 1.0 (node.cpp:44) */
    int    fit_mode;         /* MDX_FIT_FIRST4 (default), MDX_FIT_EXTERNAL or MDX_FIT_RANSAC */
    int    subspace_precision; /* mdx_fit_subspace arithmetic: MDX_SUBSPACE_F64 (default) or _F32 */
    int    call_pipelining;  /* 0 (default) or 1: consecutive device-entry calls overlap (below) */
    int    ransac_iters;     /* MDX_FIT_RANSAC hypotheses, 1..1024 (default 128) */
    double ransac_thresh;    /* MDX_FIT_RANSAC inlier reprojection error, px (default 3.0, as
                                OpenCV findHomography's ransacReprojThreshold) */
    uint32_t ransac_seed;    /* MDX_FIT_RANSAC generator seed (default 20141105) */
} mdx_params;

/*
 * Call pipelining (mdx_params.call_pipelining = 1).  The pyramid workspace holds two halves used by
 * alternate device-entry calls (mdx_flow_warp_diff_batch_dev, mdx_band_flow_dev), and a call's
 * front end (gray, pyramids) runs on the context's second stream, behind the previous call's
 * flow-independent LK work, so it overlaps that call's last LK level and its fit/warp.  The front
 * end then does NOT wait for earlier work on the context stream: the call's input frames must be
 * in HBM when it is made (mdx_memcpy_h2d returns after the copy), or the caller names the event
 * after which they are, with mdx_input_ready.  Outputs are unaffected; results are identical with
 * and without pipelining.  The workspace doubles its pyramid slabs while the flag is set.
 */

typedef struct mdx_ctx mdx_ctx;

/* Fill params with the reference's constants. */
void mdx_default_params(mdx_params* p);

/* The ABI version and sizeof(mdx_params) the library was built with.  A caller compares them with
 * MDX_ABI_VERSION and its own sizeof(mdx_params) before the first mdx_create: the struct is passed
 * by pointer, so a library newer than the caller's header would read past a shorter struct. */
int mdx_abi_version(void);
size_t mdx_params_size(void);

/* Number of grid points for a frame: ceil(w/ps) * ceil(h/ps) (:56-64, x-major order:
 * point k = ix*ny + iy sits at (ix*ps, iy*ps)). */
int mdx_grid_count(int w, int h, int pixel_step);

/* Create a context on HIP device `device`.  max_w/max_h/max_batch size the device
 * workspace (pyramids, derivatives, scratch) so that the per-frame path never allocates.
 * Returns NULL on failure; mdx_create_error() then holds the reason. */
mdx_ctx* mdx_create(int device, int max_w, int max_h, int max_batch, const mdx_params* p);
const char* mdx_create_error(void);
int mdx_destroy(mdx_ctx* ctx);
const char* mdx_last_error(const mdx_ctx* ctx);
int mdx_set_params(mdx_ctx* ctx, const mdx_params* p);
int mdx_get_params(const mdx_ctx* ctx, mdx_params* p);

/* The context's HIP stream (hipStream_t as void*) and device id; for interop only. */
void* mdx_stream(mdx_ctx* ctx);
int mdx_device(const mdx_ctx* ctx);
/* PCI bus id ("0000:xx:yy.z") of the context's device, so multi-GPU records can show which
 * distinct devices the ranks ran on. */
int mdx_device_pci(const mdx_ctx* ctx, char* buf, int len);
/* Build provenance: "src_sha256=<sha256 of the library's sources> arch=gfx950", compiled in by
 * csrc/Makefile.  tests/test_abi.py checks it against the sources in the tree. */
const char* mdx_build_info(void);
/* Wait for the context's work (and collect the LK fallback counts below). */
int mdx_sync(mdx_ctx* ctx);
/* hipDeviceSynchronize on the context's device (all streams); the same collection. */
int mdx_device_sync(mdx_ctx* ctx);
/* LK level dataflow fallbacks since mdx_create, as of the last mdx_sync / mdx_device_sync:
 *   counts[0]  group waits that gave up (a group of level l waits, bounded, for its pair's level
 *              l+1 groups, whose launch may not be dispatched in time: the device is preempted,
 *              shared, or serializes kernels as a counter-collecting profiler does)
 *   counts[1]  gate waits that gave up (the same, before a level's launch)
 *   counts[2]  levels recomputed
 * A level whose wait gave up is abandoned and recomputed in sequence within the same call, after
 * its coarser level, together with every finer level: the outputs are exact either way (the
 * reference call always returns a result, optical_flow_calculator.cpp:71).  The counts are
 * statistics, not errors. */
int mdx_lk_fallbacks(const mdx_ctx* ctx, long long counts[3]);
/* Name the input frames' producer: the next device-entry call (mdx_flow_warp_diff_batch_dev,
 * mdx_band_flow_dev, mdx_warp_diff_dev) makes its first stage wait for `hip_event` (a hipEvent_t
 * the caller recorded on its own stream after writing the frames) before reading them.  One-shot:
 * consumed by that call.  Needed with call pipelining whenever the frames are produced
 * asynchronously (a zero-copy producer on another stream); harmless without it. */
int mdx_input_ready(mdx_ctx* ctx, void* hip_event);

/*
 * Synchronous host-buffer entry: the direct replacement of calculateOpticalFlow.
 *   img1, img2  w x h frames, row pitch `stride` bytes, format `fmt`.  Only w * channels bytes
 *               of the last row are read: a pitched view (a cv::Mat ROI) may end with its last pixel.
 *   next_pts    [2*npts] float  LK output positions (x-major grid order)        or NULL
 *   status      [npts]   uint8  LK status                                       or NULL
 *   vectors     [4*npts] double the reference's Vec4d per grid point:
 *               (x, y, dx, dy) accepted / (x, y, 0, 0) tracked / (-1, -1, 0, 0) lost
 *               (:78-117; stored densely per grid point)     or NULL
 *   mask        [w*h]    uint8  thresholded |warp(gray1) - gray2| (comp, :122-127) or NULL
 *   H           [9]      double perspective transform (first-4 fit or external)  or NULL
 *   H_external  [9]      double forward H when fit_mode == MDX_FIT_EXTERNAL, else NULL
 *   num_vectors          number of accepted vectors (the reference's return value)
 * Returns MDX_OK, MDX_EDEGENERATE, or a negative error.
 */
int mdx_flow_warp_diff(mdx_ctx* ctx, const uint8_t* img1, const uint8_t* img2,
                       int w, int h, int stride, int fmt,
                       float* next_pts, uint8_t* status, double* vectors,
                       uint8_t* mask, double* H, const double* H_external, int* num_vectors);

/*
 * Asynchronous batched device entry (zero-copy; everything stays in HBM).  Pair i reads
 * d_img1 + i*frame_stride and d_img2 + i*frame_stride.  Outputs (device pointers, each may
 * be NULL except where noted):
 *   d_next_pts  [batch][npts][2] float     d_status [batch][npts] uint8
 *   d_vectors   [batch][npts][4] double    d_mask   [batch][h][w] uint8
 *   d_H         [batch][9] double          d_num_vectors [batch] int32
 *   d_H_external[batch][9] double (input; required iff fit_mode == MDX_FIT_EXTERNAL)
 * Work is enqueued on the context stream; call mdx_sync (or sync the stream) before use.
 */
int mdx_flow_warp_diff_batch_dev(mdx_ctx* ctx, int batch,
                                 const uint8_t* d_img1, const uint8_t* d_img2,
                                 int w, int h, int stride, size_t frame_stride, int fmt,
                                 float* d_next_pts, uint8_t* d_status, double* d_vectors,
                                 uint8_t* d_mask, double* d_H, const double* d_H_external,
                                 int* d_num_vectors);

/*
 * The fused back-warp + absdiff + threshold kernel alone (rows A8-A10): for each pair,
 * mask = (|warpPerspective(gray1, H) - gray2| > thresh) * 255 with the reference's
 * warpPerspective arithmetic (inverse of H, FP64 coordinates, 1/32 px, BORDER_CONSTANT 0).
 * d_gray1/d_gray2: [batch] frames of w x h gray8, row pitch `stride`, frame pitch
 * `frame_stride`.  d_H: [batch][9] forward transforms (device).  d_mask: [batch][h][w].
 */
int mdx_warp_diff_dev(mdx_ctx* ctx, int batch, const uint8_t* d_gray1, const uint8_t* d_gray2,
                      int w, int h, int stride, size_t frame_stride,
                      const double* d_H, uint8_t* d_mask);

/*
 * Row-tiled path: one frame pair split by rows over several GPUs (8K RGB
 * over 8 GPUs).  No reference interface corresponds -- the reference runs the whole frame in one
 * calculateOpticalFlow call (optical_flow_calculator.cpp:30-130); this splits that call at its
 * only global step, the first-four-accepted getPerspectiveTransform input (:118-120).
 *
 * Rank r owns the destination rows [y0, y1) (the bands partition [0, h)) and the grid points
 * whose row y = gy*pixel_step lies in that band.  Per pair:
 *   1. every rank: mdx_band_flow_dev -- rows A1-A6 for the band's points.  next_pts / status /
 *      vectors are full-frame arrays ([npts]...); only the band's entries are written.  d_cand
 *      receives the band's mdx_band_cand record.
 *   2. the caller all-gathers the ranks' records (any transport: RCCL all_gather over xGMI, or
 *      host memory) into one device array, in any order.
 *   3. every rank: mdx_band_fit_warp_dev -- the first four accepted points overall are the four
 *      smallest indices over all records; the fit, its inverse and num_vectors are then exactly
 *      the full path's.  Writes mask rows [y0, y1) to d_mask_band (row pitch w) and, when
 *      non-NULL, d_H[9] and d_num_vectors.
 * Both entries are asynchronous on the context stream.  Step 3 reads the pyramids of the
 * context's latest mdx_band_flow_dev call, which must be of the same frame pair (several bands of
 * one pair may run step 1 one after another first), and converts from that call's d_img1 the
 * frame-1 rows its warp reads beyond the band, so d_img1 must still hold frame 1.  Any other entry
 * that rebuilds the context's pyramids in between (a pair or trajectory call) voids them: step 3
 * then returns MDX_EINVAL instead of warping another pair's frames.  fit_mode must be
 * MDX_FIT_FIRST4.  With call pipelining, consecutive band calls alternate the two pyramid halves;
 * step 3 reads (and then releases) only the latest call's half, the other half having been
 * released by its own call once its classification was queued.
 */
typedef struct mdx_band_cand {
    int32_t count;     /* accepted vectors (status && |d| > min_vector_size) in the band */
    int32_t n;         /* min(count, 4) */
    int32_t idx[4];    /* x-major grid index k = gx*ny + gy of the band's first n accepted points */
    float src[8];      /* their grid positions (x, y) */
    float dst[8];      /* their tracked positions next_pts[k] */
    int32_t pad_[2];
} mdx_band_cand;       /* 96 bytes */

int mdx_band_flow_dev(mdx_ctx* ctx, const uint8_t* d_img1, const uint8_t* d_img2,
                      int w, int h, int stride, int fmt, int y0, int y1,
                      float* d_next_pts, uint8_t* d_status, double* d_vectors,
                      mdx_band_cand* d_cand);
int mdx_band_fit_warp_dev(mdx_ctx* ctx, int nrec, const mdx_band_cand* d_cands, int y0, int y1,
                          uint8_t* d_mask_band, double* d_H, int* d_num_vectors);

/*
 * Trajectory tracking: replaces OpticalFlowCalculator::calculateOpticalFlowTrajectory
 * (optical_flow_calculator.h:20-21, optical_flow_calculator.cpp:133-257), the node's live caller
 * (motion_detection_node.cpp:94-110 over 2*num_motions+1 frames, :241).  Synchronous.
 *   imgs        nimg >= 2 host frames, each w x h, row pitch `stride`, format `fmt`.  Only
 *               w * channels bytes of a frame's last row are read (as in mdx_flow_warp_diff).
 * The pixel_step grid is tracked through the nimg-1 consecutive pairs; each pass starts from the
 * points the previous one left (a point moves only when tracked and strictly inside the 10-px
 * border, :207-216).  Outputs (any may be NULL; npts = mdx_grid_count(w, h, pixel_step)):
 *   traj        [npts][nimg][2] float  point i's positions: its grid point, then each accepted
 *               move (entries past traj_len[i] are unspecified)
 *   traj_len    [npts] int32           the reference's init_traj_list[i].size(); it reports the
 *               trajectory iff traj_len[i] == nimg (:244-249)
 *   start_pts   [npts][2] float        the points entering the last pass (where the reference
 *               stores each Vec4d: optical_flow_vectors.at<Vec4d>((int)y, (int)x))
 *   vectors     [npts][4] double       the last pass's Vec4d per point (:183-206, :220-230)
 *   num_vectors                        the reference's return value (last pass only)
 * Grows the context's pyramid workspace to nimg - 1 slots (one per pair) when needed.
 */
int mdx_flow_trajectory(mdx_ctx* ctx, const uint8_t* const* imgs, int nimg, int w, int h, int stride,
                        int fmt, float* traj, int32_t* traj_len, float* start_pts, double* vectors,
                        int* num_vectors);

/*
 * One host block for a trajectory call's outputs.  With traj, start_pts, vectors and traj_len at
 * these byte offsets of one block (e.g. from mdx_host_alloc), mdx_flow_trajectory and
 * mdx_ring_trajectory read all four back with one copy instead of four.  offsets[] = {traj,
 * start_pts, vectors, traj_len}; returns the block size in bytes.  Any other placement works too.
 * Outputs that are all in page-locked memory (mdx_host_alloc) are written by the chained launch
 * itself through their device mapping, with no readback copy.  Either way traj's entries past
 * traj_len[i] are 0.
 */
size_t mdx_trajectory_layout(int npts, int nimg, size_t offsets[4]);

/*
 * Resident frame ring for the live chain: the node's raw_images_ deque (motion_detection_node.h:82,
 * filled at node.cpp:248-261), whose every frame the reference re-converts, re-uploads and
 * re-pyramids on each callback (:266-287, then optical_flow_calculator.cpp:166-170).  Here a frame
 * crosses PCIe and is pyramided (gray, padded levels, Scharr planes) once, when it enters the ring,
 * and stays in HBM while it is in it.
 *   mdx_ring_push        append a frame (w x h, row pitch `stride`, format `fmt`), then drop frames
 *                        from the front until at most `keep` remain (the deque's size after the
 *                        reference's push / pop at :248-261).  A frame of another size empties the
 *                        ring first.  Returns the number of frames held, or a negative error.
 *   mdx_ring_trajectory  calculateOpticalFlowTrajectory over the frames held (>= 2), outputs exactly
 *                        as mdx_flow_trajectory's (nimg = the ring size).
 *   mdx_ring_reset       empty the ring.
 * mdx_ring_push only queues the upload and the pyramid on the context's stream: the frame's host
 * memory (page-locked memory is read by DMA after the call returns) must stay unchanged until the
 * next mdx_ring_trajectory or mdx_sync returns.  Only w * channels bytes of the frame's last row
 * are read (as in mdx_flow_warp_diff).
 */
int mdx_ring_push(mdx_ctx* ctx, const uint8_t* img, int w, int h, int stride, int fmt, int keep);
int mdx_ring_trajectory(mdx_ctx* ctx, float* traj, int32_t* traj_len, float* start_pts, double* vectors,
                        int* num_vectors);
int mdx_ring_reset(mdx_ctx* ctx);

/*
 * Half-size ingest: the reference node's cv::resize(img, out, cv::Size(), 0.5, 0.5) of every frame
 * wider than 320 px (ros/src/motion_detection_node.cpp:470-474), as a device stage.  The arithmetic is
 * OpenCV 2.4.8's resize(): INTER_LINEAR at an integer scale of 2 is redirected to INTER_AREA's fast
 * 2x2 mode.  Restated from the published algorithm and unpinned against a real build.
 *   size      dw = cvRound(w * 0.5), dh = cvRound(h * 0.5), half to even: an even side halves, an odd
 *             side 2k+1 gives k for even k and k+1 for odd k (3->2, 5->2, 7->4, 9->4, 321->160, 323->162)
 *   full      destination pixel (dx, dy) with 2dx+1 < w and 2dy+1 < h, per channel:
 *             (S[2dy][2dx] + S[2dy][2dx+1] + S[2dy+1][2dx] + S[2dy+1][2dx+1] + 2) >> 2
 *   partial   only where an odd side rounded up (the last column for dw = k+1, the last row likewise):
 *             cvRound((float)sum / count) over the block's in-frame pixels (count 2 on an edge, 1 in the
 *             corner), half to even: two pixels summing to 1 give 0, summing to 3 give 2
 *   dropped   where an odd side rounded down, the last source column or row is read by nothing
 * Channels are treated alone, so cv_bridge's mono8 replication and bgr8 reordering commute with it:
 * mono8 is halved as one channel and stays MDX_FMT_GRAY8, rgb8 / bgr8 as three and keep their format.
 */
/* dst size of the reference's cv::resize(src, dst, Size(), 0.5, 0.5).  MDX_EINVAL: w or h < 1, or a
 * side that rounds to 0 (w == 1 or h == 1: the reference's CV_Assert(dsize.area())); *dw, *dh are then
 * untouched. */
int mdx_half_size(int w, int h, int* dw, int* dh);

/* Asynchronous, batched, every pointer a device pointer; queued on the context stream; honours
 * mdx_input_ready like the other device entries.  channels 1 or 3.  Frame b's row y starts at
 * d_src + b * frame_stride + y * stride, its halved row at d_dst + b * dst_frame_stride + y * dst_stride;
 * the bytes between dw * channels and dst_stride are never written.  d_dst must not overlap d_src.
 * Bases and pitches that are all multiples of 4 take the kernel's vector path, anything else its
 * byte path; the results are the same. */
int mdx_resize_half_dev(mdx_ctx* ctx, int batch, const uint8_t* d_src, int w, int h, int stride,
                        size_t frame_stride, int channels,
                        uint8_t* d_dst, int dst_stride, size_t dst_frame_stride);

/* One host frame, synchronous.  Only w * channels bytes of the last source row are read, and only
 * dw * channels bytes of each destination row are written. */
int mdx_resize_half(mdx_ctx* ctx, const uint8_t* src, int w, int h, int stride, int channels,
                    uint8_t* dst, int dst_stride);

/* mdx_ring_push of the halved frame: upload the full frame, halve it on the device, pyramid the
 * result.  The ring's geometry is (dw, dh); everything else is mdx_ring_push's contract (keep, the
 * return value, a frame of another size empties the ring, the host frame stays unchanged until the
 * next mdx_ring_trajectory / mdx_sync).  Frames pushed either way may share a ring when their
 * resulting sizes agree.  The context's size limits apply to the halved frame: the source may be up
 * to twice max_w x max_h; its staging buffer grows on first use. */
int mdx_ring_push_half(mdx_ctx* ctx, const uint8_t* img, int w, int h, int stride, int fmt, int keep);

/*
 * Trajectory subspace RANSAC: replaces OutlierDetector::fitSubspace
 * (common/include/motion_detection/outlier_detector.h:21, outlier_detector.cpp:236-331), called
 * by the node on the complete trajectories (motion_detection_node.cpp:348).
 *   traj        [ntraj][traj_len][2] float host trajectories (mdx_flow_trajectory's complete ones)
 *   rng         the caller's generator: the reference draws 50 x 4*num_motions samples per call
 *               from one srand(time(NULL)) stream (outlier_detector.cpp:17, :226); seed it with
 *               mdx_srand (glibc rand() restated: the same stream for the same seed)
 * Outputs (any may be NULL):
 *   columns     [4*num_motions] the winning sample's trajectory indices (the return value of
 *               fitSubspace is those trajectories); -1 when no hypothesis had an inlier
 *   is_outlier  [ntraj] 1 where the winner's residual exceeds sigma^2 * chi2_99[n-d]
 *   residuals   [ntraj] double, the winner's residuals
 *   outlier_points [n_outliers][2] float: each outlier's second-to-last point (:322), in order
 * Arithmetic: the reference's float meanSubtract, then by mdx_params.subspace_precision:
 * MDX_SUBSPACE_F64 -- double Householder QR of each sample and double residuals; MDX_SUBSPACE_F32
 * -- the reference's float shape (float basis, explicit float Pnd = I - sum u u', float x'(Pnd x)).
 * The reference itself runs Eigen's float JacobiSVD, which neither mode restates rotation for
 * rotation.
 */
typedef struct mdx_rand_state { uint32_t x[34]; int32_t pos; } mdx_rand_state;
void mdx_srand(mdx_rand_state* st, uint32_t seed);
int  mdx_rand(mdx_rand_state* st);
int  mdx_fit_subspace(mdx_ctx* ctx, const float* traj, int ntraj, int traj_len, int num_motions, double sigma,
                      mdx_rand_state* rng, int* columns, uint8_t* is_outlier, double* residuals,
                      float* outlier_points, int* n_outliers);

/*
 * Greedy Euclidean clustering and bounding rectangles: replaces FlowClusterer::clusterEuclidean
 * (common/src/flow_clusterer.cpp:231-269), which the node runs on fitSubspace's outlier_points
 * (motion_detection_node.cpp:355), and boundingRect of each kept cluster
 * (optical_flow_visualizer.cpp:230-236).  Restated from the source; unpinned against a real build
 * (no OpenCV 2.4 to compare with): copyTo's converting path and boundingRect in particular.
 *   Points are visited in input order.  Point i joins the cluster whose nearest member is nearest
 *   (strict <: the earliest-created cluster on a tie) when that distance d < distance_threshold
 *   (double compare; d = sqrt((double)s), s = dx*dx + dy*dy in float, each operation rounded,
 *   point_cluster.cpp:63-66), else it starts a new cluster.  Clusters never merge.  Kept clusters:
 *   size > min_size (:263).  Rectangle: the members converted with cvRound (round half to even),
 *   then (xmin, ymin, xmax - xmin + 1, ymax - ymin + 1); coordinates beyond +-2^30 give unspecified
 *   rectangles.
 *   points [npoints][2] float host, input order.
 * Outputs (any may be NULL):
 *   labels   [npoints] index of the point's cluster among ALL clusters, creation order
 *   num_all  number of all clusters
 *   kept     [<= max_kept] ids (into the above) of clusters with size > min_size, ascending
 *   rects    [<= max_kept][4] x, y, width, height of each kept cluster
 *   num_kept number of kept clusters (may exceed max_kept; only max_kept are written)
 * npoints == 0 is MDX_OK with zero clusters.  MDX_EINVAL: npoints or max_kept negative, npoints >
 * MDX_CLUSTER_MAX_POINTS, points NULL with npoints > 0, a non-finite coordinate (the reference's
 * behaviour there is an accident of NaN compares), a NaN distance_threshold.  A threshold <= 0 is
 * valid: every point is its own cluster.  All pair distances are computed on the device
 * (ceil(npoints / 256) launches); cluster sizes, ranks and rectangles are O(npoints) on the host
 * after the call's one synchronising copy.  Synchronous.
 */
#define MDX_CLUSTER_MAX_POINTS 262144
int mdx_cluster_euclidean(mdx_ctx* ctx, const float* points, int npoints, double distance_threshold,
                          int min_size /* reference: 5 */, int32_t* labels, int* num_all,
                          int32_t* kept, int32_t* rects, int max_kept, int* num_kept);

/*
 * First-fit clustering of flow vectors by distance and angle, and bounding rectangles (DESIGN.md
 * §7g): replaces FlowClusterer::getClusters (common/src/flow_clusterer.cpp:178-227), which the node
 * runs on the last trajectory pass's Vec4d image when egomotion is off
 * (motion_detection_node.cpp:375), and boundingRect of each kept cluster (:376-395).  Restated from
 * the source; unpinned against a real build (no OpenCV 2.4 to compare with).
 *   vectors [n][4] double host, (x, y, dx, dy) each, in the order the reference visits them: image
 *   rows outer, columns inner, both stepping pixel_step (:180-184) -- y-major, NOT the x-major grid
 *   order of the flow entries above; the caller does that gather.
 *   A vector is active iff fabs(dx) > 0 || fabs(dy) > 0 (:185); the others are skipped (label -1).
 *   Pair tests of an active vector i and an earlier active vector j:
 *     N(i, j)  sqrt((xi-xj)*(xi-xj) + (yi-yj)*(yi-yj)) < distance_threshold, all in double, each
 *              operation rounded (vector_cluster.cpp:118-121).  Exact.
 *     G(i, j)  the angular distance below angular_threshold.  Each vector's angle is atan2(dy, dx),
 *              plus 2 pi when negative (:131-139), by the host's libm; the distance is
 *              w = |angle_i - angle_j|, and 2 pi - w where w > pi (pi = M_PI, 2 pi = 2 * M_PI as
 *              doubles).  That is what the reference's |atan2(sin d, cos d)| (:123-129) computes, to
 *              within a few ulp: a decision closer than that to the threshold may differ from a
 *              reference build.
 *     MDX_VCLUSTER_ABS_INT  the reference calls unqualified abs on that double (:43).  Where only
 *              int abs(int) is in scope (<cmath> included, no global abs(double): the 2014 toolchain
 *              the reference was written with) the distance is truncated toward zero first: G is
 *              trunc(w) < angular_threshold, which for a threshold in (0, 1] is w < 1.  Without the
 *              flag (the default): fabs, what was meant and what a current libstdc++ resolves to.
 *   Assignment (:189-204), first fit with split minima: vector i joins the EARLIEST-created cluster
 *   that has some earlier member j with N(i, j) and some earlier member j' with G(i, j') -- j' need
 *   not be j (getClosestDistance and getClosestOrientation are separate minima over the cluster) --
 *   and starts a new cluster when none qualifies.  Not the nearest cluster, unlike
 *   mdx_cluster_euclidean.  Clusters never merge.  Kept clusters: size > min_size (:213).
 *   Rectangle: the members' (x, y) converted to float (node.cpp:382), then exactly
 *   mdx_cluster_euclidean's rectangle.
 * Outputs (any may be NULL):
 *   labels     [n] index of the vector's cluster among ALL clusters, creation order; -1 inactive
 *   num_active number of active vectors
 *   num_all    number of all clusters
 *   kept       [<= max_kept] ids (into the above) of clusters with size > min_size, ascending
 *   rects      [<= max_kept][4] x, y, width, height of each kept cluster
 *   num_kept   number of kept clusters (may exceed max_kept; only max_kept are written)
 * n == 0, or no active vector, is MDX_OK with zero clusters.  MDX_EINVAL: a null context; n or
 * max_kept negative; n > MDX_VCLUSTER_MAX_POINTS; vectors NULL with n > 0; a non-finite component; a
 * NaN threshold; unknown flag bits.  A threshold <= 0 is valid: every active vector is its own
 * cluster.  Every pair test and the first-fit resolution run on the device (3 * ceil(active / 256) - 1
 * launches); angles, compaction, sizes, ranks and rectangles are O(n) on the host around the call's
 * one synchronising copy.  Scratch belongs to the context and only grows.  Synchronous.
 */
#define MDX_VCLUSTER_ABS_INT 1
#define MDX_VCLUSTER_MAX_POINTS 131072   /* covers 4K at pixel_step 10 (82,944) */
int mdx_cluster_vectors(mdx_ctx* ctx, const double* vectors, int n, double distance_threshold,
                        double angular_threshold, int min_size /* reference: 5 */, int flags, int32_t* labels,
                        int* num_active, int* num_all, int32_t* kept, int32_t* rects, int max_kept,
                        int* num_kept);

/*
 * Convex hulls of clusters: replaces cv::convexHull of every kept cluster in
 * showClusterContours (common/src/optical_flow_visualizer.cpp:204-221; showFlowClusters :123-135
 * takes the same hull), which the node calls after clusterEuclidean / getClusters
 * (motion_detection_node.cpp:393 live, :510 run()) and whose hulls MotionLogger::writeContour
 * would log (:426-429, commented out in the reference).
 *   points [n][2] float host and labels [n]: the members and the cluster of each, as
 *   mdx_cluster_euclidean returns `labels`; for mdx_cluster_vectors' clusters pass (float)x, (float)y
 *   of every vector (node.cpp:382) with its `labels`.  ids [k]: the clusters wanted, strictly
 *   ascending -- what those entries return as `kept`, or any subset.  Members whose label is not in
 *   ids, and label -1, take no part.
 *   Conversion: cv::Mat(cluster).copyTo(vector<cv::Point>), exactly mdx_cluster_euclidean's for the
 *   rectangles: cvRound, half to even, float -> int32.
 *   Vertices: the extreme points of the converted set.  Duplicates count once; a point on the
 *   segment between two other members is not a vertex (collinear boundary points are excluded).  One
 *   distinct point gives 1 vertex, members that are all collinear give the 2 end points.
 *   Order: cv::convexHull(.., clockwise=false) -- counter-clockwise in a frame whose y axis points
 *   up.  The first vertex is the lexicographically greatest (greatest x, then greatest y); the hull
 *   runs along its max-y side to the lexicographically smallest vertex and along its min-y side
 *   back.  Not closed: the first vertex is not repeated.
 *   The vertex set is determined mathematically.  The start and the orientation are restated from
 *   OpenCV 2.4's documentation and source as recalled and, like the entries above, unpinned against
 *   a real build (no OpenCV to compare with).  All arithmetic is integer and exact; no tolerance
 *   exists anywhere.  Cross products are taken in int64, so converted coordinates are limited to
 *   |v| <= 2^29 (differences <= 2^30, products <= 2^60).
 * Outputs:
 *   offsets      [k+1] hull j's vertices are xy[offsets[j] .. offsets[j+1]); always complete
 *   xy           [<= max_vertices][2] int32 x, y: the first max_vertices vertices of the hulls, packed
 *                in the order of ids (may be NULL when max_vertices is 0)
 *   num_vertices (may be NULL) all vertices = offsets[k]; may exceed max_vertices
 * k == 0 or n == 0 is MDX_OK with all offsets zero.  MDX_EINVAL: a null context; n, k or max_vertices
 * negative; n > MDX_CLUSTER_MAX_POINTS; a needed pointer NULL (offsets; points and labels with n > 0; ids
 * with k > 0; xy with max_vertices > 0); ids not strictly ascending, or negative; an id with no
 * member; a non-finite coordinate (of any member); a converted coordinate of a taking-part member
 * beyond +-2^29; a requested cluster spanning more than MDX_HULL_MAX_SPAN pixel columns (8192 covers
 * an 8K frame).  The host groups the members by cluster, O(n log k); the column extremes, the chains
 * and the vertex order are the device's, one workgroup per cluster and one launch per call, with no
 * size limit per cluster below MDX_CLUSTER_MAX_POINTS.  Scratch belongs to the context and only
 * grows.  Synchronous.  There is no CPU fallback.
 */
#define MDX_HULL_MAX_SPAN 8192
int mdx_cluster_hulls(mdx_ctx* ctx, const float* points, const int32_t* labels, int n, const int32_t* ids, int k,
                      int32_t* offsets, int32_t* xy, int max_vertices, int* num_vertices);

/*
 * Flow-vector outliers by median and median absolute deviation: replaces
 * OutlierDetector::findOutliers and getOutlierVectors (common/src/outlier_detector.cpp:37-186), the
 * pair path's detector, which the node would run on calculateOpticalFlow's Vec4d image in front of
 * getClusters (MotionDetectionNode::detectOutliers, motion_detection_node.cpp:112-160).  Restated
 * from the source; unpinned against a real build.
 *   vectors [batch][n][4] double host, (x, y, dx, dy) each, one per grid point.  The statistics do not
 *   depend on the order; pass the order getClusters visits (image rows outer) so that the flags line
 *   up with what mdx_cluster_vectors is given next.
 *   Selected set S: every vector under MDX_OUTLIERS_INCLUDE_ZEROS (:130-133), else the vectors with
 *   fabs(dx) > 0 || fabs(dy) > 0 (:134).  m = |S|.
 *   Channels (:73-95): the angle atan2(dy, dx), not wrapped (vectors pointing near +pi and -pi are far
 *   apart: the reference's quirk, kept), by the host's libm; the magnitude sqrt(dy*dy + dx*dx), every
 *   operation rounded, none fused.
 *   Per channel (createMask, :120-186): the median of S's values (getMedian, :97-119: the element at
 *   (m-1)/2 of the sorted values for odd m, (v[m/2-1] + v[m/2]) / 2.0 for even m); diff = fabs(value -
 *   median); MAD = the same median of the diffs; a vector of S is flagged iff
 *   fabs(0.6745 * diff / MAD) > 3.5, evaluated left to right (a rounded multiply, then an IEEE
 *   division).  MAD = 0: a positive diff gives +inf and is flagged, a zero diff gives NaN and is not.
 *   m == 0: nothing is flagged (:140-143).  Vectors outside S are never flagged.
 *   A vector is an outlier iff either channel flags it.
 * Outputs (any may be NULL):
 *   out_flags       [batch][n] bit 0: flagged by the angle, bit 1: by the magnitude (kept apart so that
 *                   a wrong channel cannot hide behind the other one's flag)
 *   outlier_vectors [batch][n][4] getOutlierVectors (:55-71): the input with every non-outlier
 *                   replaced by (0, 0, 0, 0)
 *   stats           [batch] counts and the four order statistics; all 0 when m == 0.  std::sort leaves
 *                   the order of -0.0 and +0.0 open, so a median that is zero is specified as a value,
 *                   not by the sign of its zero; no flag depends on that sign.
 * Given the host's angles every output is exact: the squares, their sum, the root, all four
 * selections, the diffs, the z-score and the compare run on the device with explicitly rounded
 * operations, denormals kept; one launch for the whole batch, one workgroup per field.
 * n == 0 or batch == 0 is MDX_OK.  MDX_EINVAL: a null context; negative batch or n; n >
 * MDX_OUTLIERS_MAX_POINTS; unknown flag bits; vectors NULL while batch * n > 0; a non-finite component;
 * |dx| or |dy| >= 1e150 (the square must not overflow: inf - inf would put a NaN into the reference's
 * sort, which is undefined).  Scratch belongs to the context and only grows.  Synchronous.
 */
typedef struct {            /* 48 bytes */
    int32_t selected;       /* m */
    int32_t flagged_angle, flagged_magnitude, outliers;
    double  median_angle, mad_angle, median_magnitude, mad_magnitude;   /* 0 when m == 0 */
} mdx_outlier_stats;
#define MDX_OUTLIERS_INCLUDE_ZEROS 1
#define MDX_OUTLIERS_MAX_POINTS 131072   /* the cap of mdx_cluster_vectors */
int mdx_find_outliers(mdx_ctx* ctx, const double* vectors, int batch, int n, int flags, uint8_t* out_flags,
                      double* outlier_vectors, mdx_outlier_stats* stats);

/*
 * The motion mask labelled into regions: the pair path's mask turned into
 * detections on the device, by the reference's own recipe for a mask,
 * BackgroundSubtractor::getMotionContours (common/src/background_subtractor.cpp:31-35: cv::erode then
 * cv::dilate with the default 3x3 element, then findContours' 8-connected foreground blobs), each
 * blob reduced to its boundingRect (optical_flow_visualizer.cpp:230-236).  Restated from the source;
 * unpinned against a real build (no OpenCV 2.4 to compare with).
 *   Foreground: a mask byte != 0.
 *   Opening (flags & MDX_REGIONS_OPEN3): E(x, y) = 1 iff every in-image pixel of the 3x3
 *   neighbourhood of (x, y), itself included, is foreground; D(x, y) = 1 iff some in-image pixel of
 *   the 3x3 neighbourhood has E = 1 (out-of-image neighbours never erode and never dilate:
 *   morphologyDefaultBorderValue, one iteration, centre anchor).  Without the flag D is the
 *   foreground itself.
 *   Components: the 8-connected components of D, ordered by the raster index y*w + x of their first
 *   pixel.  Nested components are all reported here: findContours' RETR_EXTERNAL drops a blob that
 *   lies inside another blob's hole, and mdx_region_parents_dev (below) makes that cut on the device.
 *   Record: x, y, width, height = (xmin, ymin, xmax - xmin + 1, ymax - ymin + 1), as
 *   mdx_cluster_euclidean's rects; area = pixel count; seed_x, seed_y = the first pixel; id = the
 *   component's index among ALL components.
 *   Kept: area >= min_area (min_area <= 1 keeps every component), listed in ascending id.
 * mdx_mask_regions_dev is asynchronous on the context stream and never synchronises with the host:
 * it chains behind mdx_flow_warp_diff_batch_dev on that call's d_mask with no round trip, and it
 * honours mdx_input_ready like the other device entries.  Every pointer is a device pointer; any
 * output may be NULL.  num_kept may exceed max_regions: only max_regions records per mask are
 * written and nothing past them is touched.  The input mask is never modified (d_mask_out must not
 * overlap it).  Scratch belongs to the context, is a function of (batch, w, h) alone (about 9 bytes
 * per pixel) and only grows: no allocation after the first call at a given (batch, w, h).
 * MDX_EINVAL: a null context; batch < 1; w or h < 1; stride < w; frame_stride < h*stride;
 * w*h > 2^30; max_regions < 0; d_regions NULL with max_regions > 0; unknown flag bits;
 * d_mask_out == d_mask.
 */
#define MDX_REGIONS_OPEN3 1
typedef struct mdx_region { int32_t x, y, width, height, area, seed_x, seed_y, id; } mdx_region;  /* 32 bytes */
int mdx_mask_regions_dev(mdx_ctx* ctx, int batch, const uint8_t* d_mask, int w, int h, int stride,
                         size_t frame_stride, int flags, int min_area,
                         mdx_region* d_regions /* [batch][max_regions] or NULL */, int max_regions,
                         int32_t* d_num_all /* [batch] or NULL */, int32_t* d_num_kept /* [batch] or NULL */,
                         int32_t* d_labels /* [batch][h][w]: id among ALL components, -1 background; or NULL */,
                         uint8_t* d_mask_out /* [batch][h][w] D as 0/255, row pitch w; or NULL */);
/* The same for one mask in host memory, synchronous; same outputs (any may be NULL), same errors. */
int mdx_mask_regions(mdx_ctx* ctx, const uint8_t* mask, int w, int h, int stride, int flags, int min_area,
                     mdx_region* regions, int max_regions, int* num_all, int* num_kept,
                     int32_t* labels, uint8_t* mask_out);

/*
 * Convex hulls of the mask regions: the second thing the node takes from a blob next
 * to its boundingRect (cv::convexHull, optical_flow_visualizer.cpp:204-240), for the regions of
 * mdx_mask_regions_dev, on the device.  The hull of a blob's contour is the hull of its pixels, so
 * the vertex set is determined mathematically.
 *   Inputs: what mdx_mask_regions_dev wrote -- d_labels, d_regions and d_num_kept.  Per image b the
 *   first r = min(max(num_kept[b], 0), max_regions) records take part.
 *   Members of record j: the pixels (x, y) inside the record's rectangle whose label equals the
 *   record's id.  The rectangle is clamped to the frame first: the entry cannot validate device
 *   records and never touches memory outside the frame because of one.  Pixels of other regions inside
 *   the rectangle (nested or interleaved blobs) take no part.  A record whose id matches no pixel
 *   gives 0 vertices.  A nested blob's hull is reported like any other (for the external blobs only,
 *   pass mdx_region_parents_dev's d_external and d_num_external).  This entry gives the hull only; the
 *   contour polyline itself is mdx_region_outlines_dev's (below).  (A record edited so that its area
 *   understates its members may have its hull cut short at min(area, 2*width, 2*height) vertices.)
 *   Vertices, order, start: mdx_cluster_hulls' contract, minus the conversion (members are integers
 *   already).  Extreme points only: collinear boundary points are excluded, one pixel gives 1 vertex,
 *   a straight run its 2 end points.  The first vertex is the lexicographically greatest (greatest x,
 *   then greatest y); the hull runs along its max-y side to the lexicographically smallest vertex and
 *   along its min-y side back.  Not closed.  As there, the start and the orientation are restated from
 *   OpenCV 2.4's documentation and unpinned against a real build.  Integer and exact throughout.
 * Outputs:
 *   d_offsets      [batch][max_regions + 1] hull j's vertices are xy[b][offsets[b][j] ..
 *                  offsets[b][j+1]); always complete and monotone, entries past r repeat the total
 *   d_xy           [batch][max_vertices][2] int32 x, y: the first max_vertices vertices of image b,
 *                  packed in record order; nothing past them is written, and nothing at all when
 *                  max_vertices is 0 (d_xy may then be NULL)
 *   d_num_vertices [batch] (may be NULL) offsets[b][r]; may exceed max_vertices
 * mdx_region_hulls_dev is asynchronous on the context stream and never synchronises with the host: it
 * chains behind mdx_mask_regions_dev (itself behind mdx_flow_warp_diff_batch_dev) with no round trip,
 * and it honours mdx_input_ready like the other device entries.  Every pointer is a device pointer.
 * Three launches per call for any batch up to 65,535 images (a per-image scan of the records' vertex
 * bounds, one workgroup per record, a per-image scan of the counts that packs xy); no workgroup waits
 * for another.  max_regions == 0 is MDX_OK with offsets[b][0] = 0 and num_vertices[b] = 0.
 * Scratch belongs to the context, is a function of (batch, w, h, max_regions) alone and only grows:
 *   batch * (12 * max_regions + 8 * min(w*h, 2*min(w, h)*max_regions)) bytes (+ 255 of alignment)
 * -- per record a staging slice and a count, per image a staging block that holds every hull, a hull
 * having at most min(area, 2*width, 2*height) vertices.  No allocation after the first call at a
 * given (batch, w, h, max_regions).
 * MDX_EINVAL: a null context; batch < 1; w or h < 1; w*h > 2^30; w > MDX_HULL_MAX_SPAN (8192 covers an
 * 8K frame); max_regions < 0 or max_vertices < 0; d_labels or d_offsets NULL; d_regions or d_num_kept
 * NULL with max_regions > 0; d_xy NULL with max_vertices > 0.
 */
int mdx_region_hulls_dev(mdx_ctx* ctx, int batch, const int32_t* d_labels /* [batch][h][w] */, int w, int h,
                         const mdx_region* d_regions /* [batch][max_regions] */, int max_regions,
                         const int32_t* d_num_kept /* [batch] */,
                         int32_t* d_offsets /* [batch][max_regions + 1] */,
                         int32_t* d_xy /* [batch][max_vertices][2] or NULL */, int max_vertices,
                         int32_t* d_num_vertices /* [batch] or NULL */);
/* mdx_mask_regions and the hulls of its records for one mask in host memory, synchronous: the label
 * image stays on the device and never crosses PCIe; of xy only the min(offsets[r], max_vertices)
 * vertices that exist are copied back.  regions, num_all, num_kept as mdx_mask_regions; offsets, xy,
 * num_vertices as above for one image.  Errors: mdx_mask_regions', plus w > MDX_HULL_MAX_SPAN, negative
 * max_vertices, NULL offsets, NULL xy with max_vertices > 0. */
int mdx_mask_region_hulls(mdx_ctx* ctx, const uint8_t* mask, int w, int h, int stride, int flags, int min_area,
                          mdx_region* regions, int max_regions, int* num_all, int* num_kept,
                          int32_t* offsets /* [max_regions + 1] */, int32_t* xy, int max_vertices, int* num_vertices);

/*
 * The parent blob of each mask region, and findContours' RETR_EXTERNAL filter: the
 * reference's getMotionContours asks for CV_RETR_EXTERNAL (background_subtractor.cpp:31-35), which
 * keeps the blobs that lie in no other blob's hole.  Which blob encloses which follows from the label
 * image alone; integer and exact.  Restated, and unpinned against a real build like the rest of the
 * recipe (OpenCV 2.4's findContours is also said to clear the frame's outermost ring of pixels before
 * it traces; neither mdx_mask_regions_dev nor this entry does that).
 *   Inputs: what mdx_mask_regions_dev wrote -- d_labels, d_regions and d_num_kept; the mask is not
 *   needed.  Per image b the first r = min(max(num_kept[b], 0), max_regions) records take part.
 *   Background: the pixels with a label < 0, together with everything outside the frame.  Its
 *   components are 4-connected (the dual of the 8-connected foreground).  The component that holds
 *   the outside of the frame is the frame background: any background pixel of the frame's first or
 *   last row or column belongs to it.  Every other background component is a hole; a hole never
 *   touches the frame's edge.
 *   Enclosing background of a blob C: the background component of the pixel directly above C's seed,
 *   (seed_x, seed_y - 1); the frame background when seed_y == 0.  (That pixel is background because
 *   the seed is C's first pixel in raster order, and it lies in none of C's own holes: those are closed
 *   in by pixels of C and so lie below C's top row.)
 *   Parent: MDX_REGION_NO_PARENT (-1, C is external) when the enclosing background is the frame
 *   background; otherwise the id, among ALL components, of the pixel directly above the hole's first
 *   pixel in raster order.  (That pixel exists, is foreground, and belongs to the blob whose hole this
 *   is: an island inside the hole lies strictly below the hole's top row.)  The parent may be a
 *   component that min_area or max_regions left out of the records.
 *   Records the entry cannot trust (d_regions is device memory a caller may have edited): a record
 *   gets MDX_REGION_PARENT_UNKNOWN (-2) and is not external when its seed lies outside the frame, its
 *   seed pixel does not carry the record's id, or the pixel above its seed is not background.  No
 *   access outside the frame ever results from a record.
 * Outputs (each may be NULL):
 *   d_parent       [batch][max_regions] the parent of each participating record
 *   d_external     [batch][max_regions] the records with parent -1, in record order: what RETR_EXTERNAL
 *                  keeps.  Only the first num_external[b] entries of image b are written.
 *   d_num_external [batch] how many those are
 * Entries of d_parent and d_external past the r participating records are not touched.
 * mdx_region_parents_dev is asynchronous on the context stream and never synchronises with the host:
 * it chains behind mdx_mask_regions_dev with no round trip, mdx_region_hulls_dev chains behind it on
 * d_external / d_num_external in place of d_regions / d_num_kept (the hulls of the external blobs only),
 * and it honours mdx_input_ready like the other device entries.  Every pointer is a device pointer.
 * Five launches per call for any batch up to 65,535 images (the background labelled per 64 x 32 tile,
 * the tiles joined straight across their borders, the tile roots flattened, then every pixel; one
 * workgroup per image resolves the records); no workgroup waits for another.  max_regions == 0 is
 * MDX_OK with num_external[b] = 0.
 * Scratch belongs to the context, is a function of (batch, w, h) alone and only grows:
 *   batch * 5 * w * h bytes (+ 510 of alignment)
 * -- per pixel the background's 4-byte parent word and a mark byte; nothing is cleared between calls.
 * No allocation after the first call at a given (batch, w, h).
 * MDX_EINVAL: a null context; batch < 1; w or h < 1; w*h > 2^30; max_regions < 0; d_labels NULL;
 * d_regions or d_num_kept NULL with max_regions > 0; d_external overlapping d_regions.
 */
#define MDX_REGION_NO_PARENT (-1)
#define MDX_REGION_PARENT_UNKNOWN (-2)
int mdx_region_parents_dev(mdx_ctx* ctx, int batch, const int32_t* d_labels /* [batch][h][w] */, int w, int h,
                           const mdx_region* d_regions /* [batch][max_regions] */, int max_regions,
                           const int32_t* d_num_kept /* [batch] */,
                           int32_t* d_parent /* [batch][max_regions] or NULL */,
                           mdx_region* d_external /* [batch][max_regions] or NULL; must not overlap d_regions */,
                           int32_t* d_num_external /* [batch] or NULL */);
/* mdx_mask_regions, the parents of its records and, when offsets is given, the hulls of its EXTERNAL
 * records for one mask in host memory, synchronous: the label image stays on the device and never
 * crosses PCIe.  regions, num_all, num_kept as mdx_mask_regions (every kept record, nested or not);
 * parent [max_regions]: the first min(num_kept, max_regions) entries are written; external_index
 * [max_regions]: external_index[i] is the position in `regions` of the i-th external record, the first
 * num_external entries are written (either array may be NULL).  offsets (NULL: no hulls; xy,
 * max_vertices and num_vertices are then ignored), xy, num_vertices: mdx_mask_region_hulls' contract with
 * the external records in place of the kept ones, hull i belonging to regions[external_index[i]].
 * Errors: mdx_mask_regions', plus with offsets given mdx_mask_region_hulls'. */
int mdx_mask_regions_tree(mdx_ctx* ctx, const uint8_t* mask, int w, int h, int stride, int flags, int min_area,
                          mdx_region* regions, int max_regions, int* num_all, int* num_kept,
                          int32_t* parent /* [max_regions] */, int32_t* external_index /* [max_regions] */,
                          int* num_external,
                          int32_t* offsets /* [max_regions + 1] or NULL */, int32_t* xy, int max_vertices,
                          int* num_vertices);

/*
 * Outer border polylines of the mask regions: what getMotionContours' cv::findContours(mask,
 * contours, CV_RETR_EXTERNAL, CV_CHAIN_APPROX_NONE) itself returns for a blob -- the ordered list of its
 * border pixels -- for the regions of mdx_mask_regions_dev, on the device.  Restated from the published
 * border-following algorithm and OpenCV 2.4's behaviour; unpinned against a real build, like the rest of
 * the recipe.  Like the other region entries it does not clear the frame's outermost ring of pixels.
 *   Inputs: what mdx_mask_regions_dev wrote -- d_labels, d_regions and d_num_kept.  Per image b the first
 *   r = min(max(num_kept[b], 0), max_regions) records take part.
 *   Directions: d = 0..7 are E, NE, N, NW, W, SW, S, SE.  In that order D[d] = (1,0), (1,-1), (0,-1),
 *   (-1,-1), (-1,0), (-1,1), (0,1), (1,1), with x to the right and y down.  Increasing d runs
 *   counter-clockwise on the screen.
 *   Members of record j: the in-frame pixels whose label equals the record's id.  Everything else counts
 *   as background: other regions, label < 0, and the outside of the frame.
 *   The tracing rule.
 *     Start: p0 = (seed_x, seed_y).  Look at p0's neighbours in the order d = 3, 2, 1, 0, 7, 6, 5, 4, which
 *     runs clockwise from just past W.  The first member found is i1, in direction b0.
 *     No neighbour: if p0 has no member neighbour, the outline is the single point p0.
 *     Step: a state is (p, b).  p is a member, and b is the direction from p back to the pixel it was
 *     entered from.  For the first step, p = p0 and b = b0.  The next pixel is q = p + D[t], where t is the
 *     first of b+1, b+2, .., b+8 (mod 8) with p + D[t] a member.  The next state is (q, t xor 4).
 *     Outline: the p of every state from (p0, b0) onward, in order.  It ends with the state whose
 *     successor is (p0, b0) again.  That state is the step from i1 back to p0, and it is included.
 *     Shape of the result: p0 comes first and is not repeated at the end.  A pixel on a one-pixel-wide
 *     strand appears once per pass: a 3 x 1 line gives (0,0), (1,0), (2,0), (1,0).  A 2 x 2 square gives
 *     (0,0), (0,1), (1,1), (1,0): from the seed it runs down the blob's left side, counter-clockwise on
 *     the screen.
 *     Scope: only the outer border is traced.  Holes are never traced, which is RETR_EXTERNAL with
 *     CHAIN_APPROX_NONE.  A nested blob's outline is reported like any other record's; for the external
 *     blobs only, pass mdx_region_parents_dev's d_external / d_num_external, as with the hulls.
 *   Records the entry cannot trust (d_regions is device memory a caller may have edited): a record gives 0
 *   points if its seed lies outside the frame or its seed pixel does not carry its id (a negative id is
 *   carried by no pixel: label < 0 is background).  A record's seed may be a member but not the
 *   component's first pixel; it then gives the cycle of the rule from that seed.  That cycle is well
 *   defined and finite, though it has no meaning.  (Such a record, and records that share a start or a
 *   cycle, are traced by one device lane each: exact, but slow.)  No access outside the frame ever
 *   results from a record.
 * Outputs:
 *   d_offsets    [batch][max_regions + 1] outline j's points are xy[b][offsets[b][j] .. offsets[b][j+1]);
 *                always complete and monotone, entries past r repeat the total
 *   d_xy         [batch][max_points][2] int32 x, y: the first max_points points of image b, packed in
 *                record order; nothing past them is written, and nothing at all when max_points is 0
 *                (d_xy may then be NULL)
 *   d_num_points [batch] (may be NULL) offsets[b][r]; may exceed max_points
 * mdx_region_outlines_dev is asynchronous on the context stream and never synchronises with the host: it
 * chains behind mdx_mask_regions_dev / mdx_region_parents_dev with no round trip, and it honours
 * mdx_input_ready like the other device entries.  Every pointer is a device pointer.  No workgroup waits
 * for another.  max_regions == 0 is MDX_OK with offsets[b][0] = 0 and num_points[b] = 0 (one launch).
 * How: the rule is a bijection on the states (p, b) with p and p + D[b] members, so an outline is one
 * cycle of a permutation, and list ranking -- pointer jumping over each state's predecessor -- finds every
 * state's position in it.  Only pixels with a non-member 4-neighbour carry states, at most 7 each.  No
 * state occurs twice in an outline, so a position is below 7*w*h, the proven bound used here: the call
 * queues 7 + R launches, R = ceil(log2(7*w*h)) rounds of jumping (24 at 1080p, 26 at 4K), for any batch up
 * to 65,535 images; a round that follows one in which no state of an image reached its start returns at
 * once for that image.
 * Scratch belongs to the context, is a function of (batch, w, h) alone (max_regions takes no part) and
 * only grows; nothing in it is cleared between calls:
 *   batch * (61 * w*h + 4 * ceil(w*h / 256) + 260) bytes (+ 765 of alignment)
 * -- per pixel 7 state words of 8 bytes (the worst case: the ranking runs where the states are, but the
 * room for them cannot depend on the image), the 4-byte index of its first state and its neighbour mask
 * byte.  That is 4.0 GB for 32 x 1080p and for 8 x 4K; allocation failure is MDX_ENOMEM.  No allocation
 * after the first call at a given (batch, w, h).
 * MDX_EINVAL: a null context; batch < 1; w or h < 1; w*h > 2^28 (state indices are 31-bit: this design's
 * limit, in place of the hulls' MDX_HULL_MAX_SPAN, which does not apply); max_regions < 0 or
 * max_points < 0; d_labels or d_offsets NULL; d_regions or d_num_kept NULL with max_regions > 0; d_xy NULL
 * with max_points > 0.
 */
int mdx_region_outlines_dev(mdx_ctx* ctx, int batch, const int32_t* d_labels /* [batch][h][w] */, int w, int h,
                            const mdx_region* d_regions /* [batch][max_regions] */, int max_regions,
                            const int32_t* d_num_kept /* [batch] */,
                            int32_t* d_offsets /* [batch][max_regions + 1] */,
                            int32_t* d_xy /* [batch][max_points][2] or NULL */, int max_points,
                            int32_t* d_num_points /* [batch] or NULL */);
/* mdx_mask_regions and the outlines of its records for one mask in host memory, synchronous: the label
 * image stays on the device and never crosses PCIe; of xy only the min(offsets[r], max_points) points that
 * exist are copied back.  regions, num_all, num_kept as mdx_mask_regions.  With parent, external_index and
 * num_external all NULL every kept record is outlined, outline j belonging to regions[j].  With any of
 * the three given, they are filled as by mdx_mask_regions_tree and the EXTERNAL records are outlined,
 * outline i belonging to regions[external_index[i]].  offsets, xy, num_points as above for one image.
 * Errors: mdx_mask_regions', plus w*h > 2^28, negative max_points, NULL offsets, NULL xy with
 * max_points > 0. */
int mdx_mask_region_outlines(mdx_ctx* ctx, const uint8_t* mask, int w, int h, int stride, int flags, int min_area,
                             mdx_region* regions, int max_regions, int* num_all, int* num_kept,
                             int32_t* parent /* [max_regions] */, int32_t* external_index /* [max_regions] */,
                             int* num_external,   /* all three NULL: every kept record */
                             int32_t* offsets /* [max_regions + 1] */, int32_t* xy, int max_points, int* num_points);

/*
 * Background subtraction (ABI 11): the head of the reference's
 * BackgroundSubtractor::getMotionContours (common/src/background_subtractor.cpp:27-28) --
 * cv::BackgroundSubtractorMOG2::operator() and getBackgroundImage as OpenCV 2.4's bgfg_gaussmix2.cpp
 * (MOG2Invoker, detectShadowGMM) computes them.  Restated from the published source, unpinned against a
 * real build.  A model is a per-pixel mixture of up to nmixtures Gaussians, kept on the device; the mask
 * it writes (0 background, shadow_value shadow, 255 foreground) is a valid d_mask for mdx_mask_regions_dev,
 * which treats any non-zero byte as foreground, so frame -> mask -> opening -> external outlines runs with
 * no round trip.
 *
 * Arithmetic: IEEE binary32, no contraction, operations in the order written, division correctly rounded.
 * Per call: nframes++; learning_rate < 0: alphaT = (float)(1.0 / min(2 * nframes, history)) (in double);
 * learning_rate >= 0 and nframes > 1: alphaT = (float)learning_rate; on frame 1 alphaT =
 * (float)(1.0 / min(2, history)) whatever the rate.  alpha1 = 1.f - alphaT; prune = -alphaT * ct.
 * Per pixel, data[c] = (float)byte, state modes and per mode m weight[m], variance[m], mean[m][c]:
 *   1  n = n0 = modes, fits = background = false, total = 0.f
 *   2  for (m = 0; m < n; m++)                 -- n is re-read and may shrink inside the loop
 *        w = alpha1 * weight[m] + prune; swaps = 0
 *        if (!fits)  var = variance[m]; d[c] = mean[m][c] - data[c]; dist2 = d0*d0 + d1*d1 + d2*d2 (left to
 *                    right; one channel: d0*d0)
 *                    if (total < TB && dist2 < Tb * var) background = true
 *                    if (dist2 < Tg * var)  fits = true; w += alphaT; k = alphaT / w; mean[m][c] -= k * d[c];
 *                        vn = var + k * (dist2 - var); vn = vn > var_min ? vn : var_min;
 *                        vn = vn < var_max ? vn : var_max; variance[m] = vn;
 *                        for (i = m; i > 0; i--) { if (w < weight[i-1]) break; swaps++; swap modes i, i-1 }
 *        if (w < -prune) { w = 0.f; n--; }
 *        weight[m - swaps] = w; total += w
 *   3  total = 1.f / total; for (m < n) weight[m] *= total; n = n0 (a pruned mode stays, with weight 0)
 *   4  if (!fits)  m = (n == nmixtures) ? nmixtures - 1 : n++
 *                  n == 1: weight[m] = 1.f; else weight[m] = alphaT and weight[i] *= alpha1 for i < n - 1
 *                  mean[m][c] = data[c]; variance[m] = var_init
 *                  for (i = n - 1; i > 0; i--) { if (alphaT < weight[i-1]) break; swap modes i, i-1 }
 *   5  modes = n; mask = background ? 0 : (detect_shadows && shadow()) ? shadow_value : 255
 * shadow(), on the updated state, tw = 0.f, for (m < n):
 *        num = sum_c data[c] * mean[m][c], den = sum_c mean[m][c]^2 (both from 0.f, in channel order)
 *        if (den == 0) return false
 *        if (num <= den && num >= tau * den)  a = num / den; s = sum_c (a * mean[m][c] - data[c])^2 from 0.f;
 *                                             if (s < Tb * variance[m] * a * a) return true   (left to right)
 *        tw += weight[m]; if (tw > TB) return false
 *      return false
 * Background image, per pixel: for (m < modes) { acc[c] += weight[m] * mean[m][c] (from 0.f); tot += weight[m];
 * if (tot > TB) break; }  acc[c] *= (1.f / tot); the byte is acc[c] clamped to [0, 255] (a NaN gives 0) and
 * rounded half to even; modes == 0 gives 0.  (2.4 asserts three channels there; one channel follows the same
 * rule and is an extension.)
 * A NaN in the state (learning_rate 1 makes them: step 3 multiplies a weight 0 by 1 / 0) is held as
 * 0x7fc00000: IEEE leaves a generated NaN's sign and payload open.  Nothing else depends on either.
 */
#define MDX_BG_MAX_MIXTURES 8
#define MDX_BG_MAX_FRAMES_PER_LAUNCH 32   /* mdx_bg_apply_dev splits a longer run of frames into launches */
typedef struct mdx_bg_params {   /* 48 bytes */
    int32_t history;             /* 500 */
    int32_t nmixtures;           /* 5; 1 .. MDX_BG_MAX_MIXTURES */
    float var_threshold;         /* Tb 16 */
    float var_threshold_gen;     /* Tg 9 */
    float background_ratio;      /* TB 0.9f; (0, 1] */
    float var_init;              /* 15 */
    float var_min;               /* 4 */
    float var_max;               /* 75 */
    float ct;                    /* 0.05f */
    int32_t detect_shadows;      /* 1 */
    int32_t shadow_value;        /* 127; 0 .. 255 */
    float tau;                   /* 0.5f; [0, 1] */
} mdx_bg_params;
typedef struct mdx_bg mdx_bg;
/* OpenCV 2.4's default constructor, which the reference uses (background_subtractor.h:23). */
void mdx_bg_default_params(mdx_bg_params* p);
size_t mdx_bg_params_size(void);
/* `streams` independent models of w x h pixels of `channels` (1 or 3) interleaved bytes; params NULL: the
 * defaults.  The model belongs to the context: mdx_bg_destroy frees it, and mdx_destroy frees the models
 * that never were.  Device memory: streams * w * h * (1 + 4 * nmixtures * (2 + channels)) bytes (101 B per
 * pixel at the defaults and 3 channels); MDX_ENOMEM when it does not fit.  A fresh model has no modes and has
 * seen no frame.
 * MDX_EINVAL (and *out untouched): a null context, params-with-null out; streams < 1 (or > 65,535); w or h < 1;
 * channels not 1 or 3; nmixtures outside [1, 8]; history < 1; a threshold, variance or ct that is negative or
 * not finite; var_min > var_max; background_ratio outside (0, 1]; tau outside [0, 1]; shadow_value outside
 * [0, 255]. */
int mdx_bg_create(mdx_ctx* ctx, int streams, int w, int h, int channels, const mdx_bg_params* params, mdx_bg** out);
int mdx_bg_destroy(mdx_ctx* ctx, mdx_bg* bg);
/* modes = 0 everywhere and nframes = 0 (queued on the context's stream). */
int mdx_bg_reset(mdx_ctx* ctx, mdx_bg* bg);
/* Frames the model has seen (every stream of a model sees the same number); negative on error. */
int mdx_bg_frames(mdx_ctx* ctx, mdx_bg* bg);
/* T consecutive frames of every stream, in one launch per 32 frames: a pixel's mixture is loaded once, carried
 * in registers through the launch's frames, and stored once, so replaying a recording pays the state's traffic
 * once per launch; T = 1 is the live case.  The outcome equals T calls with one frame each, bit for bit.
 * d_frames: stream s, frame t, row y at d_frames + s * stream_stride + t * frame_stride + y * stride, w *
 * channels bytes each, any alignment.  d_fgmask (may be NULL) [streams][T][h][w], packed; with T = 1 it is a
 * d_mask for mdx_mask_regions_dev with batch = streams, stride = w, frame_stride = w * h.
 * Asynchronous on the context's stream, never synchronises with the host, honours mdx_input_ready.
 * MDX_EHIP (a launch failed): with T > 32 the launches queued before the failing one stand -- the model and
 * mdx_bg_frames have advanced by a multiple of 32 frames, which mdx_bg_frames tells.
 * MDX_EINVAL (mask and model untouched): a null context, model or d_frames; a model of another context; T < 1;
 * stride < w * channels; with T > 1 a frame_stride below (h - 1) * stride + w * channels; with streams > 1 a
 * stream_stride below (T - 1) * frame_stride + (h - 1) * stride + w * channels; a learning_rate that is not
 * finite. */
int mdx_bg_apply_dev(mdx_ctx* ctx, mdx_bg* bg, int T, const uint8_t* d_frames, int stride, size_t frame_stride,
                     size_t stream_stride, double learning_rate, uint8_t* d_fgmask);
/* The background image of every stream, d_out [streams][h][w][channels]; asynchronous like the above. */
int mdx_bg_image_dev(mdx_ctx* ctx, mdx_bg* bg, uint8_t* d_out);
/* Synchronous conveniences for a model of one stream and frames in host memory (MDX_EINVAL for more
 * streams); fgmask [h][w] may be NULL, out is [h][w][channels]. */
int mdx_bg_apply(mdx_ctx* ctx, mdx_bg* bg, const uint8_t* frame, int stride, double learning_rate, uint8_t* fgmask);
int mdx_bg_image(mdx_ctx* ctx, mdx_bg* bg, uint8_t* out);
/* One stream's model in a canonical host layout, to checkpoint it or to start from a crafted state;
 * synchronous.  weight [h][w][nmixtures], variance [h][w][nmixtures], mean [h][w][nmixtures][channels] floats,
 * modes [h][w] bytes, nframes the model's frame count (one per model: set_state of any stream sets it).  Any
 * output of get_state may be NULL; entries of modes at or above a pixel's count read 0.  set_state needs all
 * four arrays, ignores entries at or above a pixel's count, and is MDX_EINVAL (model untouched) for a count
 * above nmixtures, a negative nframes or a stream outside [0, streams). */
int mdx_bg_get_state(mdx_ctx* ctx, mdx_bg* bg, int stream, float* weight, float* variance, float* mean,
                     uint8_t* modes, int* nframes);
int mdx_bg_set_state(mdx_ctx* ctx, mdx_bg* bg, int stream, const float* weight, const float* variance,
                     const float* mean, const uint8_t* modes, int nframes);

/* Page-locked host memory for frames and outputs (e.g. the node's rgb8 staging buffer and its
 * trajectory outputs): copies between it and the device run as DMA at full link rate, while a
 * pageable buffer is staged by the runtime through bounce buffers.  Any entry taking host pointers
 * accepts either.  mdx_host_alloc returns NULL on failure. */
void* mdx_host_alloc(size_t bytes);
int mdx_host_free(void* p);

/* Device memory helpers so hosts without a HIP toolchain (ctypes, cgo, JNI) can stage
 * buffers: allocation on the context's device, copies ordered on its stream. */
void* mdx_dev_alloc(mdx_ctx* ctx, size_t bytes);
int mdx_dev_free(mdx_ctx* ctx, void* p);
int mdx_memcpy_h2d(mdx_ctx* ctx, void* dst, const void* src, size_t bytes);
int mdx_memcpy_d2h(mdx_ctx* ctx, void* dst, const void* src, size_t bytes);

/* Per-stage device time from HIP events recorded on the ctx stream around each stage.
 * mdx_enable_timing(ctx, 1) (re)starts recording; every later pipeline call records one
 * event set (up to 256 calls).  mdx_stage_ms returns the SUM over the recorded calls, in
 * milliseconds, of stage: 0 gray+pad, 1 pyramids, 2 Scharr, 3 LK, 4 classify+fit,
 * 5 warp+diff, 6 whole call; mdx_timing_calls returns how many calls were recorded.
 * mdx_cluster_hulls records a set too: stage 0 its upload, 3 k_hull, 4 its readback, 6 the three
 * together (1, 2 and 5 are empty); mdx_region_hulls_dev too: stage 2 its scan of the records' bounds, 3
 * k_region_hull, 4 the scan that packs xy, 6 the three together (0, 1 and 5 are empty);
 * mdx_region_parents_dev too: stages 0 .. 4 its tile, merge, roots, flatten and resolve kernels, 6 the
 * five together (5 is empty); mdx_region_outlines_dev too: stage 0 its set-up kernels, 1 the rounds, 2 the
 * offsets, 3 the scatter, 6 all of them (4 and 5 are empty). */
int mdx_enable_timing(mdx_ctx* ctx, int on);
int mdx_timing_calls(const mdx_ctx* ctx);
int mdx_stage_ms(mdx_ctx* ctx, int stage, float* ms);

/* Test hook: copy an internal buffer of the last call to the host (0: per-(pair, level,
 * point) float4 LK gradient sums; 1: per-level LK trace when MDX_LK_DEBUG=1 at create;
 * 7: the centred data of the last mdx_fit_subspace, [ntraj * 2 * traj_len] floats then the two
 * means; 8: its 50 per-hypothesis inlier counts, int32). */
int mdx_debug_copy(mdx_ctx* ctx, int which, void* dst, size_t bytes);
/* Test hook: d_out[i] = 32 / d_in[i] through the projective warp's FP64 division (device buffers,
 * queued on the context stream); equal to IEEE division for |d_in[i]| in [2^-100, 2^100]. */
int mdx_debug_div32(mdx_ctx* ctx, const double* d_in, double* d_out, int n);
/* Test hook: which rows of k_warp_diff each tile of the context's last warp launch ran (any entry
 * that produces a mask; the call must have returned MDX_OK).  Waits for the context's stream, then
 * reads back the per-tile records and fits the kernel itself read and applies the kernel's own
 * branch conditions.  out[pair * tiles + tile], tiles = ceil(w / 128) * ceil(rows / 64), tile column
 * fastest: 0 general (per pixel), 1 fixed point, 2 affine FP64, 3 projective, -1 a pair without a
 * fit.  Writes at most cap codes (out may be NULL when cap is 0) and returns the launch's number of
 * (pair, tile) records, or a negative error. */
int mdx_debug_warp_paths(mdx_ctx* ctx, int32_t* out, int cap);

/* Measurement probe, no reference counterpart: the memory ceiling of k_warp_diff's access mix.
 * d_mask[i] = |d_a[i] - d_b[i]| > thresh ? 255 : 0 over n bytes (n a multiple of 16, pointers
 * 16-byte aligned): the same 3 B/px (read two frames, write the mask) as a linear streaming pass,
 * 16 B per lane, non-temporal.  Queued on the context's stream and timed as its warp_diff stage
 * (mdx_stage_ms) when timing is on; bench.py reports its rate as roofline.copy_ceiling. */
int mdx_probe_stream3_dev(mdx_ctx* ctx, size_t n, const uint8_t* d_a, const uint8_t* d_b, uint8_t* d_mask,
                          int thresh);

/*
 * Synthetic frame-pair generator used by the benchmark and tests (host, deterministic,
 * byte-identical on every x86-64 host).  Spec in DESIGN.md §5: blurred value noise +
 * rectangles; frame 2 = frame 1 under the affine H_true (0.5 deg rotation about the
 * centre, scale 1.01, translation (3.2, -1.7)) + one moving patch (+8, +5) + +-2 LSB noise.
 * channels = 1 (gray) or 3 (rgb8).  H_true (9 doubles, forward) is written if non-NULL.
 */
int mdx_synth_pair(uint64_t seed, int w, int h, int channels, uint8_t* img1, uint8_t* img2,
                   double* H_true, int nthreads);

#ifdef __cplusplus
}
#endif
#endif /* MDX_H_ */
