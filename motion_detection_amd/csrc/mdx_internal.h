// mdx_internal.h -- the one interface between the HIP kernel files (mdx_front.hip, mdx_lk_point.hip,
// mdx_fit.hip, mdx_lk.hip, mdx_warp.hip, mdx_subspace.hip, mdx_cluster.hip, mdx_vcluster.hip, mdx_outliers.hip, mdx_regions.hip, mdx_resize.hip, mdx_hull.hip, mdx_outline.hip, mdx_bg.hip) and the host files (mdx_ctx.h, mdx_api.cpp,
// mdx_pair.cpp, mdx_traj.cpp, mdx_post.cpp, mdx_bg_api.cpp).  Not part of the C-ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "mdx.h"
#include "mdx_plan.h"   // constants, Level / Geometry, the class plan: everything the host plans without a device

namespace mdx {

static_assert(sizeof(float4) == kFloat4Bytes, "lk_scratch sizes the A sums by it");
// LK debug buffer (MDX_LK_DEBUG=1): after the per-point records, the traced point's iterations
// (kMaxLevels * 64 float4), then per level and persistent wave of k_lk_iter its {start, end}
// s_memrealtime stamps (100 MHz), for the wave-occupancy profile (scripts/lk_tail.py)
constexpr int kLkDbgStampOff = kMaxLevels * 64 + 64;
constexpr int kLkDbgWaves = 16384;

// the gray frame of a pair's pyramid slab: level 0's core, lv[0].pitch bytes per row
inline uint8_t* level0_core(uint8_t* slab, const Geometry& g) { return slab + g.lv[0].img_off + g.lv[0].core(); }

// Per-pair result of the classify + fit stage.
struct PairFit {
    double H[9];      // getPerspectiveTransform output (or external H); zero when no fit
    double Hinv[9];   // matrix warpPerspective actually samples with (inverse or all-zero)
    int num_vectors;  // accepted vectors (reference return value)
    int fit_status;   // 0 fitted, 1 no vectors, 2 fewer than 4 vectors
    int src_y0, src_y1;   // row bands (k_band_fit): frame-1 rows the band's warp reads
};

struct LkClassArgs {
    Geometry g;
    ClassPlan plan;
    const int16_t* rlist;    // [level][axis][kTabStride] class index -> residue
    int level;
};

struct LkArgs {
    const uint8_t* pyr1;     // prev pyramid slabs
    const uint8_t* pyr2;     // next pyramid slabs
    const uint32_t* der;     // prev derivative slabs
    Geometry g;
    int maxl;                // attained max level used by LK
    int npts, ny, pixel_step;
    int nyg;                 // LK v2: grid rows in the group order (ny, or a row band's count)
    int max_iters;
    float min_eig;
    double eps2;
    float* next_pts;         // [batch][npts][2]
    float* carry;            // LK v2: per level l > 0 a [batch][npts][2] array (at carry + l *
                             // carry_lstride) of the points level l leaves for level l-1; level 0
                             // writes next_pts.  null: next_pts carries them (levels in sequence only)
    long long carry_lstride; // floats between two levels' carried-point arrays
    uint8_t* status;         // [batch][npts]
    ClassPlan plan;          // LK v2 only
    const int16_t* cmap;     // [level][axis][kTabStride] residue -> class index
    const int16_t* rlist;    // [level][axis][kTabStride] class index -> residue
    const int16_t* ord;      // per level: nxp padded grid columns (-1 = empty), then ny grid rows,
                             // both grouped by residue class (ClassLevel::ord_off)
    const float* prev_pts;   // k_lk only: [batch][npts][2] start points (trajectories); null = the grid
    int max_sub;             // > 0: at most this many pairs per LK sub-batch (MDX_LK_SUB, tests)
    int* done;               // LK v2 dataflow: [level][done_stride] groups retired per pair, each
                             // counter on its own 128-B line (kCtrPad ints); null:
                             // the level launches run one after another
    int done_stride;
    int dep_groups;          // > 0: groups per pair of the coarser level, which a group waits for
    int* err;                // dataflow statistics, read and cleared at the context's sync points:
                             // [0] group waits and [1] gate waits that gave up, [2] levels recomputed
    int* lflags;             // dataflow: the call's per-level flags (kLkFlag* below, zeroed with
                             // `done`); null: no dataflow
    int redo;                // 1: this launch is level `level`'s conditional recompute (kLkFlag*)
    int spin_max;            // dataflow wait bound in s_sleep(8) polls; < 0: fault injection (every
                             // wait counts as timed out at once; tests)
    int flow_cap;            // dataflow: percent of the resident waves one iteration launch takes
    float4* dbg;             // optional [batch][nlev][npts] (npx, npy, iters, status) at level end
    int dbg_pt;              // point whose per-iteration values are appended after dbg (pair 0)
    int fma;                 // LK v2: 1: k_lk_iter may take the fused row body where every iterating
                             // point of the wave is certified (MDX_LK_FMA, mdx_lk.hip); 0: never
    uint32_t* body_cnt;      // optional (MDX_LK_DEBUG) [kMaxLevels][2] wave-iterations of k_lk_iter by
                             // row body: [level][0] exact, [level][1] fused
};

// default dataflow wait bound: s_sleep(8) polls, ~0.1 s
constexpr int kLkSpinDefault = 1 << 19;
// persistent waves of a recompute launch: cheap when it exits at once (the common case), and a
// recompute of the finest level at 1080p x 32 still takes only tens of ms
#ifndef MDX_LK_REDO_WAVES
#define MDX_LK_REDO_WAVES 512
#endif
constexpr int kLkRedoWaves = MDX_LK_REDO_WAVES;

// Launchers (mdx_front.hip; launch_lk: mdx_lk_point.hip).  All enqueue on `s`.
// fsel: 0 both frames of every pair, 1 the first frame only, 2 the second frame only
hipError_t launch_gray_pad(hipStream_t s, int batch, const uint8_t* in1, const uint8_t* in2, int w, int h,
                           int stride, long long frame_stride, int fmt, uint8_t* pyr1, uint8_t* pyr2,
                           const Geometry& g, int fsel = 0);
// gray + pad of level 0 and pyrDown to level 1 in one pass (k_front; launch_gray_pad when nlev == 1);
// launch_pyr_levels then builds levels 2 .. nlev-1 (k_front in level mode, one launch per level)
// rows (may be null = all): [nlev] core rows wanted per level; only the bands covering them are built
hipError_t launch_front(hipStream_t s, int batch, const uint8_t* in1, const uint8_t* in2, int w, int h, int stride,
                        long long frame_stride, int fmt, uint8_t* pyr1, uint8_t* pyr2, const Geometry& g,
                        int fsel = 0, const RowSpan* rows = nullptr);
hipError_t launch_pyr_levels(hipStream_t s, int batch, uint8_t* pyr1, uint8_t* pyr2, const Geometry& g, int fsel = 0,
                             const RowSpan* rows = nullptr);
// every level's Scharr planes, whole levels, one launch
hipError_t launch_scharr_levels(hipStream_t s, int batch, const uint8_t* pyr1, uint32_t* der, const Geometry& g);
// padded rows [prow0, prow1) of one level's derivative planes (default: all): the class-plane LK's
// per-level launches, which need only the rows its planes read (mdx_lk.hip launch_lk_v2)
hipError_t launch_scharr(hipStream_t s, int batch, const uint8_t* pyr1, uint32_t* der, const Geometry& g, int level,
                         int prow0 = 0, int prow1 = -1);
hipError_t launch_lk(hipStream_t s, int batch, const LkArgs& a);

// Trajectory passes in one launch (k_lk chain mode): pass j of point p tracks frame j -> j+1 from
// the point pass j-1 left, waiting for it through flag[p]; the pass bookkeeping of
// calculateOpticalFlowTrajectory (k_traj_update's) is done by the point's own wave.
constexpr int kMaxTrajImgs = 16;
struct TrajChain {
    const uint8_t* pyr[kMaxTrajImgs];    // padded pyramid slab of each frame
    const uint32_t* der[kMaxTrajImgs];   // its Scharr planes
    int nimg, w, h;
    float* cur;                          // [npts][2] current points (atomic hand-off between passes)
    float* traj;                         // [npts][nimg][2]
    int* tlen;                           // [npts]
    int* flag;                           // [npts] passes done (zeroed by k_traj_init)
    double* vectors;                     // [npts][4] Vec4d of the last pass, or null
    float* start_pts;                    // [npts][2] start points of the last pass, or null
    int* num;                            // [0] num_vectors, [1] hand-off waits that timed out
    double mvs;                          // min_vector_size
    // the caller's page-locked outputs, device-mapped (or null): the passes write traj, traj_len,
    // start_pts and vectors straight into them, and no readback copy follows
    float* htraj;
    int* htlen;
    float* hstart;
    double* hvec;
};
// ppw: points per wave (1: 64 lanes per point, 2: 32, 4: 16)
hipError_t launch_lk_chain(hipStream_t s, const LkArgs& a, const TrajChain& t, int ppw);
// Trajectory subspace RANSAC (fitSubspace): mean-subtracted data, nhyp hypotheses of d columns
// (cols: [nhyp][d]), winner's residuals / outlier flags; best[0] = winner or -1.  Scratch: data
// [N][2T] floats + 2 (the means), basis [nhyp] x subspace_basis_bytes(2T, d, precision), counts [nhyp].
// One hypothesis kernel and one final kernel, instantiated for the mode precision selects.
// subspace_basis_bytes: one hypothesis' basis, [2T][2T-d] doubles (MDX_SUBSPACE_F32: [2T][2T] floats).
size_t subspace_basis_bytes(int n, int d, int precision);
hipError_t launch_subspace(hipStream_t s, const float* traj, int N, int T, int d, const int* cols, int nhyp,
                           double sigma, float* data, void* basis, int* counts, double* residuals,
                           uint8_t* is_outlier, int* best, int precision);
// Greedy Euclidean clustering (clusterEuclidean, mdx_cluster.hip): root[i] = index of the first point
// of point i's cluster.  pts [N][2]; slim: a squared distance s joins iff its float bits < slim
// (bits of the largest passing s, plus 1; 0: nothing joins).  Scratch: best [N] keys.  ceil(N / kClB)
// launches on s.
constexpr int kClB = 256;    // points per block (= threads of k_cluster_step)
hipError_t launch_cluster(hipStream_t s, const float* pts, int N, uint32_t slim, unsigned long long* best,
                          int32_t* root);
// First-fit clustering of flow vectors by distance and angle (getClusters, mdx_vcluster.hip): root[i] =
// index of the first vector of active vector i's cluster.  xyt: [3][nA] doubles (x, y, angle in
// [0, 2 pi]) of the nA active vectors; slim: a squared distance s joins iff s <= slim (< 0: nothing
// joins); athr: the angular threshold; abs_int: MDX_VCLUSTER_ABS_INT.  Scratch: rows
// (vcluster_rows_bytes(nA)), qscan [kClB] and cand [kClB][32] words.  3 * ceil(nA / kClB) - 1 launches on s.
size_t vcluster_rows_bytes(int nA);
hipError_t launch_vcluster(hipStream_t s, const double* xyt, int nA, double slim, double athr, int abs_int,
                           uint32_t* rows, uint32_t* qscan, uint32_t* cand, int32_t* root);
// Flow-vector outliers by median / MAD (findOutliers, mdx_outliers.hip): one workgroup per field, one
// launch on s.  dxy: [batch][2][n] doubles (dx plane, dy plane); ang: [batch][n] the host's atan2 (the
// re-reading kernel overwrites the entries outside the selected set with NaN); mag: [batch][n] scratch;
// flags: [batch][n] bit 0 angle, bit 1 magnitude; stats: [batch].  0 < n <= MDX_OUTLIERS_MAX_POINTS.
// in_registers: fields of up to 24,576 vectors keep a channel's values in registers (ang and mag are
// then only read); false: every pass re-reads them, as larger fields always do (MDX_OL_REG=0).
hipError_t launch_outliers(hipStream_t s, int batch, int n, const double* dxy, double* ang, double* mag,
                           int include_zeros, uint8_t* flags, mdx_outlier_stats* stats, bool in_registers);
// Trajectory tracking (calculateOpticalFlowTrajectory): grid init and the per-pass point update.
hipError_t launch_traj_init(hipStream_t s, int npts, int ny, int pixel_step, int nimg, float* cur, float* traj,
                            int* tlen, int* num, int* flag = nullptr);
hipError_t launch_traj_update(hipStream_t s, int npts, const float* next_pts, const uint8_t* status, float* cur,
                              float* traj, int* tlen, int nimg, int w, int h, int last, double min_vector_size,
                              double* vectors, float* start_pts, int* num);
// launch_lk_v2 (mdx_lk.hip): where the class-plane LK of a call is enqueued.  Host only, never
// passed to a kernel.  The context fills the first block once at create, run_lk the rest per call.
struct LkLaunch {
    hipStream_t s = nullptr;         // the context's stream: everything after the LK follows it
    hipStream_t aux = nullptr;       // (may be null) second stream for the flow-independent class / A kernels
    hipStream_t s2 = nullptr;        // (null: no dataflow) every other level's iteration launch
    hipEvent_t* ev = nullptr;        // kMaxLevels + 1 events (no timing) used to order s and aux
    hipEvent_t* flow_ev = nullptr;   // dataflow: 2 events
    hipEvent_t* redo_ev = nullptr;   // dataflow fallback: kMaxLevels events
    uint8_t* cls = nullptr;          // class planes
    float4* Ab = nullptr;            // [nlev][batch][npts] per-point (A11, A12, A22, 1/D)
    uint8_t* cert = nullptr;         // [nlev][batch][npts] per-point product certificate (mdx_lk.hip), written with Ab
    int* qctr = nullptr;            // [batch][kMaxLevels][8] (x kCtrPad) queue heads
    int* done = nullptr;             // dataflow: kMaxLevels x batch + kLkFlagInts counters
    // (may be null: calls do not overlap) [kMaxLevels] events, re-recorded after each level's
    // iteration launch; the aux stream waits for the previous call's before rewriting that level's
    // class planes, A sums and queue heads (call pipelining lets the aux stream run a call ahead)
    hipEvent_t* lvl_done = nullptr;
    // (may be null) recorded by the caller once the first frames' pyramids exist; the aux work waits
    // on it instead of on everything enqueued on s so far (the second frames' pyramids may still be
    // in flight on s)
    hipEvent_t prev_ready = nullptr;
};
// Dataflow (s2, flow_ev and done non-null): the level launches alternate between s and s2, so level
// L-1 starts in level L's tail; its groups wait for their pair's level-L groups (done counters).
// Used when every XCD's work range holds two or more whole pairs (batch a multiple of 8, at least
// 16) and pairs' next_pts do not share 128-B lines (npts % 16 == 0).
// Dataflow fallback: a group whose wait gives up (the coarser level's launch was not dispatched in
// time: a preempted, shared or serialized device) abandons its level, which then drains without
// computing; right behind each level's launch, on its stream and after the coarser level's (redo_ev),
// a recompute launch re-runs the level in sequence if it gave up or the coarser level was
// recomputed, and exits at once otherwise.  Results are then always exact.
hipError_t launch_lk_v2(const LkLaunch& L, int batch, const LkArgs& a);
// MDX_FIT_RANSAC (mdx_fit.hip k_ransac_*): device scratch and parameters
constexpr int kRansacMaxIters = 1024;
struct RansacArgs {
    int iters;
    double thresh;
    uint32_t seed;
    int* list;       // [batch][npts] accepted grid indices, x-major
    double* hyps;    // [batch][iters][9]
    int* counts;     // [batch][iters]
};
// The RANSAC scratch, byte offsets: list from 0, hyps at the next 8-B boundary, counts behind them;
// bytes: the three arrays and 256 that cover the gap.
struct RansacScratch {
    size_t hyps, counts, bytes;
};
inline RansacScratch ransac_scratch(int batch, int npts, int iters)
{
    const size_t list_b = (size_t)batch * npts * sizeof(int), hyps_b = (size_t)batch * iters * 9 * sizeof(double),
                 counts_b = (size_t)batch * iters * sizeof(int);
    RansacScratch L;
    L.hyps = (list_b + 7) & ~(size_t)7;
    L.counts = L.hyps + hyps_b;
    L.bytes = list_b + hyps_b + counts_b + 256;
    return L;
}
inline size_t ransac_scratch_bytes(int batch, int npts, int iters) { return ransac_scratch(batch, npts, iters).bytes; }
// the call's RansacArgs over ransac_scratch_bytes() of device memory at base
inline RansacArgs ransac_args(void* base, int batch, int npts, const mdx_params& P)
{
    const RansacScratch L = ransac_scratch(batch, npts, P.ransac_iters);
    uint8_t* b = static_cast<uint8_t*>(base);
    return {P.ransac_iters, P.ransac_thresh, P.ransac_seed, reinterpret_cast<int*>(b),
            reinterpret_cast<double*>(b + L.hyps), reinterpret_cast<int*>(b + L.counts)};
}
// k_classify's record of one 256-point block (mdx_fit.hip), in launch_classify_fit's scratch
struct BlockSummary {
    int count;        // accepted points of the block
    int first[4];     // the first four of them (grid indices, block order); [count ..) not written
    int ransac_off;   // MDX_FIT_RANSAC: accepted points in the pair's blocks before this one (k_fit,
                      // for k_ransac_compact)
    int pad_[2];
};
static_assert(sizeof(BlockSummary) == 32, "BlockSummary: eight ints, two records per 64-B line");
inline int classify_blocks(int npts) { return (npts + 255) / 256; }
// bytes of the scratch launch_classify_fit needs
inline size_t classify_scratch_bytes(int batch, int npts)
{
    return (size_t)batch * classify_blocks(npts) * sizeof(BlockSummary);
}
// The classify + fit stage of `batch` pairs (mdx_fit.hip has the kernels' inventory).
struct FitArgs {
    const float* next_pts;      // [batch][npts][2] the LK's points
    const uint8_t* status;      // [batch][npts]
    int npts, ny, pixel_step;   // the grid (x-major, ny rows)
    int gy0, gy1;               // grid rows classified (a row band; others are neither written nor counted)
    double min_vector_size;
    double* vectors;            // (may be null) [batch][npts][4] Vec4d
    PairFit* fits;              // [batch]
    int fit_mode;
    const double* H_external;   // MDX_FIT_EXTERNAL: [batch][9]
    void* scratch;              // classify_scratch_bytes(batch, npts)
    mdx_band_cand* cand;        // non-null: row-band mode -- the band's count and first four accepted
                                // points go to cand[pair] instead of a fit
    RansacArgs ransac;          // MDX_FIT_RANSAC without cand: ransac_args(); otherwise unused
};
hipError_t launch_classify_fit(hipStream_t s, int batch, const FitArgs& a);
// Merge nrec band records (first four accepted overall = four smallest indices) and fit
hipError_t launch_band_fit(hipStream_t s, int nrec, const mdx_band_cand* cands, PairFit* fit, int w, int h, int y0,
                           int y1);
// Row bands: frame-1 gray rows [fit->src_y0, fit->src_y1) into the padded level 0 of pyr1 (the
// band's warp may read rows its own pyramid build skipped), except the rows [built0, built1) the
// pyramid build wrote.  gray1_l0: level-0 core, pitch bytes.
hipError_t launch_gray_rows(hipStream_t s, const uint8_t* img1, int w, int stride, int fmt, uint8_t* gray1_l0,
                            int pitch, const PairFit* fit, int built0 = 0, int built1 = 0);
hipError_t launch_set_fit_external(hipStream_t s, int batch, const double* H_external, PairFit* fits);
// Destination rows [row0, row1) of every pair (row1 <= h); mask row y is at mask + (y - row0) * w.
// scratch: warp_scratch_bytes(batch, w, rows of the band) of device memory for the per-pair and
// per-tile tables of k_warp_prep (the launch's own; reused by the next launch on the stream)
size_t warp_scratch_bytes(int batch, int w, int rows);
// What a launch_warp_diff handed k_warp_diff, kept by the context for the path report
// (mdx_debug_warp_paths): the workgroup-uniform fast-path inputs and the device tables.
struct WarpLaunch {
    int batch = 0, ntiles = 0;   // pairs, tiles per pair (tile column fastest); batch 0: no launch yet
    int bw0 = 0, vec_ok = 0;
    const PairFit* fits = nullptr;
    const void* tinfo = nullptr;   // TileInfo[batch][ntiles] inside the launch's scratch
};
struct GrayPlane {
    const uint8_t* p;         // pair 0's row 0
    long long frame_stride;   // bytes between pairs
    int pitch;                // bytes between rows
};
struct WarpArgs {
    GrayPlane g1, g2;         // frame 1 (warped), frame 2
    int w, h;
    const PairFit* fits;
    uint8_t* mask;            // the band's rows, w bytes each
    long long mask_stride;    // bytes between pairs
    int thresh;
    int row0 = 0, row1 = -1;  // the band; row1 < 0: h
};
hipError_t launch_warp_diff(hipStream_t s, int batch, const WarpArgs& a, void* scratch, size_t scratch_bytes,
                            WarpLaunch* rec = nullptr);
// Test hook: the row path of every (pair, tile) of launch L, from the TileInfo records and fits its
// k_warp_diff read; out[pair * ntiles + tile] = 0 general, 1 fixed point, 2 affine FP64,
// 3 projective, -1 pair without a fit.  Waits for the stream.  At most cap codes are written.
hipError_t debug_warp_paths(hipStream_t s, const WarpLaunch& L, int32_t* out, int cap);
hipError_t launch_div32(hipStream_t s, const double* in, double* out, int n);   // test hook
hipError_t launch_stream3(hipStream_t s, size_t n, const uint8_t* a, const uint8_t* b, uint8_t* o, int thresh);
hipError_t launch_export_fit(hipStream_t s, int batch, const PairFit* fits, double* H, int* num_vectors);
// mdx_regions.hip: the motion mask labelled into regions.  Seven launches on s, no
// host synchronisation.  scratch: regions_scratch_bytes(batch, w, h) of device memory, a function
// of (batch, w, h) alone (about 9 B per pixel: a 4-B label, 20 B per possible component, of which a
// w x h image has at most ceil(w/2) * ceil(h/2)); `lay`, when given, receives its layout.
constexpr int kRegionsMaxBatch = 65535;   // images per launch (grid y)
struct RegionsScratch {
    size_t lab, blk, stats, nall;   // byte offsets: labels, per-block root counts, records, component counts
};
size_t regions_scratch_bytes(int batch, int w, int h, RegionsScratch* lay = nullptr);
hipError_t launch_mask_regions(hipStream_t s, int batch, const uint8_t* mask, int w, int h, int stride,
                               size_t frame_stride, int open3, int min_area, mdx_region* regions, int max_regions,
                               int32_t* num_all, int32_t* num_kept, int32_t* labels, uint8_t* mask_out, void* scratch);
// mdx_regions.hip: the parent blob of each region record and the external records.
// Five launches on s (one when max_regions is 0), no host synchronisation, every pointer a device
// pointer.  scratch: region_parents_scratch_bytes(batch, w, h) of device memory, a function of those
// three alone (5 B per pixel: the background's 4-B parent word and a mark byte); nothing in it has
// to be cleared between calls.  ev, when given, holds seven events: ev[1 .. 5] are recorded behind
// the tile, merge, roots, flatten and resolve kernels.
struct RegionTreeScratch {
    size_t bg, mark;   // byte offsets: the background's parent words, the mark bytes
};
size_t region_parents_scratch_bytes(int batch, int w, int h, RegionTreeScratch* lay = nullptr);
hipError_t launch_region_parents(hipStream_t s, int batch, const int32_t* labels, int w, int h,
                                 const mdx_region* regions, int max_regions, const int32_t* num_kept, int32_t* parent,
                                 mdx_region* external, int32_t* num_external, void* scratch, hipEvent_t* ev = nullptr);

// cv::Mat(vector<Point2f>).copyTo(vector<cv::Point>): saturate_cast<int>(float) = cvRound, half to even.
// The rectangles (mdx_post.cpp clusters_from_roots) and the hulls (host and k_hull) convert with this.
__host__ __device__ inline int32_t cv_round(float v) { return (int32_t)lrint((double)v); }

// Convex hulls of clusters (mdx_hull.hip k_hull): one workgroup per cluster, one launch
// on s.  pts: the members grouped by cluster; recs [k]; max_ncols: the widest cluster's columns (<=
// MDX_HULL_MAX_SPAN), which sizes the dynamic LDS (hull_lds_bytes: 12 B per column).  counts [k]: each
// hull's vertices; staging: cluster c's vertices (x, y), in order, from pair out_off on (at most bound).
struct HullCluster {
    int32_t start, count;    // the cluster's members: pts[start .. start + count)
    int32_t xmin, ncols;     // smallest converted x, and xmax - xmin + 1
    int32_t out_off, bound;  // its slice of staging, in vertices: min(count, 2 * ncols) holds any hull
    int32_t pad_[2];
};
static_assert(sizeof(HullCluster) == 32, "HullCluster: eight ints");
size_t hull_lds_bytes(int ncols);
hipError_t launch_hull(hipStream_t s, int k, const HullCluster* recs, const float* pts, int max_ncols,
                       int32_t* counts, int32_t* staging);

// Convex hulls of the mask regions (mdx_hull.hip k_region_hull): three launches on s, no
// host synchronisation, every pointer a device pointer, w <= MDX_HULL_MAX_SPAN.  scratch:
// region_hulls_scratch_bytes(batch, w, h, max_regions) of device memory, a function of those four alone:
// per record its staging slice (8 B) and vertex count (4 B), per image a staging block of
// min(w*h, 2*min(w, h)*max_regions) vertices of 8 B; `lay`, when given, receives its layout.
constexpr int kRegionHullGridX = 1 << 21;   // records per k_region_hull launch (grid x of 1,024-lane workgroups)
struct RegionHullScratch {
    size_t slices, counts, staging;   // byte offsets
};
size_t region_hulls_scratch_bytes(int batch, int w, int h, int max_regions, RegionHullScratch* lay = nullptr);
hipError_t launch_region_hulls(hipStream_t s, int batch, const int32_t* labels, int w, int h, const mdx_region* regions,
                               int max_regions, const int32_t* num_kept, int32_t* offsets, int32_t* xy,
                               int max_vertices, int32_t* num_vertices, void* scratch,
                               hipEvent_t hull_begin = nullptr, hipEvent_t hull_end = nullptr);   // around k_region_hull

// Outer border polylines of the mask regions (mdx_outline.hip): region_outlines_launches
// launches on s (7 + outline_rounds(w, h) with records and room for points, 1 when max_regions is 0), no
// host synchronisation, every pointer a device pointer, w * h <= 2^28.  scratch:
// region_outlines_scratch_bytes(batch, w, h, max_regions) of device memory, a function of (batch, w, h)
// alone: per pixel 7 state words of 8 B, the 4-B index of its first state and its 1-B neighbour mask, per
// 256 pixels a 4-B state count, per image the state total and 64 round flags; nothing in it has to be
// cleared between calls.  ev, when given, holds seven events: ev[1 .. 4] are recorded behind the set-up
// kernels (mask, blocks, base, pred, starts), the rounds, the offsets and the scatter.
struct RegionOutlineScratch {
    size_t words, base, blk, nstates, flags, nbr;   // byte offsets
};
size_t region_outlines_scratch_bytes(int batch, int w, int h, int max_regions, RegionOutlineScratch* lay = nullptr);
int region_outlines_launches(int w, int h, int max_regions, int max_points);
hipError_t launch_region_outlines(hipStream_t s, int batch, const int32_t* labels, int w, int h, const mdx_region* regions,
                                  int max_regions, const int32_t* num_kept, int32_t* offsets, int32_t* xy, int max_points,
                                  int32_t* num_points, void* scratch, hipEvent_t* ev = nullptr);

// Half-size ingest (mdx_resize.hip k_half): `batch` frames of w x h pixels of `channels`
// (1 or 3) interleaved bytes halved to mdx_half_size(w, h), one launch on s (per kHalfMaxBatch frames).
// A lane owns kHalfPx adjacent destination pixels of kHalfRows rows; a wave 64 * kHalfPx and a
// workgroup kHalfWgPx destination pixels of a row.
constexpr int kHalfPx = 4;
constexpr int kHalfWavePx = 64 * kHalfPx;
constexpr int kHalfWgPx = 256 * kHalfPx;
constexpr int kHalfRows = 4;
constexpr int kHalfMaxBatch = 65535;   // frames per launch (grid z)
// whether launch_half takes k_half's vector path: every base and pitch (a batch's frame pitches too) a
// multiple of 4; otherwise its byte path
bool half_vector_path(int batch, const void* src, int stride, size_t frame_stride, const void* dst, int dst_stride,
                      size_t dst_frame_stride);
hipError_t launch_half(hipStream_t s, int batch, const uint8_t* src, int w, int h, int stride, size_t frame_stride,
                       int channels, uint8_t* dst, int dst_stride, size_t dst_frame_stride);

// Background subtraction (mdx_bg.hip): the per-pixel Gaussian mixture of `streams` independent
// models of w x h pixels.  state: per stream bg_state_floats floats, one plane of w * h per (mode, field) --
// plane m the weights of mode m, nmixtures + m its variances, 2 * nmixtures + m * channels + c its means;
// modes: [streams][h][w] bytes.  One launch each on s, no host synchronisation.
constexpr int kBgMaxFrames = 32;        // frames one k_bg_apply launch carries a mixture through
constexpr int kBgMaxStreams = 65535;    // models per launch (grid y)
struct BgModel {
    float* state;
    uint8_t* modes;
    int streams, w, h, channels;
    mdx_bg_params prm;
};
__host__ __device__ inline size_t bg_state_floats(int w, int h, int channels, int nmixtures)
{
    return (size_t)w * h * nmixtures * (2 + channels);
}
// frames: stream s, frame t, row y at frames + s * stream_stride + t * frame_stride + y * stride; alphaT [T],
// T <= kBgMaxFrames; mask (may be null): stream s, frame t at mask + s * mask_stream_stride + t * w * h
hipError_t launch_bg_apply(hipStream_t s, const BgModel& M, int T, const uint8_t* frames, int stride, size_t frame_stride,
                           size_t stream_stride, const float* alphaT, uint8_t* mask, size_t mask_stream_stride);
hipError_t launch_bg_image(hipStream_t s, const BgModel& M, uint8_t* out /* [streams][h][w][channels] */);

}  // namespace mdx
