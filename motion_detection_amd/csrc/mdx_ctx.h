// mdx_ctx.h -- the context behind the C-ABI (include/mdx.h) and what every host file (mdx_api.cpp, mdx_pair.cpp,
// mdx_traj.cpp, mdx_post.cpp, mdx_bg_api.cpp) needs of it: owning types, errors, workspace growth, the frame check.
#pragma once

#include "../../include/mdx.h"
#include "mdx_internal.h"

#include <algorithm>
#include <array>
#include <cstdarg>
#include <cstdio>
#include <initializer_list>
#include <memory>
#include <string>
#include <utility>
#include <vector>

// Device memory that frees itself.  Move-only; move assignment swaps, so the source frees the old memory.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        std::swap(p, o.p), std::swap(cap, o.cap);
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset()
    {
        if (p) (void)hipFree(p);
        p = nullptr, cap = 0;
    }
    bool alloc(size_t bytes)   // a fresh allocation (the old one is freed first); empty on failure
    {
        reset();
        if (hipMalloc(&p, bytes) != hipSuccess) p = nullptr;
        cap = p ? bytes : 0;
        return p != nullptr;
    }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

// The MDX_* environment knobs (INTEGRATION.md describes each), read once by mdx_create (read_tuning).
struct LkTuning {
    int lk_impl = 2;          // MDX_LK_IMPL: 1 = single-kernel LK (k_lk), 2 = class planes
    int lk_g = 0;             // MDX_LK_G: LK group size, 0 = per level, 4 or 8
    int lk_sub = 0;           // MDX_LK_SUB: > 0: LK sub-batch cap (tests)
    int lk_astrip = 0;        // MDX_LK_ASTRIP: grid rows per A-sum strip (0: kAStripRows)
    bool lk_debug = false;    // MDX_LK_DEBUG=1: per-level trace
    bool traj_chain = true;   // MDX_TRAJ_CHAIN=0: trajectory passes one launch per pass, not chained
    int traj_ppw = 4;         // MDX_TRAJ_PPW: trajectory LK points per wave (1, 2 or 4)
    bool lk_aux = true;       // MDX_LK_AUX=0: no aux stream (LK class / A kernels do not run ahead)
    bool lk_flow = true;      // MDX_LK_FLOW=0: no LK dataflow (no second iteration stream)
    // MDX_LK_CAP: dataflow launch share of the resident waves (%).  75: the aux stream's next-level
    // class planes and A sums pace the level hand-offs (round 6, profiles/r06_ab_lk_w5_cap.txt: 60 -3%,
    // 70 / 80 / 85 within 1%, 75 best and steadiest, 95 -1.2%)
    int lk_cap = 75;
    // MDX_LK_FMA=0: k_lk_iter never takes its fused row body (A/B runs, tests); the certificate is
    // still computed and loaded
    bool lk_fma = true;
    int spin_max = mdx::kLkSpinDefault;  // MDX_LK_SPIN_MAX (debug: < 0 injects timeouts)
    bool ol_reg = true;       // MDX_OL_REG=0: findOutliers re-reads its values on every pass at every size
};

// A background model (mdx_bg_create, mdx_bg_api.cpp): owned by its context's `bgs`, freed with it.
struct mdx_bg {
    mdx_ctx* owner = nullptr;
    int streams = 0, w = 0, h = 0, channels = 0;
    mdx_bg_params prm{};
    int nframes = 0;
    DevBuf state, modes;       // mdx_internal.h BgModel
    DevBuf hin, hout;          // the host conveniences' frame, and mask or image
    std::vector<float> xfer;   // get_state / set_state: one stream's planes on the host; only ever grows
};

struct mdx_ctx : LkTuning {   // the knobs stay plain members (c->lk_cap, ...)
    int device = 0;
    // what mdx_destroy releases: every stream, event and pinned block created (new_stream, new_events, pinned_ints)
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> events;
    std::vector<void*> pinned;
    hipStream_t stream = nullptr;
    hipStream_t aux = nullptr;               // LK class / A kernels run ahead here (MDX_LK_AUX=0: off)
    hipEvent_t lkev[mdx::kMaxLevels + 2] = {};    // launch_lk_v2's + the first frames' pyramids ready
    hipStream_t iter2 = nullptr;             // LK dataflow: every other level's iteration launch (MDX_LK_FLOW)
    hipEvent_t flowev[2] = {};
    // Call pipelining (mdx_params.call_pipelining): the pyramid slabs have two halves used by
    // alternate calls, and a call's front end runs on the aux stream right behind the previous
    // call's last class planes and A sums, so it overlaps that call's last LK level and fit/warp.
    // (A stream of its own measured 1.9x slower: a process gets 4 hardware queues, and a fifth
    // stream shares one, so its event waits block the work queued behind them.)
    hipEvent_t front_ev = nullptr;
    hipEvent_t pyr_free[2] = {};             // on `stream`, after the last reader of each half
    hipEvent_t lvl_done[mdx::kMaxLevels] = {};    // the last call's iteration launch of each level
    hipEvent_t redo_ev[mdx::kMaxLevels] = {};     // LK dataflow: each level's launch + recompute done (fallback order)
    mdx::LkLaunch lk;                          // launch_lk_v2's streams and events (run_lk adds the per-call part)
    int pyr_half = 0;                        // the half the next pipelined call writes
    hipEvent_t input_ev = nullptr;           // mdx_input_ready: the next device call's inputs (caller-owned)
    uint8_t* last_pyr1 = nullptr;            // the last pair call's pyramids (debug copies)
    uint8_t* last_pyr2 = nullptr;
    // the latest mdx_band_flow_dev's pyramids, which its fit/warp reads (band_w == 0: none, or
    // voided by another call that rebuilt the slabs since)
    uint8_t* band_pyr1 = nullptr;
    uint8_t* band_pyr2 = nullptr;
    int band_half = 0;
    const uint8_t* band_img1 = nullptr;      // the last mdx_band_flow_dev's frame 1 (its fit/warp reads it)
    int band_built[2] = {0, 0};              // level-0 rows of frame 1 that call's pyramid build wrote
    int band_stride = 0, band_fmt = 0;
    // LK dataflow fallback statistics ([0] group waits and [1] gate waits that gave up, [2] levels
    // recomputed), read back and cleared at the sync points, accumulated in lk_fallback
    DevBuf errw;
    int* err_host = nullptr;                 // pinned readback
    int* tcnt_host = nullptr;                // pinned readback of the trajectory counts
    long long lk_fallback[3] = {0, 0, 0};
    mdx_params prm{};
    int max_w = 0, max_h = 0, max_batch = 0;
    DevBuf pyr1, pyr2, der, fits;            // pyramid / derivative / fit workspace
    DevBuf in1, in2, np, st, vec, mask, H, Hext, num;   // host-path staging
    DevBuf bnp, bst;                         // LK outputs the batched caller did not ask for
    DevBuf cls, Abuf, ctab;                  // LK v2: class planes, A sums, residue tables
    DevBuf dbg;                              // LK v2 per-level trace (MDX_LK_DEBUG=1)
    DevBuf lkcnt;                            // MDX_LK_DEBUG=1: the last call's k_lk_iter wave-iterations by row body
    DevBuf csum;                             // classify: per-block summaries
    DevBuf tin, tcur, tnp, tst, ttraj, tnum, tflag;   // trajectory tracking (ttraj: the four outputs, one block)
    DevBuf straj, sdata, sq, scnt, scols, sres, sout, sbest;      // subspace RANSAC
    DevBuf clpts, clbest, clroot;            // clusterEuclidean: points, running keys, roots
    std::vector<int32_t> cl_host;            // its host side (roots, ranks, sizes, boxes): only ever grows
    DevBuf vcpts, vcroot, vcrows, vcq;       // getClusters: (x, y, angle) planes, roots, scan rows, qscan + cand
    std::vector<double> vc_host;             // its staging of the active vectors' planes: only ever grows
    std::vector<float> vc_pts;               // the active vectors' (x, y) as float, for the rectangles
    std::vector<int32_t> vc_idx;             // active vector -> input index, then the compact labels
    DevBuf hlin, hlout;                      // mdx_cluster_hulls: records + grouped members, counts + staged hulls
    std::vector<int32_t> hl_in, hl_out;      // their host images: only ever grow
    std::vector<int32_t> hl_idx;             // each member's requested cluster (-1: none), then the fill cursors
    DevBuf olin, olmag, olout;               // findOutliers: (dx, dy) planes + angles, magnitudes, stats + flags
    std::vector<double> ol_host;             // its staging of the planes: only ever grows
    std::vector<uint8_t> ol_flags;           // the flags when the caller takes only the vectors
    DevBuf rgscr;                            // mdx_mask_regions_dev: labels, block counts, component records
    DevBuf rgin, rgout;                      // mdx_mask_regions (host entry): the mask, every output
    DevBuf rhscr;                            // mdx_region_hulls_dev: staging slices, vertex counts, staged hulls
    DevBuf rhout;                            // mdx_mask_region_hulls (host entry): counts, records, labels, offsets, xy
    DevBuf rtscr;                            // mdx_region_parents_dev: the background's parent words and mark bytes
    DevBuf rtout;                            // mdx_mask_regions_tree (host entry): counts, records, parents, labels, offsets, xy
    DevBuf roscr;                            // mdx_region_outlines_dev: neighbour masks, state indices, state words
    DevBuf roout;                            // mdx_mask_region_outlines (host entry): counts, records, parents, labels, offsets, xy
    std::vector<std::unique_ptr<mdx_bg>> bgs;   // background models not yet destroyed (mdx_bg_create)
    DevBuf ring_pyr, ring_der, rin;          // resident frame ring (mdx_ring_*)
    DevBuf rfull;                            // mdx_ring_push_half: the full-size frame, halved into rin
    DevBuf hsrc, hdst;                       // mdx_resize_half (host entry): the frame and its half
    DevBuf wscr;                             // k_warp_prep's per-pair / per-tile tables
    mdx::WarpLaunch last_warp;               // the last launch_warp_diff (mdx_debug_warp_paths)
    DevBuf rsc;                              // MDX_FIT_RANSAC scratch (list, hypotheses, counts)
    std::vector<int> ring_order;             // held slots, oldest first
    int ring_cap = 0, ring_w = 0, ring_h = 0, ring_ml = -1;
    std::array<size_t, 4> lk_scratch_key{{0, 0, 0, 0}};      // (Abuf, levels, batch, points) of the last LK's scratch layout
    std::array<int, 6> plan_key{{-1, -1, -1, -1, -1, -1}};   // (w, h, pixel_step, levels, gy0, gy1) of `plan`
    int band_w = 0, band_h = 0;              // frame of the last mdx_band_flow_dev (its pyramids are live)
    mdx::ClassPlan plan{};
    bool timing = false;
    std::vector<hipEvent_t> ev;            // kSlots (mdx_api.cpp) x 7 events, once timing was enabled
    int ncalls = 0;                        // calls recorded since enable
    int cur = -1;                          // slot of the call in flight
    std::string err;
};

namespace mdx {

inline int set_err(mdx_ctx* c, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define HIP_OR_RETURN(c, expr)                                                                 \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return set_err((c), MDX_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));      \
    } while (0)

// mdx_enable_timing: event i (0 .. 6) of the timed call in flight, recorded on st (default: the context's
// stream); i == 0 opens the call's event set.  Nothing unless timing is on.
inline void mark(mdx_ctx* c, int i, hipStream_t st = nullptr)
{
    if (!c->timing || c->ev.empty()) return;
    if (i == 0) {
        c->cur = c->ncalls < (int)c->ev.size() / 7 ? c->ncalls : -1;
        c->ncalls++;
    }
    if (c->cur >= 0) (void)hipEventRecord(c->ev[c->cur * 7 + i], st ? st : c->stream);
}

inline int ensure(mdx_ctx* c, DevBuf& b, size_t need)
{
    if (need == 0) need = 1;
    if (b.p && b.cap >= need) return MDX_OK;
    if (b.p) (void)hipStreamSynchronize(c->stream);   // the aux stream's work is always joined by c->stream
    if (!b.alloc(need)) return set_err(c, MDX_ENOMEM, "hipMalloc(%zu) failed", need);
    return MDX_OK;
}

// mdx_input_ready is one-shot: the next device entry makes stream s wait for the caller's event, once
inline hipError_t wait_input_ready(mdx_ctx* c, hipStream_t s)
{
    if (!c->input_ev) return hipSuccess;
    hipEvent_t e = c->input_ev;
    c->input_ev = nullptr;
    return hipStreamWaitEvent(s, e, 0);
}

// n page-locked ints, the context's until mdx_destroy; null on failure
inline int* pinned_ints(mdx_ctx* c, int n)
{
    void* p = nullptr;
    if (hipHostMalloc(&p, sizeof(int) * n, hipHostMallocDefault) != hipSuccess) return nullptr;
    c->pinned.push_back(p);
    return static_cast<int*>(p);
}

// ensure() for each (buffer, bytes) pair in turn; stops at the first failure
inline int ensure_all(mdx_ctx* c, std::initializer_list<std::pair<DevBuf*, size_t>> needs)
{
    for (const auto& n : needs)
        if (const int rc = ensure(c, *n.first, n.second); rc != MDX_OK) return rc;
    return MDX_OK;
}

// Guard bytes kept free after the last pyramid slab of an allocation (one row of the last level).
// The lowest row an LK window reads is iny + kWin <= h - 1 + kWin, the level's last padding row
// (DESIGN.md §3.1): k_lk's plain loads of the next frame's window end exactly with the last level
// of the last slab, with no margin.  The guard keeps a window one row lower -- a bound off by one --
// inside the allocation instead of past it.  (k_lk_iter's J rows go through a range-checked
// descriptor as well.)
inline size_t slab_slack_bytes(const Geometry& g) { return ((size_t)g.lv[g.nlev - 1].pitch + 255) / 256 * 256; }

// With call pipelining the pyramid slabs hold two halves (ensure_workspace(.., two = true) makes the
// slab at least twice one call's pyramids); other users take the slab from its start.
inline size_t pyr_half_bytes(const DevBuf& b) { return b.cap / 2 / 256 * 256; }

inline int ensure_workspace(mdx_ctx* c, const Geometry& g, int batch, bool two)
{
    const size_t half = ((size_t)g.img_bytes * batch + 255) / 256 * 256 + slab_slack_bytes(g);
    return ensure_all(c, {{&c->pyr1, two ? 2 * half : half}, {&c->pyr2, two ? 2 * half : half},
                          {&c->der, (size_t)g.der_words * 4 * batch}, {&c->fits, sizeof(PairFit) * (size_t)batch}});
}

// Size, pixel format and stride of a caller's frame.  who: the entry's name, which prefixes the
// message ("who: ..."); null in the pair entries, whose messages carry no prefix.
inline int check_frame(mdx_ctx* c, const char* who, int w, int h, int stride, int fmt)
{
    const char* sep = who ? ": " : "";
    if (!who) who = "";
    if (w <= 0 || h <= 0) return set_err(c, MDX_EINVAL, "%s%sbad frame size", who, sep);
    if (fmt < MDX_FMT_GRAY8 || fmt > MDX_FMT_BGR8) return set_err(c, MDX_EINVAL, "%s%sbad pixel format %d", who, sep, fmt);
    const int cn = fmt == MDX_FMT_GRAY8 ? 1 : 3;
    if (stride < w * cn) return set_err(c, MDX_EINVAL, "%s%sstride %d < w*channels %d", who, sep, stride, w * cn);
    return MDX_OK;
}

// Bytes of a caller's host frame that are the caller's to read: h - 1 whole pitches and the last
// row's w * channels pixels.  A pitched view (a cv::Mat ROI) ends there, so the host entries copy
// this much; their device slots stay stride * h apart.
inline size_t frame_copy_bytes(int w, int h, int stride, int fmt)
{
    const int cn = fmt == MDX_FMT_GRAY8 ? 1 : 3;
    return (size_t)stride * (size_t)(h - 1) + (size_t)w * cn;
}

// The LkArgs fields every LK of a w x h frame shares: geometry, the full grid and the clamped
// iteration parameters.  The caller adds pyramids, outputs and start points.
inline LkArgs lk_args_for(const mdx_ctx* c, const Geometry& g, int w, int h)
{
    const mdx_params& P = c->prm;
    LkArgs a{};
    a.g = g;
    a.maxl = g.nlev - 1;
    a.npts = mdx_grid_count(w, h, P.pixel_step);
    a.ny = (h + P.pixel_step - 1) / P.pixel_step;
    a.nyg = a.ny;
    a.pixel_step = P.pixel_step;
    a.max_iters = std::min(std::max(P.max_iters, 0), 100);
    a.min_eig = P.min_eig;
    const double e = std::min(std::max(P.eps, 0.), 10.);
    a.eps2 = e * e;
    return a;
}

// Non-pipelined users of the pyramid / derivative slabs (from the slab start, any size): the next
// pipelined call's front end and aux work wait for them through both halves' events.
inline void release_pyr_all(mdx_ctx* c)
{
    for (hipEvent_t e : c->pyr_free)
        if (e) (void)hipEventRecord(e, c->stream);
}

// mdx_pair.cpp: the LK of a batch of pairs on the context's stream (the per-pass trajectory LK too)
int run_lk(mdx_ctx* c, const Geometry& g, LkArgs& a, int batch, int w, int h, int gy0, int gy1, bool have_scharr,
           hipEvent_t prev_ready = nullptr);
bool host_block_holds(const void* p, size_t bytes);   // mdx_api.cpp: inside one mdx_host_alloc block

}  // namespace mdx
