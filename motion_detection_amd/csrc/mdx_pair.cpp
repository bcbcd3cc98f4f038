// mdx_pair.cpp -- the per-call pair pipeline
//   gray+pad -> pyrDown x L (both frames) -> Scharr x (L+1) -> LK -> classify+fit -> warp+diff
// enqueued on the context's HIP streams.  Replaces OpticalFlowCalculator::calculateOpticalFlow
// (reference common/src/optical_flow_calculator.cpp:30-130); no allocation on the per-frame
// path once the workspace fits the frame size.  Also the entries that run parts of it: the
// warp-only and probe entries and the row bands.
#include "mdx_ctx.h"

#include <cmath>
#include <cstdlib>
#include <new>

using namespace mdx;

// The context's class plan (mdx_plan.h build_class_plan) and its device side: the tables in ctab and
// the class slab of `batch` pairs.  Rebuilt and uploaded only when frame size / pixel_step / levels /
// band change.  plan.nch == 0: the caller runs the single-kernel LK instead.
static int ensure_class_plan(mdx_ctx* c, const Geometry& g, int w, int h, int ps, int batch, int gy0, int gy1)
{
    int rc;
    const std::array<int, 6> key = {w, h, ps, g.nlev, gy0, gy1};
    if (c->plan_key != key) {
        BuiltPlan B;
        try {
            B = build_class_plan(g, w, h, ps, gy0, gy1, PlanTuning{c->lk_g, c->lk_astrip, c->max_batch});
        } catch (const std::bad_alloc&) {
            return set_err(c, MDX_ENOMEM, "class plan: out of host memory");
        }
        if ((rc = ensure(c, c->ctab, B.tab.size() * sizeof(int16_t))) != MDX_OK) return rc;
        // kernels of earlier calls may still read the old tables: the copy waits for them (the
        // stream is non-blocking, so a plain hipMemcpy would not)
        HIP_OR_RETURN(c, hipStreamSynchronize(c->stream));
        HIP_OR_RETURN(c, hipMemcpy(c->ctab.p, B.tab.data(), B.tab.size() * sizeof(int16_t), hipMemcpyHostToDevice));
        c->plan = B.plan;
        c->plan_key = key;
    }
    if (c->plan.nch == 0) return MDX_OK;
    return ensure(c, c->cls, (size_t)c->plan.bytes_per_pair * batch + 64);
}

// The next device call's first stage waits for the caller's input event (mdx_input_ready), once.
static int wait_input(mdx_ctx* c, hipStream_t st)
{
    if (!c->input_ev) return MDX_OK;
    hipEvent_t e = c->input_ev;
    c->input_ev = nullptr;
    HIP_OR_RETURN(c, hipStreamWaitEvent(st, e, 0));
    return MDX_OK;
}

// The LK of a batch of pairs on the context's stream.  Grid start points (a.prev_pts null) on a
// dense enough grid take the class-plane kernels, which launch each level's Scharr planes
// themselves; otherwise the single kernel, after the Scharr planes unless the caller already
// computed them (have_scharr).  a: every field but the class-plan ones.
int mdx::run_lk(mdx_ctx* c, const Geometry& g, LkArgs& a, int batch, int w, int h, int gy0, int gy1, bool have_scharr,
                hipEvent_t prev_ready)
{
    int rc;
    hipStream_t s = c->stream;
    bool v2 = c->lk_impl == 2 && a.prev_pts == nullptr;
    if (v2) {
        if ((rc = ensure_class_plan(c, g, w, h, c->prm.pixel_step, batch, gy0, gy1)) != MDX_OK) return rc;
        v2 = c->plan.nch != 0;   // very sparse grids: the single-kernel LK
    }
    if (!v2) {
        if (gy0 != 0 || gy1 != a.ny)
            return set_err(c, MDX_EINVAL, "row bands need the class-plane LK (pixel_step too large)");
        if (!have_scharr) HIP_OR_RETURN(c, launch_scharr_levels(s, batch, a.pyr1, const_cast<uint32_t*>(a.der), g));
        HIP_OR_RETURN(c, launch_lk(s, batch, a));
        return MDX_OK;
    }
    a.plan = c->plan;
    a.max_sub = c->lk_sub;
    a.err = c->errw.as<int>();
    a.spin_max = c->spin_max;
    a.flow_cap = c->lk_cap;
    a.fma = c->lk_fma ? 1 : 0;
    a.cmap = c->ctab.as<int16_t>();
    a.rlist = c->ctab.as<int16_t>() + kTabRlist;
    a.ord = c->ctab.as<int16_t>() + kTabOrd;
    const int npts = a.npts;
    if (c->lk_debug) {
        if ((rc = ensure(c, c->dbg, ((size_t)npts * g.nlev * batch + kLkDbgStampOff + kMaxLevels * kLkDbgWaves) * 16)) !=
            MDX_OK)
            return rc;
        a.dbg = c->dbg.as<float4>();
        const char* e = std::getenv("MDX_LK_DEBUG_PT");
        a.dbg_pt = e ? std::atoi(e) : -1;
        // this call's wave-iterations by row body (mdx_debug_copy selector 6)
        if ((rc = ensure(c, c->lkcnt, kMaxLevels * 2 * sizeof(uint32_t))) != MDX_OK) return rc;
        HIP_OR_RETURN(c, hipMemsetAsync(c->lkcnt.p, 0, kMaxLevels * 2 * sizeof(uint32_t), s));
        a.body_cnt = c->lkcnt.as<uint32_t>();
    }
    const LkScratch sc = lk_scratch(g.nlev, batch, npts);
    if ((rc = ensure(c, c->Abuf, sc.bytes)) != MDX_OK) return rc;
    // A pipelined call's aux work waits for the previous call's iterations level by level (lvl_done),
    // which keeps the two calls apart only while both put a level's A sums and queue heads in the
    // same place: when the layout moves, everything enqueued so far finishes first
    const std::array<size_t, 4> lay = {reinterpret_cast<size_t>(c->Abuf.p), (size_t)g.nlev, (size_t)batch, (size_t)npts};
    if (c->lk_scratch_key != lay) {
        HIP_OR_RETURN(c, hipStreamSynchronize(c->stream));
        c->lk_scratch_key = lay;
    }
    uint8_t* base = c->Abuf.as<uint8_t>();
    a.carry = reinterpret_cast<float*>(base + sc.carry);
    a.carry_lstride = (long long)(sc.carry_level / sizeof(float));
    LkLaunch L = c->lk;
    L.cls = c->cls.as<uint8_t>();
    L.Ab = c->Abuf.as<float4>();
    L.cert = base + sc.cert;
    L.qctr = reinterpret_cast<int*>(base + sc.qctr);
    L.done = reinterpret_cast<int*>(base + sc.done);
    L.lvl_done = c->prm.call_pipelining ? c->lvl_done : nullptr;
    L.prev_ready = prev_ready;
    HIP_OR_RETURN(c, launch_lk_v2(L, batch, a));
    return MDX_OK;
}

// The warp+diff stage of every entry, on c->stream: k_warp_prep's scratch, the launch, and its
// record for the path report (mdx_debug_warp_paths).
static int run_warp_diff(mdx_ctx* c, int batch, const WarpArgs& a)
{
    const size_t wsb = warp_scratch_bytes(batch, a.w, (a.row1 < 0 ? a.h : a.row1) - a.row0);
    if (const int rc = ensure(c, c->wscr, wsb); rc != MDX_OK) return rc;
    HIP_OR_RETURN(c, launch_warp_diff(c->stream, batch, a, c->wscr.p, wsb, &c->last_warp));
    return MDX_OK;
}
// a pyramid slab's gray frames as a warp operand
static GrayPlane pyr_gray(uint8_t* slab, const Geometry& g)
{
    return {level0_core(slab, g), g.img_bytes, g.lv[0].pitch};
}

// The pipeline on device buffers: a call's frames, outputs and (row-band mode) band.
struct PipelineArgs {
    int batch;
    const uint8_t *d_img1, *d_img2;   // [batch] frames, frame_stride bytes apart
    int w, h, stride;
    size_t frame_stride;
    int fmt;
    float* d_np;                      // [batch][npts][2]: must be valid (the LK writes them), as d_st
    uint8_t* d_st;                    // [batch][npts]
    double* d_vec = nullptr;          // the optional outputs: Vec4d, mask, H, num_vectors
    uint8_t* d_mask = nullptr;
    double* d_H = nullptr;
    int* d_num = nullptr;
    const double* d_Hext = nullptr;   // MDX_FIT_EXTERNAL
    // Row-band mode (cand != null, batch 1): LK and classification for grid rows [gy0, gy1) only
    // (gy1 < 0: every row), the band's record to *cand, no fit and no mask.
    int gy0 = 0, gy1 = -1;
    mdx_band_cand* cand = nullptr;
    bool may_overlap = false;         // a device entry: call pipelining may run this call's front end early
};
static int run_pipeline(mdx_ctx* c, const PipelineArgs& A)
{
    const mdx_params& P = c->prm;
    const int batch = A.batch, w = A.w, h = A.h, stride = A.stride, fmt = A.fmt;
    mdx_band_cand* const cand = A.cand;
    if (w <= 0 || h <= 0 || batch <= 0) return set_err(c, MDX_EINVAL, "bad frame size or batch");
    int rc = check_frame(c, nullptr, w, h, stride, fmt);
    if (rc != MDX_OK) return rc;
    if (batch > 1 && A.frame_stride < (size_t)stride * h) return set_err(c, MDX_EINVAL, "frame_stride too small");
    if (P.fit_mode == MDX_FIT_EXTERNAL && !A.d_Hext) return set_err(c, MDX_EINVAL, "fit_mode EXTERNAL needs H_external");
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    // call pipelining: this call's pyramids go to the half the previous call did not use, and its
    // front end runs on the front stream once that half's last reader (two calls back) is done
    const bool pipe = A.may_overlap && P.call_pipelining && c->aux && c->lk_impl == 2;
    Geometry g = make_geometry(w, h, P.max_level);
    if ((rc = ensure_workspace(c, g, batch, pipe)) != MDX_OK) return rc;
    const int npts = mdx_grid_count(w, h, P.pixel_step);
    const int ny = (h + P.pixel_step - 1) / P.pixel_step;
    const int gy0 = A.gy0, gy1 = A.gy1 < 0 ? ny : A.gy1;
    const int nyb = gy1 - gy0;
    hipStream_t s = c->stream;
    uint8_t* pyr1 = c->pyr1.as<uint8_t>();
    uint8_t* pyr2 = c->pyr2.as<uint8_t>();
    uint32_t* der = c->der.as<uint32_t>();
    PairFit* fits = c->fits.as<PairFit>();
    hipStream_t fs_ = s;
    int half = 0;
    if (pipe) {
        half = c->pyr_half;
        c->pyr_half ^= 1;
        pyr1 += half * pyr_half_bytes(c->pyr1);
        pyr2 += half * pyr_half_bytes(c->pyr2);
        fs_ = c->aux;
        HIP_OR_RETURN(c, hipStreamWaitEvent(fs_, c->pyr_free[half], 0));
    }
    if ((rc = wait_input(c, fs_)) != MDX_OK) return rc;
    c->last_pyr1 = pyr1;
    c->last_pyr2 = pyr2;
    // a row band's fit/warp reads these pyramids; any other call voids the band's
    if (cand) {
        c->band_pyr1 = pyr1;
        c->band_pyr2 = pyr2;
        c->band_half = half;
    } else {
        c->band_w = c->band_h = 0;
    }

    mark(c, 0, fs_);
    // The class planes and A sums need only the first frames' pyramids: build those first and let
    // the aux stream start on them while the second frames' pyramids are built.  Stage "gray_pad"
    // = gray + pad + level 1 of the first frames (k_front), "pyrdown" = the rest of the pyramids.
    hipEvent_t prev_ready = nullptr;
    const uint8_t *d_img1 = A.d_img1, *d_img2 = A.d_img2;
    const long long fs = (long long)A.frame_stride;
    // a row band (batch 1): the rows of the previous frame's pyramid its class planes read
    RowSpan rows[kMaxLevels] = {};   // band_built_rows reads rows[1] on a one-level pyramid too
    const RowSpan* prows = nullptr;
    if (cand && c->lk_impl == 2 && npts > 0 && nyb > 0 && nyb < ny) {
        if ((rc = ensure_class_plan(c, g, w, h, P.pixel_step, batch, gy0, gy1)) != MDX_OK) return rc;
        if (c->plan.nch != 0) {
            band_rows(g, c->plan, rows);
            prows = rows;
        }
    }
    // level-0 rows of frame 1 this call builds (mdx_band_fit_warp_dev converts the others it needs)
    const RowSpan built = prows ? band_built_rows(rows, h) : RowSpan{0, h};
    c->band_built[0] = built.lo;
    c->band_built[1] = built.hi;
    if (c->aux && c->lk_impl == 2) {
        HIP_OR_RETURN(c, launch_front(fs_, batch, d_img1, d_img2, w, h, stride, fs, fmt, pyr1, pyr2, g, 1, prows));
        mark(c, 1, fs_);
        HIP_OR_RETURN(c, launch_pyr_levels(fs_, batch, pyr1, pyr2, g, 1, prows));
        HIP_OR_RETURN(c, hipEventRecord(c->lkev[kMaxLevels + 1], fs_));
        prev_ready = c->lkev[kMaxLevels + 1];
        HIP_OR_RETURN(c, launch_front(fs_, batch, d_img1, d_img2, w, h, stride, fs, fmt, pyr1, pyr2, g, 2));
        HIP_OR_RETURN(c, launch_pyr_levels(fs_, batch, pyr1, pyr2, g, 2));
        if (pipe) {
            mark(c, 2, fs_);
            HIP_OR_RETURN(c, hipEventRecord(c->front_ev, fs_));
            HIP_OR_RETURN(c, hipStreamWaitEvent(s, c->front_ev, 0));
        }
    } else {
        HIP_OR_RETURN(c, launch_front(s, batch, d_img1, d_img2, w, h, stride, fs, fmt, pyr1, pyr2, g));
        mark(c, 1);
        HIP_OR_RETURN(c, launch_pyr_levels(s, batch, pyr1, pyr2, g));
    }
    if (!pipe) mark(c, 2);
    // Scharr derivatives feed only the LK.  The class-plane LK launches them itself, on its
    // aux stream right before each level's class planes, so they overlap the coarser levels'
    // iterations; the single-kernel LK needs them up front.
    mark(c, 3);
    if (npts > 0 && nyb > 0) {
        LkArgs a = lk_args_for(c, g, w, h);
        a.pyr1 = pyr1;
        a.pyr2 = pyr2;
        a.der = der;
        a.nyg = nyb;
        a.next_pts = A.d_np;
        a.status = A.d_st;
        if ((rc = run_lk(c, g, a, batch, w, h, gy0, gy1, false, prev_ready)) != MDX_OK) return rc;
    }
    mark(c, 4);
    if ((rc = ensure(c, c->csum, classify_scratch_bytes(batch, npts))) != MDX_OK) return rc;
    FitArgs fa = {A.d_np, A.d_st, npts, ny, P.pixel_step, gy0, gy1, P.min_vector_size, A.d_vec, fits, P.fit_mode,
                  A.d_Hext, c->csum.p, cand, RansacArgs{}};
    if (P.fit_mode == MDX_FIT_RANSAC && !cand) {
        if ((rc = ensure(c, c->rsc, ransac_scratch_bytes(batch, npts, P.ransac_iters))) != MDX_OK) return rc;
        fa.ransac = ransac_args(c->rsc.p, batch, npts, P);
    }
    HIP_OR_RETURN(c, launch_classify_fit(s, batch, fa));
    mark(c, 5);
    if (A.d_mask && !cand) {
        const WarpArgs wa = {pyr_gray(pyr1, g), pyr_gray(pyr2, g), w, h, fits, A.d_mask, (long long)w * h, P.thresh};
        if ((rc = run_warp_diff(c, batch, wa)) != MDX_OK) return rc;
    }
    if ((A.d_H || A.d_num) && !cand) HIP_OR_RETURN(c, launch_export_fit(s, batch, fits, A.d_H, A.d_num));
    // (a row band: mdx_band_fit_warp_dev reads these pyramids, whichever half they are in, and
    // records their release again after its warp)
    if (pipe) HIP_OR_RETURN(c, hipEventRecord(c->pyr_free[half], s));
    else release_pyr_all(c);
    mark(c, 6);
    return MDX_OK;
}

extern "C" int mdx_flow_warp_diff_batch_dev(mdx_ctx* c, int batch, const uint8_t* d_img1, const uint8_t* d_img2,
                                            int w, int h, int stride, size_t frame_stride, int fmt, float* d_next_pts,
                                            uint8_t* d_status, double* d_vectors, uint8_t* d_mask, double* d_H,
                                            const double* d_H_external, int* d_num_vectors)
{
    if (!c) return MDX_EINVAL;
    if (!d_img1 || !d_img2 || batch <= 0) return set_err(c, MDX_EINVAL, "null frame pointer or batch <= 0");
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    const size_t need = (size_t)mdx_grid_count(w, h, c->prm.pixel_step) * batch;
    int rc;
    if (!d_next_pts) {
        if ((rc = ensure(c, c->bnp, need * 8)) != MDX_OK) return rc;
        d_next_pts = c->bnp.as<float>();
    }
    if (!d_status) {
        if ((rc = ensure(c, c->bst, need)) != MDX_OK) return rc;
        d_status = c->bst.as<uint8_t>();
    }
    PipelineArgs A = {batch, d_img1, d_img2, w, h, stride, frame_stride, fmt, d_next_pts, d_status,
                      d_vectors, d_mask, d_H, d_num_vectors, d_H_external};
    A.may_overlap = true;
    return run_pipeline(c, A);
}

extern "C" int mdx_flow_warp_diff(mdx_ctx* c, const uint8_t* img1, const uint8_t* img2, int w, int h, int stride,
                                  int fmt, float* next_pts, uint8_t* status, double* vectors, uint8_t* mask, double* H,
                                  const double* H_external, int* num_vectors)
{
    if (!c) return MDX_EINVAL;
    if (!img1 || !img2) return set_err(c, MDX_EINVAL, "null frame pointer");
    int rc = check_frame(c, nullptr, w, h, stride, fmt);
    if (rc != MDX_OK) return rc;
    if (c->prm.fit_mode == MDX_FIT_EXTERNAL && !H_external)
        return set_err(c, MDX_EINVAL, "fit_mode EXTERNAL needs H_external");
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    const size_t in_bytes = (size_t)stride * h;                    // device slot
    const size_t copy_bytes = frame_copy_bytes(w, h, stride, fmt);   // what the caller's frame holds
    const int npts = mdx_grid_count(w, h, c->prm.pixel_step);
    const size_t pts = (size_t)(npts > 0 ? npts : 1);
    if ((rc = ensure_all(c, {{&c->in1, in_bytes}, {&c->in2, in_bytes}, {&c->np, pts * 8}, {&c->st, pts},
                             {&c->vec, pts * 32}, {&c->mask, (size_t)w * h}, {&c->H, 72}, {&c->Hext, 72},
                             {&c->num, 4}})) != MDX_OK)
        return rc;

    hipStream_t s = c->stream;
    HIP_OR_RETURN(c, hipMemcpyAsync(c->in1.p, img1, copy_bytes, hipMemcpyHostToDevice, s));
    HIP_OR_RETURN(c, hipMemcpyAsync(c->in2.p, img2, copy_bytes, hipMemcpyHostToDevice, s));
    if (H_external) HIP_OR_RETURN(c, hipMemcpyAsync(c->Hext.p, H_external, 72, hipMemcpyHostToDevice, s));
    const PipelineArgs A = {1, c->in1.as<uint8_t>(), c->in2.as<uint8_t>(), w, h, stride, in_bytes, fmt, c->np.as<float>(),
                            c->st.as<uint8_t>(), vectors ? c->vec.as<double>() : nullptr,
                            mask ? c->mask.as<uint8_t>() : nullptr, c->H.as<double>(), c->num.as<int>(),
                            H_external ? c->Hext.as<double>() : nullptr};
    if ((rc = run_pipeline(c, A)) != MDX_OK) return rc;
    int num = 0;
    if (next_pts && npts > 0) HIP_OR_RETURN(c, hipMemcpyAsync(next_pts, c->np.p, (size_t)npts * 8, hipMemcpyDeviceToHost, s));
    if (status && npts > 0) HIP_OR_RETURN(c, hipMemcpyAsync(status, c->st.p, (size_t)npts, hipMemcpyDeviceToHost, s));
    if (vectors && npts > 0) HIP_OR_RETURN(c, hipMemcpyAsync(vectors, c->vec.p, (size_t)npts * 32, hipMemcpyDeviceToHost, s));
    if (mask) HIP_OR_RETURN(c, hipMemcpyAsync(mask, c->mask.p, (size_t)w * h, hipMemcpyDeviceToHost, s));
    if (H) HIP_OR_RETURN(c, hipMemcpyAsync(H, c->H.p, 72, hipMemcpyDeviceToHost, s));
    HIP_OR_RETURN(c, hipMemcpyAsync(&num, c->num.p, 4, hipMemcpyDeviceToHost, s));
    HIP_OR_RETURN(c, hipStreamSynchronize(s));
    if (num_vectors) *num_vectors = num;
    if (c->prm.fit_mode != MDX_FIT_EXTERNAL && num < 4) return MDX_EDEGENERATE;
    return MDX_OK;
}

extern "C" int mdx_warp_diff_dev(mdx_ctx* c, int batch, const uint8_t* d_gray1, const uint8_t* d_gray2, int w, int h,
                                 int stride, size_t frame_stride, const double* d_H, uint8_t* d_mask)
{
    if (!c) return MDX_EINVAL;
    if (!d_gray1 || !d_gray2 || !d_H || !d_mask || batch <= 0 || w <= 0 || h <= 0 || stride < w)
        return set_err(c, MDX_EINVAL, "mdx_warp_diff_dev: bad argument");
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    int rc = ensure(c, c->fits, sizeof(PairFit) * (size_t)batch);
    if (rc != MDX_OK) return rc;
    hipStream_t s = c->stream;
    PairFit* fits = c->fits.as<PairFit>();
    if ((rc = wait_input(c, s)) != MDX_OK) return rc;
    for (int i = 0; i < 5; i++) mark(c, i);
    HIP_OR_RETURN(c, launch_set_fit_external(s, batch, d_H, fits));
    mark(c, 5);
    const long long fs = (long long)frame_stride;
    const WarpArgs wa = {{d_gray1, fs, stride}, {d_gray2, fs, stride}, w, h, fits, d_mask, (long long)w * h, c->prm.thresh};
    if ((rc = run_warp_diff(c, batch, wa)) != MDX_OK) return rc;
    mark(c, 6);
    return MDX_OK;
}

extern "C" int mdx_probe_stream3_dev(mdx_ctx* c, size_t n, const uint8_t* d_a, const uint8_t* d_b, uint8_t* d_mask,
                                     int thresh)
{
    if (!c) return MDX_EINVAL;
    if (!d_a || !d_b || !d_mask || n == 0 || n % 16 || ((uintptr_t)d_a | (uintptr_t)d_b | (uintptr_t)d_mask) % 16)
        return set_err(c, MDX_EINVAL, "mdx_probe_stream3_dev: bad argument");
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    for (int i = 0; i < 6; i++) mark(c, i);
    HIP_OR_RETURN(c, launch_stream3(c->stream, n, d_a, d_b, d_mask, thresh));
    mark(c, 6);
    return MDX_OK;
}

extern "C" int mdx_band_flow_dev(mdx_ctx* c, const uint8_t* d_img1, const uint8_t* d_img2, int w, int h, int stride,
                                 int fmt, int y0, int y1, float* d_next_pts, uint8_t* d_status, double* d_vectors,
                                 mdx_band_cand* d_cand)
{
    if (!c) return MDX_EINVAL;
    if (!d_img1 || !d_img2 || !d_next_pts || !d_status || !d_cand)
        return set_err(c, MDX_EINVAL, "mdx_band_flow_dev: null pointer");
    if (w <= 0 || h <= 0 || y0 < 0 || y1 > h || y0 >= y1) return set_err(c, MDX_EINVAL, "bad band [%d, %d) of %d rows", y0, y1, h);
    if (c->prm.fit_mode != MDX_FIT_FIRST4) return set_err(c, MDX_EINVAL, "row bands need fit_mode FIRST4");
    const int ps = c->prm.pixel_step;
    // grid rows whose y = gy*ps lies in [y0, y1)
    const int gy0 = (y0 + ps - 1) / ps, gy1 = (y1 + ps - 1) / ps;
    c->band_w = c->band_h = 0;
    PipelineArgs A = {1, d_img1, d_img2, w, h, stride, (size_t)stride * h, fmt, d_next_pts, d_status, d_vectors};
    A.gy0 = gy0;
    A.gy1 = gy1;
    A.cand = d_cand;
    A.may_overlap = true;
    const int rc = run_pipeline(c, A);
    if (rc == MDX_OK) {
        c->band_w = w;
        c->band_h = h;
        c->band_img1 = d_img1;
        c->band_stride = stride;
        c->band_fmt = fmt;
    }
    return rc;
}

extern "C" int mdx_band_fit_warp_dev(mdx_ctx* c, int nrec, const mdx_band_cand* d_cands, int y0, int y1,
                                     uint8_t* d_mask_band, double* d_H, int* d_num_vectors)
{
    if (!c) return MDX_EINVAL;
    if (nrec <= 0 || !d_cands || !d_mask_band) return set_err(c, MDX_EINVAL, "mdx_band_fit_warp_dev: bad argument");
    const int w = c->band_w, h = c->band_h;
    if (w <= 0 || h <= 0)
        return set_err(c, MDX_EINVAL, "mdx_band_fit_warp_dev: no mdx_band_flow_dev before, or another call rebuilt "
                                      "the context's pyramids since");
    if (y0 < 0 || y1 > h || y0 >= y1) return set_err(c, MDX_EINVAL, "bad band [%d, %d) of %d rows", y0, y1, h);
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    const Geometry g = make_geometry(w, h, c->prm.max_level);
    hipStream_t s = c->stream;
    PairFit* fits = c->fits.as<PairFit>();
    if (!c->band_pyr1 || !c->band_img1) return set_err(c, MDX_EINVAL, "mdx_band_fit_warp_dev: no mdx_band_flow_dev before");
    HIP_OR_RETURN(c, launch_band_fit(s, nrec, d_cands, fits, w, h, y0, y1));
    // the band's flow built frame 1's pyramid for its own rows only: the rows this band's warp
    // reads beyond them (the fit is known now) are converted from the frame
    HIP_OR_RETURN(c, launch_gray_rows(s, c->band_img1, w, c->band_stride, c->band_fmt, level0_core(c->band_pyr1, g),
                                      g.lv[0].pitch, fits, c->band_built[0], c->band_built[1]));
    const WarpArgs wa = {pyr_gray(c->band_pyr1, g), pyr_gray(c->band_pyr2, g), w, h, fits, d_mask_band,
                         (long long)w * (y1 - y0), c->prm.thresh, y0, y1};
    if (const int rc = run_warp_diff(c, 1, wa); rc != MDX_OK) return rc;
    if (d_H || d_num_vectors) HIP_OR_RETURN(c, launch_export_fit(s, 1, fits, d_H, d_num_vectors));
    // the band's pyramids have been read: the pipelined call two calls on may overwrite them
    if (c->prm.call_pipelining) HIP_OR_RETURN(c, hipEventRecord(c->pyr_free[c->band_half], s));
    else release_pyr_all(c);
    return MDX_OK;
}
