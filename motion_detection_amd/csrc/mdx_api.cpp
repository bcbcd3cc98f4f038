// mdx_api.cpp -- host side of the C-ABI (include/mdx.h): parameters, context lifetime (the device
// workspace is sized once at create time), the environment knobs, sync points, stage timing,
// error and allocation entries and the debug hooks.  The pair pipeline is mdx_pair.cpp, the
// trajectories and the ring mdx_traj.cpp, the subspace fit and clustering mdx_post.cpp.
#include "mdx_ctx.h"

#include <cstdlib>
#include <map>
#include <mutex>

using namespace mdx;

static thread_local std::string g_create_err;

extern "C" void mdx_default_params(mdx_params* p)
{
    p->win = 40;
    p->max_level = 5;
    p->max_iters = 10;
    p->eps = 0.03;
    p->min_eig = 0.001f;
    p->thresh = 190;
    p->pixel_step = 10;
    p->min_vector_size = 1.0;
    p->fit_mode = MDX_FIT_FIRST4;
    p->subspace_precision = MDX_SUBSPACE_F64;
    p->call_pipelining = 0;
    p->ransac_iters = 128;
    p->ransac_thresh = 3.0;
    p->ransac_seed = 20141105u;
}

extern "C" int mdx_grid_count(int w, int h, int ps)
{
    if (w <= 0 || h <= 0 || ps <= 0) return 0;
    return ((w + ps - 1) / ps) * ((h + ps - 1) / ps);
}

// null, or why the parameters are not supported
static const char* check_params(const mdx_params* p)
{
    if (p->win != kWin) return "only win == 40 (the reference constant) is supported";
    if (p->max_level < 0 || p->max_level >= kMaxLevels) return "max_level out of range [0, 7]";
    if (p->pixel_step <= 0) return "pixel_step must be > 0 (reference leaves it unset: UB)";
    if (p->fit_mode != MDX_FIT_FIRST4 && p->fit_mode != MDX_FIT_EXTERNAL && p->fit_mode != MDX_FIT_RANSAC) return "bad fit_mode";
    if (p->ransac_iters < 1 || p->ransac_iters > kRansacMaxIters) return "ransac_iters must be in [1, 1024]";
    if (!(p->ransac_thresh >= 0.0) || !(p->ransac_thresh < 1e6)) return "ransac_thresh must be in [0, 1e6)";
    if (p->subspace_precision != MDX_SUBSPACE_F64 && p->subspace_precision != MDX_SUBSPACE_F32) return "bad subspace_precision";
    if (p->call_pipelining != 0 && p->call_pipelining != 1) return "call_pipelining must be 0 or 1";
    return nullptr;
}

// Page-locked blocks handed out by mdx_host_alloc: [base, base + bytes).  The trajectory entry
// writes its outputs straight into them only when a whole output range lies inside one block.
static std::mutex g_host_mu;
static std::map<uintptr_t, size_t> g_host_blocks;
bool mdx::host_block_holds(const void* p, size_t bytes)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    std::lock_guard<std::mutex> lk(g_host_mu);
    auto it = g_host_blocks.upper_bound(a);
    if (it == g_host_blocks.begin()) return false;
    --it;
    return a >= it->first && bytes <= it->second && a - it->first <= it->second - bytes;
}

extern "C" const char* mdx_create_error(void) { return g_create_err.c_str(); }
extern "C" int mdx_abi_version(void) { return MDX_ABI_VERSION; }
extern "C" size_t mdx_params_size(void) { return sizeof(mdx_params); }

// Every MDX_* environment knob, read once per context (INTEGRATION.md lists them).  MDX_LK_DEBUG_PT
// alone is read per call (run_lk).
static LkTuning read_tuning()
{
    LkTuning t;
    auto num = [](const char* name, int dflt) {
        const char* e = std::getenv(name);
        return e ? std::atoi(e) : dflt;
    };
    t.lk_impl = num("MDX_LK_IMPL", 2) == 1 ? 1 : 2;
    t.lk_g = num("MDX_LK_G", 0);
    t.lk_sub = num("MDX_LK_SUB", 0);
    t.lk_astrip = std::max(0, std::min(num("MDX_LK_ASTRIP", 0), 64));
    t.lk_debug = num("MDX_LK_DEBUG", 0) != 0;
    t.traj_chain = num("MDX_TRAJ_CHAIN", 1) != 0;
    const int ppw = num("MDX_TRAJ_PPW", 4);
    t.traj_ppw = ppw == 1 ? 1 : ppw == 2 ? 2 : 4;
    t.lk_aux = num("MDX_LK_AUX", 1) != 0;
    t.lk_flow = num("MDX_LK_FLOW", 1) != 0;
    t.ol_reg = num("MDX_OL_REG", 1) != 0;
    t.lk_cap = std::min(std::max(num("MDX_LK_CAP", 75), 10), 100);
    t.lk_fma = num("MDX_LK_FMA", 1) != 0;
    t.spin_max = num("MDX_LK_SPIN_MAX", kLkSpinDefault);
    return t;
}

// Streams and events are created through these, so that mdx_destroy finds every one in the lists.
static bool new_stream(mdx_ctx* c, hipStream_t* s)
{
    if (hipStreamCreateWithFlags(s, hipStreamNonBlocking) != hipSuccess) {
        *s = nullptr;
        return false;
    }
    c->streams.push_back(*s);
    return true;
}

static bool new_events(mdx_ctx* c, hipEvent_t* e, int n, unsigned flags = hipEventDisableTiming)
{
    for (int i = 0; i < n; i++) {
        if (hipEventCreateWithFlags(&e[i], flags) != hipSuccess) return false;   // e[i] stays null
        c->events.push_back(e[i]);
    }
    return true;
}

extern "C" mdx_ctx* mdx_create(int device, int max_w, int max_h, int max_batch, const mdx_params* p)
{
    g_create_err.clear();
    mdx_params prm;
    if (p) prm = *p;
    else mdx_default_params(&prm);
    if (const char* why = check_params(&prm)) { g_create_err = why; return nullptr; }
    if (max_w <= 0 || max_h <= 0 || max_batch <= 0) { g_create_err = "max_w/max_h/max_batch must be > 0"; return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { g_create_err = "no HIP device visible"; return nullptr; }
    if (device < 0 || device >= ndev) { g_create_err = "device index out of range"; return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { g_create_err = "hipSetDevice failed"; return nullptr; }
    mdx_ctx* c = new mdx_ctx();
    c->device = device;
    c->prm = prm;
    c->max_w = max_w;
    c->max_h = max_h;
    c->max_batch = max_batch;
    static_cast<LkTuning&>(*c) = read_tuning();
    // every failure exit: the message, then mdx_destroy releases whatever exists so far
    auto fail = [&](const std::string& msg) -> mdx_ctx* {
        g_create_err = msg;
        mdx_destroy(c);
        return nullptr;
    };
    if (!new_stream(c, &c->stream)) return fail("hipStreamCreate failed");
    if (c->lk_aux) {
        bool ok = new_stream(c, &c->aux) && new_events(c, c->lkev, kMaxLevels + 2);
        if (ok && c->lk_flow)
            ok = new_stream(c, &c->iter2) && new_events(c, c->flowev, 2) && new_events(c, c->redo_ev, kMaxLevels);
        // call pipelining's events (mdx_params.call_pipelining may be switched on at any call)
        ok = ok && new_events(c, &c->front_ev, 1) && new_events(c, c->pyr_free, 2) && new_events(c, c->lvl_done, kMaxLevels);
        if (!ok) return fail("aux stream / event creation failed");
    }
    c->lk = LkLaunch{c->stream, c->aux, c->iter2, c->lkev, c->flowev, c->iter2 ? c->redo_ev : nullptr};
    if (ensure(c, c->errw, 16) != MDX_OK || hipMemset(c->errw.p, 0, 16) != hipSuccess || !(c->err_host = pinned_ints(c, 4)))
        return fail("error-word allocation failed");
    Geometry g = make_geometry(max_w, max_h, prm.max_level);
    if (ensure_workspace(c, g, max_batch, prm.call_pipelining != 0) != MDX_OK) return fail(c->err);
    return c;
}

extern "C" int mdx_destroy(mdx_ctx* c)
{
    if (!c) return MDX_EINVAL;
    (void)hipSetDevice(c->device);
    for (hipStream_t s : {c->stream, c->aux, c->iter2})   // aux: pipelined front ends
        if (s) (void)hipStreamSynchronize(s);
    for (hipEvent_t e : c->events) (void)hipEventDestroy(e);
    for (hipStream_t s : c->streams) (void)hipStreamDestroy(s);
    for (void* p : c->pinned) (void)hipHostFree(p);
    delete c;   // the device buffers free themselves
    return MDX_OK;
}

extern "C" const char* mdx_last_error(const mdx_ctx* c) { return c ? c->err.c_str() : "null context"; }
extern "C" void* mdx_stream(mdx_ctx* c) { return c ? (void*)c->stream : nullptr; }
extern "C" int mdx_device(const mdx_ctx* c) { return c ? c->device : -1; }
extern "C" int mdx_device_pci(const mdx_ctx* c, char* buf, int len)
{
    if (!c || !buf || len < 16) return MDX_EINVAL;
    return hipDeviceGetPCIBusId(buf, len, c->device) == hipSuccess ? MDX_OK : MDX_EHIP;
}

extern "C" int mdx_set_params(mdx_ctx* c, const mdx_params* p)
{
    if (!c || !p) return MDX_EINVAL;
    if (const char* why = check_params(p)) return set_err(c, MDX_EINVAL, "%s", why);
    c->prm = *p;
    return MDX_OK;
}

extern "C" int mdx_get_params(const mdx_ctx* c, mdx_params* p)
{
    if (!c || !p) return MDX_EINVAL;
    *p = c->prm;
    return MDX_OK;
}

// The LK dataflow's fallbacks since the last check: a sync point queues the statistics word's
// readback on the context stream (every LK launch of a call is joined into it); after the sync
// lk_err_result adds them to the context's totals (mdx_lk_fallbacks) and clears the word.  A wait
// that gave up is not an error: its level was recomputed in sequence within the same call.
static int lk_err_result(mdx_ctx* c)
{
    const int groups = c->err_host[0], gates = c->err_host[1], redone = c->err_host[2];
    if (groups == 0 && gates == 0 && redone == 0) return MDX_OK;
    c->err_host[0] = c->err_host[1] = c->err_host[2] = 0;
    c->lk_fallback[0] += groups;
    c->lk_fallback[1] += gates;
    c->lk_fallback[2] += redone;
    HIP_OR_RETURN(c, hipMemsetAsync(c->errw.p, 0, 12, c->stream));
    HIP_OR_RETURN(c, hipStreamSynchronize(c->stream));
    // a give-up (a group wait or a gate) is always followed by its level's recompute (launch_lk_v2):
    // one without it would be a scheduling bug, and its outputs could be wrong
    if (groups + gates > 0 && redone == 0)
        return set_err(c, MDX_EHIP, "LK dataflow: %d wait(s) and %d gate(s) gave up but no level was recomputed",
                       groups, gates);
    return MDX_OK;
}

extern "C" int mdx_lk_fallbacks(const mdx_ctx* c, long long* counts)
{
    if (!c || !counts) return MDX_EINVAL;
    for (int i = 0; i < 3; i++) counts[i] = c->lk_fallback[i];
    return MDX_OK;
}

static int sync_point(mdx_ctx* c, bool whole_device)
{
    if (!c) return MDX_EINVAL;
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    HIP_OR_RETURN(c, hipMemcpyAsync(c->err_host, c->errw.p, 12, hipMemcpyDeviceToHost, c->stream));
    if (whole_device) HIP_OR_RETURN(c, hipDeviceSynchronize());
    else HIP_OR_RETURN(c, hipStreamSynchronize(c->stream));
    return lk_err_result(c);
}

extern "C" int mdx_sync(mdx_ctx* c) { return sync_point(c, false); }
extern "C" int mdx_device_sync(mdx_ctx* c) { return sync_point(c, true); }

extern "C" int mdx_input_ready(mdx_ctx* c, void* hip_event)
{
    if (!c) return MDX_EINVAL;
    c->input_ev = static_cast<hipEvent_t>(hip_event);
    return MDX_OK;
}

static constexpr int kSlots = 256;   // timed calls kept between mdx_enable_timing and readout

extern "C" int mdx_enable_timing(mdx_ctx* c, int on)
{
    if (!c) return MDX_EINVAL;
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    while (on && c->ev.size() < (size_t)kSlots * 7) {   // a retry after a failure goes on where it stopped
        hipEvent_t e = nullptr;
        if (!new_events(c, &e, 1, hipEventDefault))
            return set_err(c, MDX_EHIP, "hipEventCreate(&c->ev[i]) failed: %s", hipGetErrorString(hipGetLastError()));
        c->ev.push_back(e);
    }
    c->timing = on != 0;
    c->ncalls = 0;
    c->cur = -1;
    return MDX_OK;
}

extern "C" int mdx_timing_calls(const mdx_ctx* c) { return c ? c->ncalls : 0; }

// Sum over the recorded calls of the time between the stage's bracketing events.
extern "C" int mdx_stage_ms(mdx_ctx* c, int stage, float* ms)
{
    if (!c || !ms || stage < 0 || stage > 6) return MDX_EINVAL;
    if (!c->timing || c->ev.empty()) return set_err(c, MDX_EINVAL, "timing not enabled");
    if (c->ncalls > kSlots) return set_err(c, MDX_EINVAL, "more than %d timed calls", kSlots);
    float total = 0.f;
    for (int k = 0; k < c->ncalls; k++) {
        hipEvent_t* e = c->ev.data() + k * 7;
        HIP_OR_RETURN(c, hipEventSynchronize(e[6]));
        float t = 0.f;
        if (stage == 6) HIP_OR_RETURN(c, hipEventElapsedTime(&t, e[0], e[6]));
        else HIP_OR_RETURN(c, hipEventElapsedTime(&t, e[stage], e[stage + 1]));
        total += t;
    }
    *ms = total;
    return MDX_OK;
}

// Test hook: copy an internal LK v2 buffer to the host (0 = A sums, 1 = per-level trace, 6 = MDX_LK_DEBUG
// contexts only: the last call's k_lk_iter wave-iterations by row body, uint32 [kMaxLevels][2] =
// (exact, fused) per level; 7 = the last mdx_fit_subspace's centred data, [ntraj * 2 * traj_len] floats
// followed by the two means; 8 = its 50 per-hypothesis inlier counts, int32).
#if MDX_WARP_STAMP
namespace mdx { hipError_t debug_warp_stamps(void* dst, size_t bytes); }
#endif
extern "C" int mdx_debug_copy(mdx_ctx* c, int which, void* dst, size_t bytes)
{
    if (!c || !dst) return MDX_EINVAL;
#if MDX_WARP_STAMP
    if (which == 99) {   // diagnostic build: the warp's in-kernel clock stamps (scripts/warp_burst.py)
        HIP_OR_RETURN(c, hipDeviceSynchronize());
        HIP_OR_RETURN(c, debug_warp_stamps(dst, bytes));
        return MDX_OK;
    }
#endif
    DevBuf& b = which == 0 ? c->Abuf : which == 1 ? c->dbg : which == 2 ? c->pyr1 : which == 3 ? c->pyr2
              : which == 4 ? c->der : which == 6 ? c->lkcnt : which == 7 ? c->sdata : which == 8 ? c->scnt : c->cls;
    if (!b.p) return set_err(c, MDX_EINVAL, "debug buffer %d unavailable", which);
    HIP_OR_RETURN(c, hipStreamSynchronize(c->stream));
    // pyramids: the half the last pair call wrote
    const uint8_t* src = static_cast<const uint8_t*>(b.p);
    if (which == 2 && c->last_pyr1) src = c->last_pyr1;
    if (which == 3 && c->last_pyr2) src = c->last_pyr2;
    const size_t avail = b.cap - (size_t)(src - static_cast<const uint8_t*>(b.p));
    HIP_OR_RETURN(c, hipMemcpy(dst, src, bytes < avail ? bytes : avail, hipMemcpyDeviceToHost));
    return MDX_OK;
}

extern "C" int mdx_debug_div32(mdx_ctx* c, const double* d_in, double* d_out, int n)
{
    if (!c || !d_in || !d_out || n <= 0) return MDX_EINVAL;
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    HIP_OR_RETURN(c, launch_div32(c->stream, d_in, d_out, n));
    return MDX_OK;
}

extern "C" int mdx_debug_warp_paths(mdx_ctx* c, int32_t* out, int cap)
{
    if (!c || cap < 0 || (cap > 0 && !out)) return MDX_EINVAL;
    const WarpLaunch& L = c->last_warp;
    if (L.batch <= 0) return set_err(c, MDX_EINVAL, "mdx_debug_warp_paths: no warp launch on this context yet");
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    HIP_OR_RETURN(c, debug_warp_paths(c->stream, L, out, cap));
    return L.batch * L.ntiles;
}

extern "C" void* mdx_host_alloc(size_t bytes)
{
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(g_host_mu);
    g_host_blocks[reinterpret_cast<uintptr_t>(p)] = bytes ? bytes : 1;
    return p;
}

extern "C" int mdx_host_free(void* p)
{
    if (!p) return MDX_OK;
    {
        std::lock_guard<std::mutex> lk(g_host_mu);
        g_host_blocks.erase(reinterpret_cast<uintptr_t>(p));
    }
    return hipHostFree(p) == hipSuccess ? MDX_OK : MDX_EHIP;
}

extern "C" void* mdx_dev_alloc(mdx_ctx* c, size_t bytes)
{
    if (!c) return nullptr;
    (void)hipSetDevice(c->device);
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) {
        set_err(c, MDX_ENOMEM, "hipMalloc(%zu) failed", bytes);
        return nullptr;
    }
    return p;
}

extern "C" int mdx_dev_free(mdx_ctx* c, void* p)
{
    if (!c) return MDX_EINVAL;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    HIP_OR_RETURN(c, hipFree(p));
    return MDX_OK;
}

extern "C" int mdx_memcpy_h2d(mdx_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c) return MDX_EINVAL;
    HIP_OR_RETURN(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_OR_RETURN(c, hipStreamSynchronize(c->stream));
    return MDX_OK;
}

extern "C" int mdx_memcpy_d2h(mdx_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c) return MDX_EINVAL;
    HIP_OR_RETURN(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_OR_RETURN(c, hipStreamSynchronize(c->stream));
    return MDX_OK;
}

// Half-size ingest (include/mdx.h; the kernel is mdx_resize.hip's k_half).
extern "C" int mdx_half_size(int w, int h, int* dw, int* dh)
{
    if (w < 2 || h < 2 || !dw || !dh) return MDX_EINVAL;   // a side of 1 rounds to 0
    // cvRound(side * 0.5): an odd side 2k + 1 lies halfway between k and k + 1 and goes to the even one
    auto half = [](int v) { return v / 2 + ((v & 1) & (v / 2 & 1)); };
    *dw = half(w);
    *dh = half(h);
    return MDX_OK;
}

static int check_half(mdx_ctx* c, const char* who, int batch, const uint8_t* src, int w, int h, int stride,
                      size_t frame_stride, int channels, const uint8_t* dst, int dst_stride, size_t dst_frame_stride,
                      int* dw, int* dh)
{
    if (!src || !dst || batch < 1) return set_err(c, MDX_EINVAL, "%s: null pointer or batch < 1", who);
    if (channels != 1 && channels != 3) return set_err(c, MDX_EINVAL, "%s: channels %d, not 1 or 3", who, channels);
    if (mdx_half_size(w, h, dw, dh) != MDX_OK) return set_err(c, MDX_EINVAL, "%s: a side of %d x %d halves to 0", who, w, h);
    if (*dh > 65535 * kHalfRows) return set_err(c, MDX_EINVAL, "%s: more than %d rows", who, 2 * 65535 * kHalfRows);
    if ((long long)w * channels > INT32_MAX || stride < w * channels)
        return set_err(c, MDX_EINVAL, "%s: stride %d < w*channels", who, stride);
    if (frame_stride < (size_t)h * (size_t)stride) return set_err(c, MDX_EINVAL, "%s: frame_stride < h*stride", who);
    if (dst_stride < *dw * channels) return set_err(c, MDX_EINVAL, "%s: dst_stride %d < dw*channels %d", who, dst_stride, *dw * channels);
    if (dst_frame_stride < (size_t)*dh * (size_t)dst_stride)
        return set_err(c, MDX_EINVAL, "%s: dst_frame_stride < dh*dst_stride", who);
    // the bytes either side touches: whole frames but the last, whose last row ends with its pixels
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
    const uintptr_t s1 = s0 + (size_t)(batch - 1) * frame_stride + (size_t)(h - 1) * stride + (size_t)w * channels;
    const uintptr_t d1 = d0 + (size_t)(batch - 1) * dst_frame_stride + (size_t)(*dh - 1) * dst_stride + (size_t)*dw * channels;
    if (s0 < d1 && d0 < s1) return set_err(c, MDX_EINVAL, "%s: source and destination overlap", who);
    return MDX_OK;
}

extern "C" int mdx_resize_half_dev(mdx_ctx* c, int batch, const uint8_t* d_src, int w, int h, int stride,
                                   size_t frame_stride, int channels, uint8_t* d_dst, int dst_stride,
                                   size_t dst_frame_stride)
{
    if (!c) return MDX_EINVAL;
    int dw, dh;
    if (const int rc = check_half(c, "mdx_resize_half_dev", batch, d_src, w, h, stride, frame_stride, channels, d_dst,
                                  dst_stride, dst_frame_stride, &dw, &dh);
        rc != MDX_OK)
        return rc;
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (c->input_ev) {      // mdx_input_ready: one-shot
        hipEvent_t e = c->input_ev;
        c->input_ev = nullptr;
        HIP_OR_RETURN(c, hipStreamWaitEvent(s, e, 0));
    }
    HIP_OR_RETURN(c, launch_half(s, batch, d_src, w, h, stride, frame_stride, channels, d_dst, dst_stride, dst_frame_stride));
    return MDX_OK;
}

extern "C" int mdx_resize_half(mdx_ctx* c, const uint8_t* src, int w, int h, int stride, int channels, uint8_t* dst,
                               int dst_stride)
{
    if (!c) return MDX_EINVAL;
    int dw, dh;
    const size_t fs = (size_t)std::max(h, 0) * (size_t)std::max(stride, 0);
    // (host pointers: the overlap test compares what it is given; the device copies never overlap)
    if (const int rc = check_half(c, "mdx_resize_half", 1, src, w, h, stride, fs, channels, dst, dst_stride,
                                  (size_t)std::max(h, 0) * (size_t)std::max(dst_stride, 0), &dw, &dh);
        rc != MDX_OK)
        return rc;
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    const int dpitch = (dw * channels + 3) & ~3;
    if (const int rc = ensure_all(c, {{&c->hsrc, fs}, {&c->hdst, (size_t)dpitch * dh}}); rc != MDX_OK) return rc;
    hipStream_t s = c->stream;
    // the caller's last row holds w * channels bytes, not stride
    HIP_OR_RETURN(c, hipMemcpyAsync(c->hsrc.p, src, (size_t)(h - 1) * stride + (size_t)w * channels, hipMemcpyHostToDevice, s));
    HIP_OR_RETURN(c, launch_half(s, 1, c->hsrc.as<uint8_t>(), w, h, stride, 0, channels, c->hdst.as<uint8_t>(), dpitch, 0));
    HIP_OR_RETURN(c, hipMemcpy2DAsync(dst, (size_t)dst_stride, c->hdst.p, (size_t)dpitch, (size_t)dw * channels, (size_t)dh,
                                      hipMemcpyDeviceToHost, s));
    HIP_OR_RETURN(c, hipStreamSynchronize(s));
    return MDX_OK;
}
