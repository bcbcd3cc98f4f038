// mdx_traj.cpp -- trajectory tracking (calculateOpticalFlowTrajectory) on host frames and on the
// resident frame ring.
#include "mdx_ctx.h"

using namespace mdx;

// The trajectory passes of calculateOpticalFlowTrajectory (optical_flow_calculator.cpp:143-257) over
// nimg frames whose padded pyramids and Scharr planes are on the device already: pass j tracks the
// points the previous pass left from frame j (pyr[j], der[j]) to frame j + 1 (pyr[j + 1]).  Every
// pass runs the point LK from the carried points: for one pair it is faster than the class-plane
// kernels even on the grid start points of pass 0, whose per-level tails one pair cannot fill.
extern "C" size_t mdx_trajectory_layout(int npts, int nimg, size_t offsets[4])
{
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t p = (size_t)(npts > 0 ? npts : 1), n = (size_t)(nimg > 0 ? nimg : 1);
    size_t o[4];
    o[0] = 0;
    o[1] = al(p * n * 8);
    o[2] = o[1] + al(p * 8);
    o[3] = o[2] + al(p * 32);
    if (offsets)
        for (int i = 0; i < 4; i++) offsets[i] = o[i];
    return o[3] + p * 4;
}

static int trajectory_passes(mdx_ctx* c, const Geometry& g, int nimg, int w, int h, const uint8_t* const* pyr,
                             const uint32_t* const* der, float* traj, int32_t* traj_len, float* start_pts,
                             double* vectors, int* num_vectors)
{
    const mdx_params& P = c->prm;
    const LkArgs a = lk_args_for(c, g, w, h);
    const int npts = a.npts, ny = a.ny;
    const size_t pts = (size_t)(npts > 0 ? npts : 1);
    // the four outputs in one block, laid out as mdx_trajectory_layout says (one readback copy
    // when the host block matches)
    size_t off[4];
    const size_t obytes = mdx_trajectory_layout(npts, nimg, off);
    int rc = ensure_all(c, {{&c->tcur, pts * 8}, {&c->tnp, pts * 8}, {&c->tst, pts}, {&c->ttraj, obytes},
                            {&c->tnum, 8}});
    if (rc != MDX_OK) return rc;
    if (!c->tcnt_host && !(c->tcnt_host = pinned_ints(c, 4)))
        return set_err(c, MDX_ENOMEM, "trajectory passes: hipHostMalloc(counts)");
    hipStream_t s = c->stream;
    float* cur = c->tcur.as<float>();
    uint8_t* ob = c->ttraj.as<uint8_t>();
    float* tr = reinterpret_cast<float*>(ob + off[0]);
    float* tstart = reinterpret_cast<float*>(ob + off[1]);
    double* tvec = reinterpret_cast<double*>(ob + off[2]);
    int* tl = reinterpret_cast<int*>(ob + off[3]);
    int* dnum = c->tnum.as<int>();
    const bool chain = c->traj_chain && nimg <= kMaxTrajImgs && npts > 0;
    bool direct = false;   // the chained launch writes the caller's mapped outputs itself
    if (chain && (rc = ensure(c, c->tflag, pts * 4)) != MDX_OK) return rc;
    HIP_OR_RETURN(c, launch_traj_init(s, npts, ny, P.pixel_step, nimg, cur, tr, tl, dnum,
                                      chain ? c->tflag.as<int>() : nullptr));
    if (chain) {
        // every pass in one launch: pass j + 1 of a point starts as soon as its pass j is done, so
        // the passes' launch tails overlap (the per-pass launches below leave each tail idle)
        TrajChain t{};
        for (int j = 0; j < nimg; j++) {
            t.pyr[j] = pyr[j];
            t.der[j] = der[j];
        }
        t.nimg = nimg;
        t.w = w;
        t.h = h;
        t.cur = cur;
        t.traj = tr;
        t.tlen = tl;
        t.flag = c->tflag.as<int>();
        t.vectors = tvec;
        t.start_pts = tstart;
        // the caller's outputs in mapped page-locked memory (mdx_host_alloc): the launch writes them
        if (npts > 0 && traj && traj_len && start_pts && vectors) {
            // only whole ranges inside one mdx_host_alloc block qualify (a partly pinned or short
            // buffer takes the copy path, which reports its errors); pageable memory is never queried
            const size_t pn = (size_t)npts, nn = (size_t)nimg;
            auto mapped = [&](void* p, size_t bytes) -> void* {
                if (!host_block_holds(p, bytes)) return nullptr;
                hipPointerAttribute_t at{};
                if (hipPointerGetAttributes(&at, p) != hipSuccess) {
                    (void)hipGetLastError();
                    return nullptr;
                }
                return at.type == hipMemoryTypeHost ? at.devicePointer : nullptr;
            };
            void* m[4] = {mapped(traj, pn * nn * 8), mapped(traj_len, pn * 4), mapped(start_pts, pn * 8),
                          mapped(vectors, pn * 32)};
            if (m[0] && m[1] && m[2] && m[3]) {
                t.htraj = static_cast<float*>(m[0]);
                t.htlen = static_cast<int*>(m[1]);
                t.hstart = static_cast<float*>(m[2]);
                t.hvec = static_cast<double*>(m[3]);
                direct = true;
            }
        }
        t.num = dnum;
        t.mvs = P.min_vector_size;
        HIP_OR_RETURN(c, launch_lk_chain(s, a, t, c->traj_ppw));
    }
    for (int j = 0; !chain && j + 1 < nimg && npts > 0; j++) {
        LkArgs b = a;
        b.pyr1 = pyr[j];
        b.pyr2 = pyr[j + 1];
        b.der = der[j];
        b.next_pts = c->tnp.as<float>();
        b.status = c->tst.as<uint8_t>();
        b.prev_pts = cur;
        if ((rc = run_lk(c, g, b, 1, w, h, 0, ny, true)) != MDX_OK) return rc;
        HIP_OR_RETURN(c, launch_traj_update(s, npts, c->tnp.as<float>(), c->tst.as<uint8_t>(), cur, tr, tl, nimg, w, h,
                                            j == nimg - 2, P.min_vector_size, tvec, tstart, dnum));
    }
    int num = 0;
    if (npts > 0 && !direct) {
        uint8_t* hb = reinterpret_cast<uint8_t*>(traj);
        const bool one_block = traj && start_pts && vectors && traj_len &&
                               reinterpret_cast<uint8_t*>(start_pts) == hb + off[1] &&
                               reinterpret_cast<uint8_t*>(vectors) == hb + off[2] &&
                               reinterpret_cast<uint8_t*>(traj_len) == hb + off[3];
        if (one_block) {
            HIP_OR_RETURN(c, hipMemcpyAsync(hb, ob, off[3] + (size_t)npts * 4, hipMemcpyDeviceToHost, s));
        } else {
            if (traj) HIP_OR_RETURN(c, hipMemcpyAsync(traj, tr, (size_t)npts * nimg * 8, hipMemcpyDeviceToHost, s));
            if (traj_len) HIP_OR_RETURN(c, hipMemcpyAsync(traj_len, tl, (size_t)npts * 4, hipMemcpyDeviceToHost, s));
            if (start_pts) HIP_OR_RETURN(c, hipMemcpyAsync(start_pts, tstart, (size_t)npts * 8, hipMemcpyDeviceToHost, s));
            if (vectors) HIP_OR_RETURN(c, hipMemcpyAsync(vectors, tvec, (size_t)npts * 32, hipMemcpyDeviceToHost, s));
        }
    }
    c->tcnt_host[0] = c->tcnt_host[1] = 0;
    HIP_OR_RETURN(c, hipMemcpyAsync(c->tcnt_host, dnum, chain ? 8 : 4, hipMemcpyDeviceToHost, s));
    HIP_OR_RETURN(c, hipStreamSynchronize(s));
    num = c->tcnt_host[0];
    if (chain && c->tcnt_host[1] != 0)
        return set_err(c, MDX_EHIP, "trajectory passes: %d point hand-off(s) timed out", c->tcnt_host[1]);
    if (num_vectors) *num_vectors = num;
    return MDX_OK;
}

// calculateOpticalFlowTrajectory (optical_flow_calculator.cpp:133-257) on host frames.  Pair slot j
// holds frames (j, j+1): the gray / pyramid / Scharr stages run batched over all slots in one
// launch each (the reference rebuilds each frame's pyramid twice, :166-170; these are the same
// images), then the nimg-1 LK passes run in order on the points the previous pass left.
extern "C" int mdx_flow_trajectory(mdx_ctx* c, const uint8_t* const* imgs, int nimg, int w, int h, int stride,
                                   int fmt, float* traj, int32_t* traj_len, float* start_pts, double* vectors,
                                   int* num_vectors)
{
    if (!c) return MDX_EINVAL;
    if (!imgs || nimg < 2) return set_err(c, MDX_EINVAL, "mdx_flow_trajectory: need >= 2 frames");
    for (int i = 0; i < nimg; i++)
        if (!imgs[i]) return set_err(c, MDX_EINVAL, "mdx_flow_trajectory: null frame %d", i);
    int rc = check_frame(c, "mdx_flow_trajectory", w, h, stride, fmt);
    if (rc != MDX_OK) return rc;
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    const int npairs = nimg - 1;
    const Geometry g = make_geometry(w, h, c->prm.max_level);
    if ((rc = ensure_workspace(c, g, npairs, false)) != MDX_OK) return rc;
    c->band_w = c->band_h = 0;   // the slabs are rebuilt: a pending band fit/warp has nothing to read
    const size_t fbytes = (size_t)stride * h;                        // device slot
    const size_t copy_bytes = frame_copy_bytes(w, h, stride, fmt);   // what each caller's frame holds
    if ((rc = ensure(c, c->tin, fbytes * nimg)) != MDX_OK) return rc;
    hipStream_t s = c->stream;
    uint8_t* din = c->tin.as<uint8_t>();
    for (int i = 0; i < nimg; i++)
        HIP_OR_RETURN(c, hipMemcpyAsync(din + fbytes * i, imgs[i], copy_bytes, hipMemcpyHostToDevice, s));
    uint8_t* pyr1 = c->pyr1.as<uint8_t>();
    uint8_t* pyr2 = c->pyr2.as<uint8_t>();
    uint32_t* der = c->der.as<uint32_t>();
    HIP_OR_RETURN(c, launch_front(s, npairs, din, din + fbytes, w, h, stride, (long long)fbytes, fmt, pyr1, pyr2, g));
    HIP_OR_RETURN(c, launch_pyr_levels(s, npairs, pyr1, pyr2, g));
    HIP_OR_RETURN(c, launch_scharr_levels(s, npairs, pyr1, der, g));
    // frame j's pyramid is slot j of pyr1 (j < nimg-1) and the last frame's slot nimg-2 of pyr2
    std::vector<const uint8_t*> fp(nimg);
    std::vector<const uint32_t*> fd(nimg);
    for (int j = 0; j < npairs; j++) {
        fp[j] = pyr1 + (size_t)g.img_bytes * j;
        fd[j] = der + (size_t)g.der_words * j;
    }
    fp[npairs] = pyr2 + (size_t)g.img_bytes * (npairs - 1);
    fd[npairs] = nullptr;
    rc = trajectory_passes(c, g, nimg, w, h, fp.data(), fd.data(), traj, traj_len, start_pts, vectors, num_vectors);
    release_pyr_all(c);
    return rc;
}

// The resident ring (include/mdx.h): slot k of ring_pyr / ring_der holds one frame's padded pyramid
// and Scharr planes; ring_order lists the held slots oldest first.
static int ring_grow(mdx_ctx* c, const Geometry& g, int cap)
{
    if (cap <= c->ring_cap) return MDX_OK;
    DevBuf np, nd;   // freed again on any failure exit
    auto fail = [&](const char* what) { return set_err(c, MDX_ENOMEM, "mdx_ring_push: %s", what); };
    if (!np.alloc((size_t)g.img_bytes * cap + slab_slack_bytes(g))) return fail("hipMalloc(pyramids)");
    if (!nd.alloc((size_t)g.der_words * 4 * cap)) return fail("hipMalloc(derivatives)");
    // the held frames move to slots 0 .. n-1, in order; the context's state changes only once
    // every copy has landed (a failed copy leaves the old ring intact and frees the new buffers)
    std::vector<int> order(c->ring_order.size());
    for (size_t k = 0; k < c->ring_order.size(); k++) {
        const int o = c->ring_order[k];
        if (hipMemcpyAsync(np.as<uint8_t>() + (size_t)g.img_bytes * k, c->ring_pyr.as<uint8_t>() + (size_t)g.img_bytes * o,
                           g.img_bytes, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(nd.as<uint8_t>() + (size_t)g.der_words * 4 * k,
                           c->ring_der.as<uint8_t>() + (size_t)g.der_words * 4 * o, (size_t)g.der_words * 4,
                           hipMemcpyDeviceToDevice, c->stream) != hipSuccess) {
            (void)hipStreamSynchronize(c->stream);
            return fail("slot copy failed");
        }
        order[k] = (int)k;
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail("slot copy failed");
    c->ring_order = order;
    c->ring_pyr = std::move(np);
    c->ring_der = std::move(nd);
    c->ring_cap = cap;
    return MDX_OK;
}

extern "C" int mdx_ring_reset(mdx_ctx* c)
{
    if (!c) return MDX_EINVAL;
    c->ring_order.clear();
    return MDX_OK;
}

// mdx_ring_push and mdx_ring_push_half: the frame (halved first when `half`) enters a free slot as its
// padded pyramid and Scharr planes.  The ring's geometry is the size the frame has after the halving.
static int ring_push(mdx_ctx* c, const char* who, const uint8_t* img, int w, int h, int stride, int fmt, int keep,
                     bool half)
{
    if (!c) return MDX_EINVAL;
    if (!img) return set_err(c, MDX_EINVAL, "%s: null frame", who);
    if (keep < 1) return set_err(c, MDX_EINVAL, "%s: keep must be >= 1", who);
    int rc = check_frame(c, who, w, h, stride, fmt);
    if (rc != MDX_OK) return rc;
    const int cn = fmt == MDX_FMT_GRAY8 ? 1 : 3;
    int rw = w, rh = h, rstride = stride;          // the frame the pyramid is built from
    if (half) {
        if (mdx_half_size(w, h, &rw, &rh) != MDX_OK) return set_err(c, MDX_EINVAL, "%s: a side of %d x %d halves to 0", who, w, h);
        rstride = (rw * cn + 3) & ~3;              // k_half's vector path, whenever the caller's pitch allows it
    }
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    if (rw != c->ring_w || rh != c->ring_h || c->prm.max_level != c->ring_ml) {   // another geometry: start over
        c->ring_order.clear();
        if (c->ring_pyr.p) (void)hipStreamSynchronize(c->stream);
        c->ring_pyr.reset();
        c->ring_der.reset();
        c->ring_cap = 0;
        c->ring_w = rw;
        c->ring_h = rh;
        c->ring_ml = c->prm.max_level;
    }
    const Geometry g = make_geometry(rw, rh, c->prm.max_level);
    const int n = (int)c->ring_order.size();
    if ((rc = ring_grow(c, g, std::max(n + 1, std::max(keep, 4)))) != MDX_OK) return rc;
    // a free slot: the lowest one no held frame uses
    std::vector<char> used(c->ring_cap, 0);
    for (int o : c->ring_order) used[o] = 1;
    int slot = 0;
    while (used[slot]) slot++;
    const size_t fbytes = (size_t)rstride * rh;
    // the upload lands in rfull when it is halved into rin, else in rin itself
    DevBuf& up = half ? c->rfull : c->rin;
    if ((rc = ensure_all(c, {{&up, (size_t)stride * h}, {&c->rin, fbytes}})) != MDX_OK) return rc;
    hipStream_t s = c->stream;
    HIP_OR_RETURN(c, hipMemcpyAsync(up.p, img, frame_copy_bytes(w, h, stride, fmt), hipMemcpyHostToDevice, s));
    if (half)
        HIP_OR_RETURN(c, launch_half(s, 1, up.as<uint8_t>(), w, h, stride, 0, cn, c->rin.as<uint8_t>(), rstride, 0));
    uint8_t* pyr = c->ring_pyr.as<uint8_t>() + (size_t)g.img_bytes * slot;
    uint32_t* der = c->ring_der.as<uint32_t>() + (size_t)g.der_words * slot;
    HIP_OR_RETURN(c, launch_front(s, 1, c->rin.as<uint8_t>(), c->rin.as<uint8_t>(), rw, rh, rstride, (long long)fbytes, fmt,
                                  pyr, pyr, g, 1));
    HIP_OR_RETURN(c, launch_pyr_levels(s, 1, pyr, pyr, g, 1));
    HIP_OR_RETURN(c, launch_scharr_levels(s, 1, pyr, der, g));
    c->ring_order.push_back(slot);
    while ((int)c->ring_order.size() > keep) c->ring_order.erase(c->ring_order.begin());
    return (int)c->ring_order.size();
}

extern "C" int mdx_ring_push(mdx_ctx* c, const uint8_t* img, int w, int h, int stride, int fmt, int keep)
{
    return ring_push(c, "mdx_ring_push", img, w, h, stride, fmt, keep, false);
}

extern "C" int mdx_ring_push_half(mdx_ctx* c, const uint8_t* img, int w, int h, int stride, int fmt, int keep)
{
    return ring_push(c, "mdx_ring_push_half", img, w, h, stride, fmt, keep, true);
}

extern "C" int mdx_ring_trajectory(mdx_ctx* c, float* traj, int32_t* traj_len, float* start_pts, double* vectors,
                                   int* num_vectors)
{
    if (!c) return MDX_EINVAL;
    const int nimg = (int)c->ring_order.size();
    if (nimg < 2) return set_err(c, MDX_EINVAL, "mdx_ring_trajectory: the ring holds %d frame(s), need >= 2", nimg);
    if (c->prm.max_level != c->ring_ml)
        return set_err(c, MDX_EINVAL, "mdx_ring_trajectory: max_level changed since the frames were pushed");
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    const Geometry g = make_geometry(c->ring_w, c->ring_h, c->prm.max_level);
    std::vector<const uint8_t*> fp(nimg);
    std::vector<const uint32_t*> fd(nimg);
    for (int j = 0; j < nimg; j++) {
        fp[j] = c->ring_pyr.as<uint8_t>() + (size_t)g.img_bytes * c->ring_order[j];
        fd[j] = c->ring_der.as<uint32_t>() + (size_t)g.der_words * c->ring_order[j];
    }
    return trajectory_passes(c, g, nimg, c->ring_w, c->ring_h, fp.data(), fd.data(), traj, traj_len, start_pts, vectors,
                             num_vectors);
}
