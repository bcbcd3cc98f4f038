// mdx_bg_api.cpp -- the host side of background subtraction (include/mdx.h mdx_bg_*): the model
// as an owned resource of its context, the per-frame learning rate, the launches of mdx_bg.hip, and the
// translation between the device's plane layout and the canonical host layout of get_state / set_state.
#include "mdx_ctx.h"

#include <cmath>
#include <cstring>

using namespace mdx;

extern "C" void mdx_bg_default_params(mdx_bg_params* p)
{
    if (!p) return;
    *p = mdx_bg_params{500, 5, 16.f, 9.f, 0.9f, 15.f, 4.f, 75.f, 0.05f, 1, 127, 0.5f};
}

extern "C" size_t mdx_bg_params_size(void) { return sizeof(mdx_bg_params); }

static const char* check_bg_params(const mdx_bg_params& p)
{
    if (p.nmixtures < 1 || p.nmixtures > MDX_BG_MAX_MIXTURES) return "nmixtures outside [1, 8]";
    if (p.history < 1) return "history < 1";
    for (float v : {p.var_threshold, p.var_threshold_gen, p.var_init, p.var_min, p.var_max, p.ct})
        if (!std::isfinite(v) || v < 0.f) return "a threshold, variance or ct is negative or not finite";
    if (p.var_min > p.var_max) return "var_min > var_max";
    if (!(p.background_ratio > 0.f && p.background_ratio <= 1.f)) return "background_ratio outside (0, 1]";
    if (!(p.tau >= 0.f && p.tau <= 1.f)) return "tau outside [0, 1]";
    if (p.shadow_value < 0 || p.shadow_value > 255) return "shadow_value outside [0, 255]";
    return nullptr;
}

// bg is a live model of c (bg is not dereferenced unless it is)
static bool owns(const mdx_ctx* c, const mdx_bg* bg)
{
    for (const auto& b : c->bgs)
        if (b.get() == bg) return true;
    return false;
}

static int check_model(mdx_ctx* c, const char* who, const mdx_bg* bg)
{
    if (!bg) return set_err(c, MDX_EINVAL, "%s: null model", who);
    if (!owns(c, bg)) return set_err(c, MDX_EINVAL, "%s: not a model of this context", who);
    return MDX_OK;
}

static BgModel dev_model(const mdx_bg* bg)
{
    return BgModel{bg->state.as<float>(), bg->modes.as<uint8_t>(), bg->streams, bg->w, bg->h, bg->channels, bg->prm};
}

extern "C" int mdx_bg_create(mdx_ctx* c, int streams, int w, int h, int channels, const mdx_bg_params* params, mdx_bg** out)
{
    if (!c) return MDX_EINVAL;
    const char* who = "mdx_bg_create";
    if (!out) return set_err(c, MDX_EINVAL, "%s: out is NULL", who);
    if (streams < 1 || streams > kBgMaxStreams || w < 1 || h < 1) return set_err(c, MDX_EINVAL, "%s: bad streams or size", who);
    if (channels != 1 && channels != 3) return set_err(c, MDX_EINVAL, "%s: channels %d, not 1 or 3", who, channels);
    mdx_bg_params p;
    mdx_bg_default_params(&p);
    if (params) p = *params;
    if (const char* why = check_bg_params(p)) return set_err(c, MDX_EINVAL, "%s: %s", who, why);
    const size_t N = (size_t)w * h;
    if (N > (size_t)1 << 31) return set_err(c, MDX_EINVAL, "%s: more than 2^31 pixels", who);
    // streams * N * nmixtures * (2 + channels) * 4 bytes, without overflow: N <= 2^31, the rest < 2^16 * 40 * 4
    const size_t per_px = (size_t)p.nmixtures * (2 + channels) * 4;
    if ((size_t)streams * per_px > ((size_t)1 << 62) / N) return set_err(c, MDX_ENOMEM, "%s: the state does not fit", who);
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    auto bg = std::make_unique<mdx_bg>();
    bg->owner = c, bg->streams = streams, bg->w = w, bg->h = h, bg->channels = channels, bg->prm = p;
    if (!bg->state.alloc((size_t)streams * N * per_px) || !bg->modes.alloc((size_t)streams * N))
        return set_err(c, MDX_ENOMEM, "%s: hipMalloc of %zu B of state failed", who, (size_t)streams * N * (per_px + 1));
    HIP_OR_RETURN(c, hipMemsetAsync(bg->modes.p, 0, (size_t)streams * N, c->stream));
    *out = bg.get();
    c->bgs.push_back(std::move(bg));
    return MDX_OK;
}

extern "C" int mdx_bg_destroy(mdx_ctx* c, mdx_bg* bg)
{
    if (!c) return MDX_EINVAL;
    if (const int rc = check_model(c, "mdx_bg_destroy", bg); rc != MDX_OK) return rc;
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    HIP_OR_RETURN(c, hipStreamSynchronize(c->stream));   // its launches may still run
    for (auto it = c->bgs.begin(); it != c->bgs.end(); ++it)
        if (it->get() == bg) {
            c->bgs.erase(it);
            break;
        }
    return MDX_OK;
}

extern "C" int mdx_bg_reset(mdx_ctx* c, mdx_bg* bg)
{
    if (!c) return MDX_EINVAL;
    if (const int rc = check_model(c, "mdx_bg_reset", bg); rc != MDX_OK) return rc;
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    HIP_OR_RETURN(c, hipMemsetAsync(bg->modes.p, 0, (size_t)bg->streams * bg->w * bg->h, c->stream));
    bg->nframes = 0;
    return MDX_OK;
}

extern "C" int mdx_bg_frames(mdx_ctx* c, mdx_bg* bg)
{
    if (!c) return MDX_EINVAL;
    if (const int rc = check_model(c, "mdx_bg_frames", bg); rc != MDX_OK) return rc;
    return bg->nframes;
}

// the learning rate of the call that makes the model's frame count `nframes`
static float bg_alpha(const mdx_bg_params& p, int nframes, double learning_rate)
{
    if (learning_rate >= 0 && nframes > 1) return (float)learning_rate;
    return (float)(1.0 / std::min(2 * (long long)nframes, (long long)p.history));
}

extern "C" int mdx_bg_apply_dev(mdx_ctx* c, mdx_bg* bg, int T, const uint8_t* d_frames, int stride, size_t frame_stride,
                                size_t stream_stride, double learning_rate, uint8_t* d_fgmask)
{
    if (!c) return MDX_EINVAL;
    const char* who = "mdx_bg_apply_dev";
    if (const int rc = check_model(c, who, bg); rc != MDX_OK) return rc;
    if (T < 1) return set_err(c, MDX_EINVAL, "%s: T < 1", who);
    if (!d_frames) return set_err(c, MDX_EINVAL, "%s: d_frames is NULL", who);
    if (!std::isfinite(learning_rate)) return set_err(c, MDX_EINVAL, "%s: learning_rate is not finite", who);
    const long long row = (long long)bg->w * bg->channels;
    if (stride < row) return set_err(c, MDX_EINVAL, "%s: stride %d < w*channels %lld", who, stride, row);
    const size_t fbytes = (size_t)(bg->h - 1) * stride + (size_t)row;
    if (T > 1 && frame_stride < fbytes) return set_err(c, MDX_EINVAL, "%s: frames overlap (frame_stride %zu)", who, frame_stride);
    if (bg->streams > 1 && (frame_stride > (SIZE_MAX - fbytes) / (size_t)T ||
                            stream_stride < (size_t)(T - 1) * frame_stride + fbytes))
        return set_err(c, MDX_EINVAL, "%s: streams overlap (stream_stride %zu)", who, stream_stride);
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    HIP_OR_RETURN(c, wait_input_ready(c, s));
    const size_t N = (size_t)bg->w * bg->h;
    const BgModel M = dev_model(bg);
    for (int t0 = 0; t0 < T; t0 += kBgMaxFrames) {
        const int nt = std::min(kBgMaxFrames, T - t0);
        float alpha[kBgMaxFrames];
        for (int t = 0; t < nt; t++) alpha[t] = bg_alpha(bg->prm, bg->nframes + 1 + t, learning_rate);
        HIP_OR_RETURN(c, launch_bg_apply(s, M, nt, d_frames + (size_t)t0 * frame_stride, stride, frame_stride, stream_stride,
                                         alpha, d_fgmask ? d_fgmask + (size_t)t0 * N : nullptr, (size_t)T * N));
        bg->nframes += nt;
    }
    return MDX_OK;
}

extern "C" int mdx_bg_image_dev(mdx_ctx* c, mdx_bg* bg, uint8_t* d_out)
{
    if (!c) return MDX_EINVAL;
    const char* who = "mdx_bg_image_dev";
    if (const int rc = check_model(c, who, bg); rc != MDX_OK) return rc;
    if (!d_out) return set_err(c, MDX_EINVAL, "%s: d_out is NULL", who);
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    HIP_OR_RETURN(c, wait_input_ready(c, c->stream));
    HIP_OR_RETURN(c, launch_bg_image(c->stream, dev_model(bg), d_out));
    return MDX_OK;
}

extern "C" int mdx_bg_apply(mdx_ctx* c, mdx_bg* bg, const uint8_t* frame, int stride, double learning_rate, uint8_t* fgmask)
{
    if (!c) return MDX_EINVAL;
    const char* who = "mdx_bg_apply";
    if (const int rc = check_model(c, who, bg); rc != MDX_OK) return rc;
    if (bg->streams != 1) return set_err(c, MDX_EINVAL, "%s: a model of %d streams", who, bg->streams);
    if (!frame) return set_err(c, MDX_EINVAL, "%s: frame is NULL", who);
    if (!std::isfinite(learning_rate)) return set_err(c, MDX_EINVAL, "%s: learning_rate is not finite", who);
    const long long row = (long long)bg->w * bg->channels;
    if (stride < row) return set_err(c, MDX_EINVAL, "%s: stride %d < w*channels %lld", who, stride, row);
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    const size_t N = (size_t)bg->w * bg->h, fbytes = (size_t)(bg->h - 1) * stride + (size_t)row;   // the caller's last row ends there
    if (const int rc = ensure_all(c, {{&bg->hin, fbytes}, {&bg->hout, N * bg->channels}}); rc != MDX_OK) return rc;
    HIP_OR_RETURN(c, hipMemcpyAsync(bg->hin.p, frame, fbytes, hipMemcpyHostToDevice, c->stream));
    if (const int rc = mdx_bg_apply_dev(c, bg, 1, bg->hin.as<uint8_t>(), stride, fbytes, 0, learning_rate,
                                        fgmask ? bg->hout.as<uint8_t>() : nullptr);
        rc != MDX_OK)
        return rc;
    if (fgmask) HIP_OR_RETURN(c, hipMemcpyAsync(fgmask, bg->hout.p, N, hipMemcpyDeviceToHost, c->stream));
    HIP_OR_RETURN(c, hipStreamSynchronize(c->stream));
    return MDX_OK;
}

extern "C" int mdx_bg_image(mdx_ctx* c, mdx_bg* bg, uint8_t* out)
{
    if (!c) return MDX_EINVAL;
    const char* who = "mdx_bg_image";
    if (const int rc = check_model(c, who, bg); rc != MDX_OK) return rc;
    if (bg->streams != 1) return set_err(c, MDX_EINVAL, "%s: a model of %d streams", who, bg->streams);
    if (!out) return set_err(c, MDX_EINVAL, "%s: out is NULL", who);
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)bg->w * bg->h * bg->channels;
    if (const int rc = ensure(c, bg->hout, bytes); rc != MDX_OK) return rc;
    if (const int rc = mdx_bg_image_dev(c, bg, bg->hout.as<uint8_t>()); rc != MDX_OK) return rc;
    HIP_OR_RETURN(c, hipMemcpyAsync(out, bg->hout.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_OR_RETURN(c, hipStreamSynchronize(c->stream));
    return MDX_OK;
}

static int check_stream(mdx_ctx* c, const char* who, const mdx_bg* bg, int stream)
{
    if (stream < 0 || stream >= bg->streams) return set_err(c, MDX_EINVAL, "%s: stream %d of %d", who, stream, bg->streams);
    return MDX_OK;
}

extern "C" int mdx_bg_get_state(mdx_ctx* c, mdx_bg* bg, int stream, float* weight, float* variance, float* mean,
                                uint8_t* modes, int* nframes)
{
    if (!c) return MDX_EINVAL;
    const char* who = "mdx_bg_get_state";
    if (const int rc = check_model(c, who, bg); rc != MDX_OK) return rc;
    if (const int rc = check_stream(c, who, bg, stream); rc != MDX_OK) return rc;
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    const int nm = bg->prm.nmixtures, cn = bg->channels;
    const size_t N = (size_t)bg->w * bg->h, fl = bg_state_floats(bg->w, bg->h, cn, nm);
    std::vector<uint8_t> md(N);
    bg->xfer.resize(fl);
    float* st = bg->xfer.data();
    HIP_OR_RETURN(c, hipMemcpyAsync(st, bg->state.as<float>() + (size_t)stream * fl, fl * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_OR_RETURN(c, hipMemcpyAsync(md.data(), bg->modes.as<uint8_t>() + (size_t)stream * N, N, hipMemcpyDeviceToHost, c->stream));
    HIP_OR_RETURN(c, hipStreamSynchronize(c->stream));
    for (size_t p = 0; p < N; p++)
        for (int m = 0; m < nm; m++) {
            const bool live = m < md[p];   // the planes hold nothing meaningful at or above the count
            if (weight) weight[p * nm + m] = live ? st[(size_t)m * N + p] : 0.f;
            if (variance) variance[p * nm + m] = live ? st[(size_t)(nm + m) * N + p] : 0.f;
            if (mean)
                for (int k = 0; k < cn; k++)
                    mean[(p * nm + m) * cn + k] = live ? st[(size_t)(2 * nm + m * cn + k) * N + p] : 0.f;
        }
    if (modes) memcpy(modes, md.data(), N);
    if (nframes) *nframes = bg->nframes;
    return MDX_OK;
}

extern "C" int mdx_bg_set_state(mdx_ctx* c, mdx_bg* bg, int stream, const float* weight, const float* variance,
                                const float* mean, const uint8_t* modes, int nframes)
{
    if (!c) return MDX_EINVAL;
    const char* who = "mdx_bg_set_state";
    if (const int rc = check_model(c, who, bg); rc != MDX_OK) return rc;
    if (const int rc = check_stream(c, who, bg, stream); rc != MDX_OK) return rc;
    if (!weight || !variance || !mean || !modes) return set_err(c, MDX_EINVAL, "%s: a needed pointer is NULL", who);
    if (nframes < 0) return set_err(c, MDX_EINVAL, "%s: negative nframes", who);
    const int nm = bg->prm.nmixtures, cn = bg->channels;
    const size_t N = (size_t)bg->w * bg->h, fl = bg_state_floats(bg->w, bg->h, cn, nm);
    for (size_t p = 0; p < N; p++)
        if (modes[p] > nm) return set_err(c, MDX_EINVAL, "%s: pixel %zu has %d modes of %d", who, p, modes[p], nm);
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    bg->xfer.resize(fl);
    float* st = bg->xfer.data();
    auto canon = [](float v) {   // a NaN as the kernel stores one: 0x7fc00000
        const uint32_t q = 0x7fc00000u;
        if (std::isnan(v)) memcpy(&v, &q, 4);
        return v;
    };
    for (size_t p = 0; p < N; p++)
        for (int m = 0; m < nm; m++) {
            const bool live = m < modes[p];
            st[(size_t)m * N + p] = live ? canon(weight[p * nm + m]) : 0.f;
            st[(size_t)(nm + m) * N + p] = live ? canon(variance[p * nm + m]) : 0.f;
            for (int k = 0; k < cn; k++)
                st[(size_t)(2 * nm + m * cn + k) * N + p] = live ? canon(mean[(p * nm + m) * cn + k]) : 0.f;
        }
    HIP_OR_RETURN(c, hipMemcpyAsync(bg->state.as<float>() + (size_t)stream * fl, st, fl * 4, hipMemcpyHostToDevice, c->stream));
    HIP_OR_RETURN(c, hipMemcpyAsync(bg->modes.as<uint8_t>() + (size_t)stream * N, modes, N, hipMemcpyHostToDevice, c->stream));
    HIP_OR_RETURN(c, hipStreamSynchronize(c->stream));
    bg->nframes = nframes;
    return MDX_OK;
}
