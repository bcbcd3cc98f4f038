// mdx_bg.hip -- background subtraction by a per-pixel Gaussian mixture: the head of the
// reference's BackgroundSubtractor::getMotionContours (common/src/background_subtractor.cpp:27-28),
// cv::BackgroundSubtractorMOG2::operator() and getBackgroundImage as OpenCV 2.4's bgfg_gaussmix2.cpp computes
// them (MOG2Invoker, detectShadowGMM).  Restated from the published source; unpinned against a real build (no
// OpenCV here).  include/mdx.h states the arithmetic rule by rule; this file follows it literally, quirks
// included: IEEE binary32, no contraction, operations in the order written, correctly rounded division.
//
//   k_bg_apply   one lane owns one pixel of one stream.  It loads the pixel's mixture once -- only the modes
//                below its `modes` count -- carries it in registers through the launch's T frames (T <=
//                kBgMaxFrames, alphaT of each frame in the kernel arguments), writes one mask byte per frame,
//                and stores the mixture once: every weight below the new count, but mean and variance only of
//                the slots whose content changed (a fit, a swap, a new mode).  A slot the frames only
//                reweighted costs 4 B of store, not 4 * (2 + channels).
//   k_bg_image   the background image: the weighted mean of the leading modes up to background_ratio.
//
// State layout (private to this file and bg_state_index): per stream, one plane of w * h floats per (mode,
// field) -- nmixtures weight planes, nmixtures variance planes, nmixtures * channels mean planes -- and, apart,
// one `modes` byte per pixel.  Lane i of a wave holds pixel p0 + i, so every load and store of a wave is one
// contiguous run of 256 B (floats) or 64 B (mask, modes); the frame bytes are read as bytes at any pitch, so
// there is one path for every width and alignment.  The mode loops and both bubble-ups are unrolled to
// NM = nmixtures with compile-time indices: the mixture lives in VGPRs, never in scratch.
// A NaN (learning_rate 1 makes them: a renormalisation by 1 / 0) is stored as 0x7fc00000: IEEE leaves the
// sign and payload of a generated NaN open, and hosts differ in it.
// No lane touches memory of a pixel index >= w * h, and none reads or writes a mode >= its count.
#include "mdx_internal.h"

#include <type_traits>

namespace mdx {

namespace {

template <int CN, int NM> struct Mixture {
    float wt[NM], vr[NM], mu[NM][CN];
    int modes;
    uint32_t dirty;   // bit m: slot m's mean and variance differ from memory
};

template <int CN, int NM> __device__ __forceinline__ void swap_modes(Mixture<CN, NM>& g, int i)   // i and i - 1
{
    float t = g.wt[i];
    g.wt[i] = g.wt[i - 1], g.wt[i - 1] = t;
    t = g.vr[i];
    g.vr[i] = g.vr[i - 1], g.vr[i - 1] = t;
#pragma unroll
    for (int c = 0; c < CN; c++) {
        t = g.mu[i][c];
        g.mu[i][c] = g.mu[i - 1][c], g.mu[i - 1][c] = t;
    }
    g.dirty |= 3u << (i - 1);
}

// detectShadowGMM on the updated mixture
template <int CN, int NM> __device__ __forceinline__ bool bg_shadow(const Mixture<CN, NM>& g, const float (&data)[CN],
                                                                    const mdx_bg_params& P)
{
    bool res = false, done = false;
    float tw = 0.f;
#pragma unroll
    for (int m = 0; m < NM; m++) {
        if (m < g.modes && !done) {
            float num = 0.f, den = 0.f;
#pragma unroll
            for (int c = 0; c < CN; c++) {
                num += data[c] * g.mu[m][c];
                den += g.mu[m][c] * g.mu[m][c];
            }
            if (den == 0.f) {
                done = true;
            } else {
                if (num <= den && num >= P.tau * den) {
                    const float a = num / den;
                    float s = 0.f;
#pragma unroll
                    for (int c = 0; c < CN; c++) {
                        const float e = a * g.mu[m][c] - data[c];
                        s += e * e;
                    }
                    if (s < P.var_threshold * g.vr[m] * a * a) res = true, done = true;
                }
                if (!done) {
                    tw += g.wt[m];
                    if (tw > P.background_ratio) done = true;
                }
            }
        }
    }
    return res;
}

// MOG2Invoker for one pixel and one frame; returns the mask byte
template <int CN, int NM> __device__ __forceinline__ uint8_t bg_update(Mixture<CN, NM>& g, const float (&data)[CN],
                                                                       float alphaT, const mdx_bg_params& P)
{
    const float alpha1 = 1.f - alphaT, prune = -alphaT * P.ct;
    int n = g.modes;
    const int n0 = n;
    bool fits = false, background = false;
    float total = 0.f;
#pragma unroll
    for (int m = 0; m < NM; m++) {
        if (m < n) {   // n may have shrunk
            float w = alpha1 * g.wt[m] + prune;
            int swaps = 0;
            if (!fits) {
                const float var = g.vr[m];
                float d[CN], dist2 = 0.f;
#pragma unroll
                for (int c = 0; c < CN; c++) {
                    d[c] = g.mu[m][c] - data[c];
                    dist2 = c ? dist2 + d[c] * d[c] : d[c] * d[c];
                }
                if (total < P.background_ratio && dist2 < P.var_threshold * var) background = true;
                if (dist2 < P.var_threshold_gen * var) {
                    fits = true;
                    w += alphaT;
                    const float k = alphaT / w;
#pragma unroll
                    for (int c = 0; c < CN; c++) g.mu[m][c] -= k * d[c];
                    float vn = var + k * (dist2 - var);
                    vn = vn > P.var_min ? vn : P.var_min;
                    vn = vn < P.var_max ? vn : P.var_max;
                    g.vr[m] = vn;
                    g.dirty |= 1u << m;
                    bool go = true;
#pragma unroll
                    for (int i = m; i > 0; i--) {
                        if (go) {
                            if (w < g.wt[i - 1]) go = false;
                            else swaps++, swap_modes(g, i);
                        }
                    }
                }
            }
            if (w < -prune) w = 0.f, n--;
#pragma unroll
            for (int j = 0; j <= m; j++)
                if (j == m - swaps) g.wt[j] = w;
            total += w;
        }
    }
    total = 1.f / total;
#pragma unroll
    for (int m = 0; m < NM; m++)
        if (m < n) g.wt[m] *= total;
    n = n0;   // the count is restored: a pruned mode stays, with weight 0
    if (!fits) {
        if (n != NM) n++;
        // the new mode's slot is n - 1 either way
#pragma unroll
        for (int j = 0; j < NM; j++) {
            if (j == n - 1) {
                g.wt[j] = n == 1 ? 1.f : alphaT;
#pragma unroll
                for (int c = 0; c < CN; c++) g.mu[j][c] = data[c];
                g.vr[j] = P.var_init;
                g.dirty |= 1u << j;
            } else if (j < n - 1) {
                g.wt[j] *= alpha1;
            }
        }
        bool go = true;
#pragma unroll
        for (int i = NM - 1; i > 0; i--) {
            if (i <= n - 1 && go) {
                if (alphaT < g.wt[i - 1]) go = false;
                else swap_modes(g, i);
            }
        }
    }
    g.modes = n;
    if (background) return 0;
    if (P.detect_shadows && bg_shadow(g, data, P)) return (uint8_t)P.shadow_value;
    return 255;
}

__device__ __forceinline__ float canonical_nan(float v) { return v != v ? __uint_as_float(0x7fc00000u) : v; }

struct BgApplyArgs {
    BgModel M;
    const uint8_t* frames;
    uint8_t* mask;                 // may be null
    int stride, T;
    size_t frame_stride, stream_stride;
    size_t mask_stream_stride;     // bytes between two streams' masks; frames of a stream are w * h apart
    float alphaT[kBgMaxFrames];
};

template <int CN> __device__ __forceinline__ void load_pixel(const uint8_t* __restrict__ p, float (&data)[CN])
{
#pragma unroll
    for (int c = 0; c < CN; c++) data[c] = (float)p[c];
}

}  // namespace

// grid (ceil(w * h / 256), streams), 256 threads
template <int CN, int NM> __global__ __launch_bounds__(256) void k_bg_apply(BgApplyArgs a)
{
    const size_t N = (size_t)a.M.w * a.M.h;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const int s = blockIdx.y;
    float* __restrict__ st = a.M.state + (size_t)s * bg_state_floats(a.M.w, a.M.h, CN, NM) + p;
    uint8_t* __restrict__ md = a.M.modes + (size_t)s * N + p;
    const int y = (int)(p / a.M.w), x = (int)(p - (size_t)y * a.M.w);
    const uint8_t* __restrict__ px = a.frames + (size_t)s * a.stream_stride + (size_t)y * a.stride + (size_t)x * CN;
    float data[CN];
    load_pixel<CN>(px, data);

    Mixture<CN, NM> g;
    g.modes = *md;
    g.dirty = 0;
#pragma unroll
    for (int m = 0; m < NM; m++) {
        g.wt[m] = 0.f, g.vr[m] = 0.f;
#pragma unroll
        for (int c = 0; c < CN; c++) g.mu[m][c] = 0.f;
        if (m < g.modes) {
            g.wt[m] = st[(size_t)m * N];
            g.vr[m] = st[(size_t)(NM + m) * N];
#pragma unroll
            for (int c = 0; c < CN; c++) g.mu[m][c] = st[(size_t)(2 * NM + m * CN + c) * N];
        }
    }
    const int modes0 = g.modes;
    uint8_t* mk = a.mask ? a.mask + (size_t)s * a.mask_stream_stride + p : nullptr;
    for (int t = 0; t < a.T; t++) {
        float next[CN];
#pragma unroll
        for (int c = 0; c < CN; c++) next[c] = 0.f;
        if (t + 1 < a.T) load_pixel<CN>(px + (size_t)(t + 1) * a.frame_stride, next);   // in flight during the update
        const uint8_t v = bg_update<CN, NM>(g, data, a.alphaT[t], a.M.prm);
        if (mk) mk[(size_t)t * N] = v;
#pragma unroll
        for (int c = 0; c < CN; c++) data[c] = next[c];
    }
    if (g.modes != modes0) *md = (uint8_t)g.modes;
#pragma unroll
    for (int m = 0; m < NM; m++) {
        if (m < g.modes) {
            st[(size_t)m * N] = canonical_nan(g.wt[m]);
            if ((g.dirty >> m) & 1u) {
                st[(size_t)(NM + m) * N] = canonical_nan(g.vr[m]);
#pragma unroll
                for (int c = 0; c < CN; c++) st[(size_t)(2 * NM + m * CN + c) * N] = canonical_nan(g.mu[m][c]);
            }
        }
    }
}

// grid (ceil(w * h / 256), streams), 256 threads; out [streams][h][w][CN]
template <int CN, int NM> __global__ __launch_bounds__(256) void k_bg_image(BgModel M, uint8_t* __restrict__ out)
{
    const size_t N = (size_t)M.w * M.h;
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const int s = blockIdx.y;
    const float* __restrict__ st = M.state + (size_t)s * bg_state_floats(M.w, M.h, CN, NM) + p;
    const int modes = M.modes[(size_t)s * N + p];
    float acc[CN], tot = 0.f;
#pragma unroll
    for (int c = 0; c < CN; c++) acc[c] = 0.f;
    bool done = false;
#pragma unroll
    for (int m = 0; m < NM; m++) {
        if (m < modes && !done) {
            const float w = st[(size_t)m * N];
#pragma unroll
            for (int c = 0; c < CN; c++) acc[c] += w * st[(size_t)(2 * NM + m * CN + c) * N];
            tot += w;
            if (tot > M.prm.background_ratio) done = true;
        }
    }
    const float inv = 1.f / tot;
    uint8_t* o = out + ((size_t)s * N + p) * CN;
#pragma unroll
    for (int c = 0; c < CN; c++) {
        float v = acc[c] * inv;
        v = v >= 0.f ? v : 0.f;        // a NaN goes to 0
        v = v > 255.f ? 255.f : v;
        o[c] = modes ? (uint8_t)rintf(v) : 0;
    }
}

namespace {

// the (channels, nmixtures) specialisation: F is called with two integral constants
template <typename F> bool bg_dispatch(int cn, int nm, F&& f)
{
    auto by_nm = [&](auto CN) {
        switch (nm) {
        case 1: f(CN, std::integral_constant<int, 1>{}); return true;
        case 2: f(CN, std::integral_constant<int, 2>{}); return true;
        case 3: f(CN, std::integral_constant<int, 3>{}); return true;
        case 4: f(CN, std::integral_constant<int, 4>{}); return true;
        case 5: f(CN, std::integral_constant<int, 5>{}); return true;
        case 6: f(CN, std::integral_constant<int, 6>{}); return true;
        case 7: f(CN, std::integral_constant<int, 7>{}); return true;
        case 8: f(CN, std::integral_constant<int, 8>{}); return true;
        }
        return false;
    };
    if (cn == 1) return by_nm(std::integral_constant<int, 1>{});
    if (cn == 3) return by_nm(std::integral_constant<int, 3>{});
    return false;
}

inline bool bg_grid(const BgModel& M, dim3* grid)
{
    const size_t N = (size_t)M.w * M.h, nb = (N + 255) / 256;
    if (M.w < 1 || M.h < 1 || M.streams < 1 || M.streams > kBgMaxStreams || nb > 0x7fffffffu) return false;
    *grid = dim3((unsigned)nb, (unsigned)M.streams);
    return true;
}

}  // namespace

hipError_t launch_bg_apply(hipStream_t s, const BgModel& M, int T, const uint8_t* frames, int stride, size_t frame_stride,
                           size_t stream_stride, const float* alphaT, uint8_t* mask, size_t mask_stream_stride)
{
    dim3 grid;
    if (!bg_grid(M, &grid) || T < 1 || T > kBgMaxFrames) return hipErrorInvalidValue;
    BgApplyArgs a{};
    a.M = M, a.frames = frames, a.mask = mask, a.stride = stride, a.T = T;
    a.frame_stride = frame_stride, a.stream_stride = stream_stride, a.mask_stream_stride = mask_stream_stride;
    for (int t = 0; t < T; t++) a.alphaT[t] = alphaT[t];
    const bool ok = bg_dispatch(M.channels, M.prm.nmixtures, [&](auto CN, auto NM) {
        hipLaunchKernelGGL((k_bg_apply<decltype(CN)::value, decltype(NM)::value>), grid, dim3(256), 0, s, a);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_bg_image(hipStream_t s, const BgModel& M, uint8_t* out)
{
    dim3 grid;
    if (!bg_grid(M, &grid)) return hipErrorInvalidValue;
    const bool ok = bg_dispatch(M.channels, M.prm.nmixtures, [&](auto CN, auto NM) {
        hipLaunchKernelGGL((k_bg_image<decltype(CN)::value, decltype(NM)::value>), grid, dim3(256), 0, s, M, out);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace mdx
