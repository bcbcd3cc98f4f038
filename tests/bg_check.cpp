// bg_check.cpp -- a scalar restatement of the background-subtraction contract (include/mdx.h):
// OpenCV 2.4's MOG2Invoker, detectShadowGMM and getBackgroundImage as the header states them, one pixel at a
// time with plain loops and run-time indices.  It shares no code with the kernels.  tests/test_bg.py compiles it
// (g++ -O1 -ffp-contract=off), compares it word for word with a vectorised numpy restatement, and uses it as the
// oracle of the GPU tests; scripts/micro/bg_cpu.cpp includes it for the CPU timing (BG_CHECK_NO_MAIN).
//
//   bg_check IN OUT      (both binary, little endian)
// IN : int32 w, h, channels, T, has_state, nframes0; int32 history, nmixtures; float Tb, Tg, TB, var_init,
//      var_min, var_max, ct; int32 detect_shadows, shadow_value; float tau; double learning_rate;
//      T * h * w * channels frame bytes (packed); with has_state: weight [h][w][nmix], variance [h][w][nmix],
//      mean [h][w][nmix][channels] floats and modes [h][w] bytes.
// OUT: T masks [h][w]; T background images [h][w][channels] (after each frame); the final weight, variance, mean
//      and modes (entries at or above a pixel's count 0, a NaN as 0x7fc00000); int32 nframes; kNumCounters int64
//      branch counters, in the order of the enum below.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace bgc {

struct Params {
    int32_t history, nmixtures;
    float Tb, Tg, TB, var_init, var_min, var_max, ct;
    int32_t detect_shadows, shadow_value;
    float tau;
};

enum Counter {
    kFitMode0,            // fit found at mode 0
    kFitSwapped,          // fit found at mode >= 1 with >= 1 swap
    kVarClampLow,         // fit with the variance clamped low
    kVarClampHigh,        // fit with the variance clamped high
    kPruneLast,           // prune of the last mode
    kPruneNotLast,        // prune of a mode that is not the last (the loop bound shrinks)
    kNewAppended,         // new mode appended
    kNewReplaced,         // new mode replacing the weakest at a full mixture
    kNewBubbled,          // new mode bubbled above an older one
    kShadowTrue,          // shadow() true
    kShadowFalseTw,       // shadow() false by tw > TB
    kShadowDenZero,       // den == 0
    kBackgroundNotFirst,  // background via a mode other than the first
    kImageBreakEarly,     // background image breaking before the last mode
    kNumCounters
};

struct Model {
    int w = 0, h = 0, cn = 0;
    Params P{};
    int nframes = 0;
    std::vector<float> weight, variance, mean;   // [h][w][nmix], [h][w][nmix], [h][w][nmix][cn]
    std::vector<uint8_t> modes;
    long long counters[kNumCounters] = {};
    bool count = true;

    void init(int w_, int h_, int cn_, const Params& p)
    {
        w = w_, h = h_, cn = cn_, P = p, nframes = 0;
        const size_t N = (size_t)w * h;
        weight.assign(N * P.nmixtures, 0.f), variance.assign(N * P.nmixtures, 0.f);
        mean.assign(N * P.nmixtures * cn, 0.f), modes.assign(N, 0);
    }
    void bump(int c) { if (count) counters[c]++; }

    void swap_modes(float* wt, float* vr, float* mu, int i, int j) const
    {
        float t = wt[i]; wt[i] = wt[j]; wt[j] = t;
        t = vr[i]; vr[i] = vr[j]; vr[j] = t;
        for (int c = 0; c < cn; c++) { t = mu[i * cn + c]; mu[i * cn + c] = mu[j * cn + c]; mu[j * cn + c] = t; }
    }

    bool shadow(const float* wt, const float* vr, const float* mu, int n, const float* data)
    {
        float tw = 0.f;
        for (int m = 0; m < n; m++) {
            float num = 0.f, den = 0.f;
            for (int c = 0; c < cn; c++) {
                num += data[c] * mu[m * cn + c];
                den += mu[m * cn + c] * mu[m * cn + c];
            }
            if (den == 0.f) { bump(kShadowDenZero); return false; }
            if (num <= den && num >= P.tau * den) {
                const float a = num / den;
                float s = 0.f;
                for (int c = 0; c < cn; c++) {
                    const float e = a * mu[m * cn + c] - data[c];
                    s += e * e;
                }
                if (s < P.Tb * vr[m] * a * a) { bump(kShadowTrue); return true; }
            }
            tw += wt[m];
            if (tw > P.TB) { bump(kShadowFalseTw); return false; }
        }
        return false;
    }

    uint8_t pixel(size_t p, const uint8_t* px, float alphaT)
    {
        const int nmix = P.nmixtures;
        float* wt = &weight[p * nmix];
        float* vr = &variance[p * nmix];
        float* mu = &mean[p * nmix * cn];
        float data[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
        for (int c = 0; c < cn; c++) data[c] = (float)px[c];
        const float alpha1 = 1.f - alphaT, prune = -alphaT * P.ct;
        int n = modes[p];
        const int n0 = n;
        bool fits = false, background = false;
        float total = 0.f;
        for (int m = 0; m < n; m++) {
            float w = alpha1 * wt[m] + prune;
            int swaps = 0;
            if (!fits) {
                const float var = vr[m];
                float dist2 = 0.f;
                for (int c = 0; c < cn; c++) {
                    d[c] = mu[m * cn + c] - data[c];
                    const float sq = d[c] * d[c];
                    dist2 = c == 0 ? sq : dist2 + sq;
                }
                if (total < P.TB && dist2 < P.Tb * var) {
                    if (!background && m > 0) bump(kBackgroundNotFirst);
                    background = true;
                }
                if (dist2 < P.Tg * var) {
                    fits = true;
                    w += alphaT;
                    const float k = alphaT / w;
                    for (int c = 0; c < cn; c++) mu[m * cn + c] -= k * d[c];
                    float vn = var + k * (dist2 - var);
                    if (!(vn > P.var_min)) bump(kVarClampLow);
                    vn = vn > P.var_min ? vn : P.var_min;
                    if (!(vn < P.var_max)) bump(kVarClampHigh);
                    vn = vn < P.var_max ? vn : P.var_max;
                    vr[m] = vn;
                    for (int i = m; i > 0; i--) {
                        if (w < wt[i - 1]) break;
                        swaps++;
                        swap_modes(wt, vr, mu, i, i - 1);
                    }
                    if (m == 0) bump(kFitMode0);
                    if (m >= 1 && swaps >= 1) bump(kFitSwapped);
                }
            }
            if (w < -prune) {
                bump(m == n - 1 ? kPruneLast : kPruneNotLast);
                w = 0.f;
                n--;
            }
            wt[m - swaps] = w;
            total += w;
        }
        total = 1.f / total;
        for (int m = 0; m < n; m++) wt[m] *= total;
        n = n0;
        if (!fits) {
            int m;
            if (n == nmix) { m = nmix - 1; bump(kNewReplaced); }
            else { m = n++; bump(kNewAppended); }
            if (n == 1) wt[m] = 1.f;
            else {
                wt[m] = alphaT;
                for (int i = 0; i < n - 1; i++) wt[i] *= alpha1;
            }
            for (int c = 0; c < cn; c++) mu[m * cn + c] = data[c];
            vr[m] = P.var_init;
            bool bubbled = false;
            for (int i = n - 1; i > 0; i--) {
                if (alphaT < wt[i - 1]) break;
                swap_modes(wt, vr, mu, i, i - 1);
                bubbled = true;
            }
            if (bubbled) bump(kNewBubbled);
        }
        modes[p] = (uint8_t)n;
        if (background) return 0;
        if (P.detect_shadows && shadow(wt, vr, mu, n, data)) return (uint8_t)P.shadow_value;
        return 255;
    }

    static float alpha_of(const Params& P, int nframes, double learning_rate)
    {
        if (learning_rate >= 0 && nframes > 1) return (float)learning_rate;
        const long long a = 2ll * nframes, b = P.history;
        return (float)(1.0 / (double)(a < b ? a : b));
    }

    // rows [y0, y1) of one frame whose alphaT the caller computed (the threaded CPU timing splits the rows)
    void apply_rows(const uint8_t* frame, float alphaT, uint8_t* mask, int y0, int y1)
    {
        for (int y = y0; y < y1; y++)
            for (int x = 0; x < w; x++) {
                const size_t p = (size_t)y * w + x;
                const uint8_t v = pixel(p, frame + p * cn, alphaT);
                if (mask) mask[p] = v;
            }
    }

    void apply(const uint8_t* frame, double learning_rate, uint8_t* mask)
    {
        nframes++;
        apply_rows(frame, alpha_of(P, nframes, learning_rate), mask, 0, h);
    }

    void image(uint8_t* out)
    {
        const int nmix = P.nmixtures;
        for (size_t p = 0; p < (size_t)w * h; p++) {
            float acc[3] = {0.f, 0.f, 0.f}, tot = 0.f;
            const int n = modes[p];
            for (int m = 0; m < n; m++) {
                const float wm = weight[p * nmix + m];
                for (int c = 0; c < cn; c++) acc[c] += wm * mean[(p * nmix + m) * cn + c];
                tot += wm;
                if (tot > P.TB) {
                    if (m < n - 1) bump(kImageBreakEarly);
                    break;
                }
            }
            const float inv = 1.f / tot;
            for (int c = 0; c < cn; c++) {
                float v = acc[c] * inv;
                v = v >= 0.f ? v : 0.f;   // a NaN gives 0
                v = v > 255.f ? 255.f : v;
                out[p * cn + c] = n ? (uint8_t)nearbyintf(v) : 0;   // half to even (the default rounding mode)
            }
        }
    }
};

}  // namespace bgc

#ifndef BG_CHECK_NO_MAIN
namespace {

bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

void put_floats(FILE* f, const std::vector<float>& v, const std::vector<uint8_t>& modes, int nmix, int per_mode)
{
    std::vector<uint32_t> o(v.size());
    for (size_t p = 0; p < modes.size(); p++)
        for (int m = 0; m < nmix; m++)
            for (int k = 0; k < per_mode; k++) {
                const size_t i = (p * nmix + m) * per_mode + k;
                uint32_t u;
                memcpy(&u, &v[i], 4);
                if (v[i] != v[i]) u = 0x7fc00000u;
                o[i] = m < modes[p] ? u : 0u;
            }
    fwrite(o.data(), 4, o.size(), f);
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 3) return fprintf(stderr, "usage: bg_check IN OUT\n"), 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return perror(argv[1]), 2;
    int32_t hd[6];
    bgc::Params P;
    double lr;
    static_assert(sizeof(bgc::Params) == 48, "twelve 4-byte fields");
    if (!rd(in, hd, sizeof hd) || !rd(in, &P, sizeof P) || !rd(in, &lr, 8)) return fprintf(stderr, "short header\n"), 2;
    const int w = hd[0], h = hd[1], cn = hd[2], T = hd[3], has_state = hd[4];
    if (w < 1 || h < 1 || (cn != 1 && cn != 3) || T < 0 || P.nmixtures < 1 || P.nmixtures > 8) return fprintf(stderr, "bad header\n"), 2;
    const size_t N = (size_t)w * h;
    std::vector<uint8_t> frames(N * cn * T);
    if (!rd(in, frames.data(), frames.size())) return fprintf(stderr, "short frames\n"), 2;
    bgc::Model M;
    M.init(w, h, cn, P);
    if (has_state) {
        if (!rd(in, M.weight.data(), M.weight.size() * 4) || !rd(in, M.variance.data(), M.variance.size() * 4) ||
            !rd(in, M.mean.data(), M.mean.size() * 4) || !rd(in, M.modes.data(), N))
            return fprintf(stderr, "short state\n"), 2;
        for (uint8_t m : M.modes)
            if (m > P.nmixtures) return fprintf(stderr, "bad modes\n"), 2;
    }
    M.nframes = hd[5];
    fclose(in);
    std::vector<uint8_t> masks(N * T), images(N * cn * T);
    for (int t = 0; t < T; t++) {
        M.apply(&frames[N * cn * t], lr, &masks[N * t]);
        M.image(&images[N * cn * t]);
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return perror(argv[2]), 2;
    fwrite(masks.data(), 1, masks.size(), out);
    fwrite(images.data(), 1, images.size(), out);
    put_floats(out, M.weight, M.modes, P.nmixtures, 1);
    put_floats(out, M.variance, M.modes, P.nmixtures, 1);
    put_floats(out, M.mean, M.modes, P.nmixtures, cn);
    fwrite(M.modes.data(), 1, N, out);
    const int32_t nf = M.nframes;
    fwrite(&nf, 4, 1, out);
    long long cnt[bgc::kNumCounters];
    for (int i = 0; i < bgc::kNumCounters; i++) cnt[i] = M.counters[i];
    fwrite(cnt, 8, bgc::kNumCounters, out);
    return fclose(out) == 0 ? 0 : 2;
}
#endif
