// lk_jbias_check.cpp -- k_lk_iter's route from the J - I dot-product word to a float (lk_jd512,
// motion_detection_amd/csrc/mdx_plan.h) run on a CPU: the identity over every value the word can
// take, the range it rests on, and the scaled products and running sums against the unscaled ones.
// Violations go to stderr; the exit status is 1 when there was one.  One summary line on stdout.
//   g++ -std=c++17 -O1 -ffp-contract=off -I motion_detection_amd/csrc tests/lk_jbias_check.cpp
#include "mdx_plan.h"

#include <cstdio>
#include <cstring>

using namespace mdx;

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond) && ++g_fail <= 40) {                  \
            fprintf(stderr, "FAIL %s: ", #cond);          \
            fprintf(stderr, __VA_ARGS__);                 \
            fputc('\n', stderr);                          \
        }                                                 \
    } while (0)

static uint32_t bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, sizeof(u));
    return u;
}

// what the row body computed before: the shift, then the integer convert
static float jd_float(int x) { return (float)(x >> kLkJShift); }

int main()
{
    // 1. the range of x = S + 256 - 512*I from the weight and tap bounds: w00, w01, w10 >= 0 and
    // w11 >= -1 summing to 16384 over bytes, I*32 in [0, 8160]
    const long long smin = -1LL * 255, smax = (16384LL + 1) * 255;
    const long long xmin = smin + 256 - 512LL * (255 * 32), xmax = smax + 256;
    CHECK(xmin == kLkXMin && xmax == kLkXMax, "x in [%lld, %lld], header [%d, %d]", xmin, xmax, kLkXMin, kLkXMax);
    CHECK(xmin == -4177919 && xmax == 4178431, "x in [%lld, %lld]", xmin, xmax);
    CHECK(xmin > -(1LL << 22) && xmax < (1LL << 22), "x in [%lld, %lld] leaves (-2^22, 2^22)", xmin, xmax);
    CHECK(bits(kLkJBiasFloat) == kLkJBiasWord, "bias float %08x, word %08x", bits(kLkJBiasFloat), kLkJBiasWord);
    // the class plane's word plus the tap sum is the biased x, with no int32 wrap
    CHECK((long long)lk_class_c(kLkIMax) + smin == (long long)kLkJBiasWord + xmin, "C + S at the lower end");
    CHECK((long long)lk_class_c(0) + smax == (long long)kLkJBiasWord + xmax, "C + S at the upper end");
    CHECK((long long)kLkJBiasWord + xmax < (1LL << 31), "biased word stays a positive int32");

    // 2. the identity, bit for bit, for every x of the range (and every x of (-2^22, 2^22) besides)
    long long checked = 0;
    for (int x = -(1 << 22) + 1; x < (1 << 22); x++) {
        const float got = lk_jd512(kLkJBiasWord + (uint32_t)x), want = 512.f * jd_float(x);
        CHECK(bits(got) == bits(want), "x %d: %a (%08x), want %a (%08x)", x, got, bits(got), want, bits(want));
        if (x >= kLkXMin && x <= kLkXMax) checked++;
    }
    CHECK(checked == (long long)kLkXMax - kLkXMin + 1, "%lld values of the range", checked);

    // 3. products and running sums at the ends of jd's range: 512 times the unscaled ones, same
    // roundings, in the exact body's form (round the product, then add) and the fused body's (one fma)
    const int jds[2] = {kLkXMax >> kLkJShift, kLkXMin >> kLkJShift};
    const float fs[6] = {4080.f, -4080.f, 2056.f, -2056.f, 1.f, -1.f};
    CHECK(jds[0] == 8160 && jds[1] == -8160, "jd in [%d, %d]", jds[1], jds[0]);
    int sums = 0;
    float mix = 0.f, mix512 = 0.f, mixf = 0.f, mixf512 = 0.f;     // every combination in turn, 400 terms
    for (int t = 0; t < 400; t++) {
        const int ji = (t / 6) & 1, x = ji ? kLkXMin : kLkXMax;
        const float f = fs[t % 6], fd = jd_float(x), fd512 = lk_jd512(kLkJBiasWord + (uint32_t)x);
        mix = mix + f * fd;
        mix512 = mix512 + f * fd512;
        mixf = fmaf(f, fd, mixf);
        mixf512 = fmaf(f, fd512, mixf512);
        CHECK(bits(mix512) == bits(512.f * mix), "mixed sum, term %d: %a vs 512 * %a", t, mix512, mix);
        CHECK(bits(mixf512) == bits(512.f * mixf), "mixed fused sum, term %d: %a vs 512 * %a", t, mixf512, mixf);
    }
    for (int ji = 0; ji < 2; ji++)
        for (int fi = 0; fi < 6; fi++) {
            const int x = ji ? kLkXMin : kLkXMax;
            const float f = fs[fi], fd = (float)jds[ji], fd512 = lk_jd512(kLkJBiasWord + (uint32_t)x);
            CHECK(bits(fd512) == bits(512.f * fd), "jd %d: %a", jds[ji], fd512);
            CHECK(bits(f * fd512) == bits(512.f * (f * fd)), "f %g jd %d: product %a vs 512 * %a", f, jds[ji], f * fd512, f * fd);
            float acc = 0.f, acc512 = 0.f, accf = 0.f, accf512 = 0.f;
            for (int t = 0; t < 400; t++) {
                acc = acc + f * fd;
                acc512 = acc512 + f * fd512;
                accf = fmaf(f, fd, accf);
                accf512 = fmaf(f, fd512, accf512);
                CHECK(bits(acc512) == bits(512.f * acc), "f %g jd %d term %d: %a vs 512 * %a", f, jds[ji], t, acc512, acc);
                CHECK(bits(accf512) == bits(512.f * accf), "fused, f %g jd %d term %d: %a vs 512 * %a", f, jds[ji], t, accf512, accf);
            }
            // the final scale: 2^-29 of the scaled sum is 2^-20 of the reference's
            CHECK(bits(acc512 * (1.f / (1 << 29))) == bits(acc * (1.f / (1 << 20))), "f %g jd %d: final scale", f, jds[ji]);
            sums++;
        }
    printf("{\"x_checked\": %lld, \"x_min\": %d, \"x_max\": %d, \"sums\": %d, \"failures\": %d}\n", checked, kLkXMin, kLkXMax,
           sums, g_fail);
    return g_fail ? 1 : 0;
}
