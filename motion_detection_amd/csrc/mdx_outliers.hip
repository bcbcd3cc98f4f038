// mdx_outliers.hip -- flow-vector outliers by median / MAD: OutlierDetector::findOutliers
// (reference common/src/outlier_detector.cpp:37-186: createAngleMatrix, createMagnitudeMatrix,
// getMedian, createMask).  Pinned against this reading of the source; unpinned against a real build.
//
// Per field of n vectors and per channel (angle, magnitude) the reference sorts the selected values
// for their median, sorts |value - median| for the MAD, and flags every selected vector whose
// modified z-score 0.6745 * |value - median| / MAD exceeds 3.5.  The four sorts are four exact order
// statistics, found here by radix select:
//   value -> key   the 64 bits of the double, sign flipped for non-negatives and every bit flipped
//                  for negatives: unsigned key order is the doubles' order (-0.0 just below +0.0).
//   select(r)      the key of rank r among the selected values, one 8-bit digit per pass from the
//                  top: a 256-bin histogram of the digit over the keys that match the digits fixed
//                  so far (one copy per wave in LDS), the bin that holds rank r, the count below it.
//                  Eight passes; each goes over the channel's values again and, for the MAD,
//                  recomputes |value - median| from them (the diffs are never stored).
//   median         select(m / 2).  For odd m that is it.  For even m the lower middle element is the
//                  same value unless exactly m / 2 values lie below it; then it is their maximum,
//                  one more pass.  median = (lower + upper) / 2.0.
// The angle comes from the host (libm atan2, no device transcendentals); the magnitude
// sqrt(dy*dy + dx*dx), the differences, the z-score and the compare run here with explicitly rounded
// operations, denormals kept.  A vector outside the selected set carries NaN as its value in both
// channels: a NaN matches no histogram and fails the final compare, as does the 0 / 0 of a zero
// difference over a zero MAD.
//
// One workgroup per field runs everything in turn and writes each flag byte once; a batch is one
// launch and no workgroup waits for another.  Nothing needs clearing between calls.
//
// Where the values live (k_outliers<kR>).  Fields of up to 4,096 and 24,576 vectors (kR = 4, 24) keep
// a channel's values in registers, kR per thread, from one read of the planes; larger fields (kR = 0)
// re-read them from global memory on every pass (8 B per vector, L2-resident), after a first pass
// that writes the magnitudes and the NaN marks.  Measured at 20,736 vectors: 162 us against 196 us
// (profiles/outliers_timing.txt); MDX_OL_REG=0 selects the re-reading kernel at every size.  The
// 24-value kernel sits at the 128-VGPR limit of a 1,024-thread workgroup and spills seven index words
// once, outside the passes.
#include "mdx_internal.h"

namespace mdx {

constexpr int kOlT = 1024;             // threads of k_outliers
constexpr int kOlW = kOlT / 64;        // waves
constexpr int kOlU = 4;                // loads in flight per thread and pass
constexpr int kOlRegSmall = 4;         // values per thread the register variants hold: fields of up to
constexpr int kOlRegLarge = 24;        // 4,096 and 24,576 vectors (a 1080p grid at pixel_step 10: 20,736)

struct OlShared {
    uint32_t hist[kOlW][256];          // digit histograms, one per wave
    uint32_t tot[256];                 // their sum
    uint32_t digit, below;             // the bin that holds the wanted rank, the count in the bins before it
    uint32_t cnt[4];                   // selected, flagged by angle, by magnitude, by either
    unsigned long long best;           // ol_max_below
};

__device__ __forceinline__ unsigned long long ol_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : b ^ 0x8000000000000000ull;
}

__device__ __forceinline__ double ol_unkey(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? k ^ 0x8000000000000000ull : ~k));
}

// the value a pass ranks: the channel value, or its distance from the median (NaN stays NaN)
template <bool kDiff> __device__ __forceinline__ double ol_value(double v, double med)
{
    return kDiff ? fabs(__dsub_rn(v, med)) : v;
}

// One count into this wave's histogram.  Coherent flow puts most of a wave into one bin of the
// upper digits (sign and exponent), and LDS atomics on one address run one after another: the lanes
// that share the first active lane's digit are counted with one add.
__device__ __forceinline__ void ol_count(uint32_t* h, bool act, uint32_t d, int lane)
{
    const unsigned long long am = __ballot(act);
    if (am == 0) return;               // wave-uniform
    const int first = __ffsll((long long)am) - 1;
    const uint32_t d0 = (uint32_t)__shfl((int)d, first);
    const bool same = act && d == d0;
    const unsigned long long sm = __ballot(same);
    if (lane == first) atomicAdd(&h[d0], (uint32_t)__popcll(sm));
    if (act && !same) atomicAdd(&h[d], 1u);
}

// The values a workgroup ranks.  kR > 0: thread t holds value j * kOlT + t in x[j] (NaN past the end
// and outside the selected set), up to kR * kOlT values; kR == 0: every pass re-reads plane v.
template <int kR> struct OlSrc {
    const double* v;
    int n;
    double x[kR > 0 ? kR : 1];
};

template <bool kDiff>
__device__ __forceinline__ void ol_count_value(double x, double med, unsigned long long mask, unsigned long long prefix,
                                               int shift, uint32_t* h, int lane)
{
    const double y = ol_value<kDiff>(x, med);
    const unsigned long long k = ol_key(y);
    ol_count(h, y == y && (k & mask) == prefix, (uint32_t)(k >> shift) & 255u, lane);
}

// The key of rank r (0-based, r < the number of non-NaN values) among the values of s, and *less, the
// number of keys below it.  Every thread of the workgroup calls it and gets the result.  sh.hist is
// all zero on entry and on return.
template <bool kDiff, int kR>
__device__ __forceinline__ unsigned long long ol_select(const OlSrc<kR>& s, double med, uint32_t r, OlShared& sh,
                                                        uint32_t* less)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    unsigned long long prefix = 0, mask = 0;
    uint32_t lt = 0;
#pragma unroll 1
    for (int shift = 56; shift >= 0; shift -= 8) {
        if constexpr (kR > 0) {
#pragma unroll
            for (int j = 0; j < kR; j++) {
                // opaque copy: the key does not depend on the digit, and the compiler would keep all
                // kR of them next to the values across the passes (kR = 24: spills)
                double x = s.x[j];
                asm volatile("" : "+v"(x));
                ol_count_value<kDiff>(x, med, mask, prefix, shift, sh.hist[wave], lane);
            }
        } else {
#pragma unroll 1
            for (int base = 0; base < s.n; base += kOlU * kOlT) {     // wave-uniform trip count
                double x[kOlU];
#pragma unroll
                for (int u = 0; u < kOlU; u++) {
                    const int i = base + u * kOlT + tid;
                    x[u] = i < s.n ? s.v[i] : nan;
                }
#pragma unroll
                for (int u = 0; u < kOlU; u++) ol_count_value<kDiff>(x[u], med, mask, prefix, shift, sh.hist[wave], lane);
            }
        }
        __syncthreads();
        if (tid < 256) {
            uint32_t c = 0;
#pragma unroll
            for (int w = 0; w < kOlW; w++) {
                c += sh.hist[w][tid];
                sh.hist[w][tid] = 0;
            }
            sh.tot[tid] = c;
        }
        __syncthreads();
        if (tid < 64) {                // lane t: bins 4t .. 4t+3
            uint32_t q[4], sum = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                q[k] = sh.tot[4 * tid + k];
                sum += q[k];
            }
            uint32_t inc = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = (uint32_t)__shfl_up((int)inc, o);
                if (lane >= o) inc += t;
            }
            uint32_t exc = inc - sum;
            if (exc <= r && r < inc) {  // one lane: the candidates number more than r
                uint32_t d = 0;
#pragma unroll
                for (int k = 0; k < 3; k++)
                    if (d == (uint32_t)k && exc + q[k] <= r) {
                        exc += q[k];
                        d = k + 1;
                    }
                sh.digit = 4 * tid + d;
                sh.below = exc;
            }
        }
        __syncthreads();
        prefix |= (unsigned long long)sh.digit << shift;
        mask |= 255ull << shift;
        r -= sh.below;
        lt += sh.below;
        // (the next pass's first write to digit / below follows two more barriers)
    }
    *less = lt;
    return prefix;
}

// the largest key below `key` (there is one); every thread calls it and gets the result
template <bool kDiff, int kR>
__device__ __forceinline__ unsigned long long ol_max_below(const OlSrc<kR>& s, double med, unsigned long long key,
                                                           OlShared& sh)
{
    const int tid = threadIdx.x;
    if (tid == 0) sh.best = 0;
    __syncthreads();
    unsigned long long best = 0;       // a key below another one is a selected value's: never 0 (-NaN)
    auto take = [&](double x) {
        const double y = ol_value<kDiff>(x, med);
        const unsigned long long k = ol_key(y);
        if (y == y && k < key && k > best) best = k;
    };
    if constexpr (kR > 0) {
#pragma unroll
        for (int j = 0; j < kR; j++) take(s.x[j]);
    } else {
        for (int i = tid; i < s.n; i += kOlT) take(s.v[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = (unsigned long long)__shfl_xor((long long)best, o);
        best = t > best ? t : best;
    }
    if ((tid & 63) == 0) atomicMax(&sh.best, best);
    __syncthreads();
    const unsigned long long res = sh.best;
    __syncthreads();
    return res;
}

// getMedian (:97-119) of the m non-NaN values of s (of their distances from med0 when kDiff)
template <bool kDiff, int kR>
__device__ __forceinline__ double ol_median(const OlSrc<kR>& s, uint32_t m, double med0, OlShared& sh)
{
    uint32_t less;
    const unsigned long long hk = ol_select<kDiff>(s, med0, m / 2, sh, &less);
    const double hi = ol_unkey(hk);
    if (m & 1) return hi;
    const double lo = less == m / 2 ? ol_unkey(ol_max_below<kDiff>(s, med0, hk, sh)) : hi;
    return __ddiv_rn(__dadd_rn(lo, hi), 2.0);
}

// createMask's test (:166-167): 0.6745 * diff / MAD left to right; +inf passes, NaN does not
__device__ __forceinline__ bool ol_flag(double v, double med, double mad)
{
    return fabs(__ddiv_rn(__dmul_rn(0.6745, fabs(__dsub_rn(v, med))), mad)) > 3.5;
}

// createMagnitudeMatrix (:92)
__device__ __forceinline__ double ol_magnitude(double x, double y)
{
    return __dsqrt_rn(__dadd_rn(__dmul_rn(y, y), __dmul_rn(x, x)));
}

// grid: the fields.  dxy: [batch][2][n] (dx plane, dy plane); ang: [batch][n], the host's atan2;
// flags: [batch][n].  kR > 0 (n <= kR * kOlT): a channel's values stay in registers from one read,
// the angle's flag bits wait in a register for the magnitude's, and ang / mag are only read.  kR == 0:
// the first pass writes NaN over the entries of ang outside the selected set and fills mag
// ([batch][n] scratch), and every later pass re-reads one of the two planes.
template <int kR>
__global__ __launch_bounds__(kOlT) void k_outliers(const double* __restrict__ dxy, double* __restrict__ ang,
                                                    double* __restrict__ mag, int n, int include_zeros,
                                                    uint8_t* __restrict__ flags, mdx_outlier_stats* __restrict__ stats)
{
    __shared__ OlShared sh;
    const int tid = threadIdx.x, lane = tid & 63;
    const size_t f = blockIdx.x;
    const double* dx = dxy + f * 2 * (size_t)n;
    const double* dy = dx + n;
    double* a = ang + f * (size_t)n;
    double* g = mag + f * (size_t)n;
    uint8_t* fl = flags + f * (size_t)n;
    for (int k = tid; k < kOlW * 256; k += kOlT) (&sh.hist[0][0])[k] = 0;
    if (tid < 4) sh.cnt[tid] = 0;
    __syncthreads();
    // the selected set (:130-134)
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    OlSrc<kR> src;
    src.v = a;
    src.n = n;
    uint32_t mine = 0;
    if constexpr (kR > 0) {
#pragma unroll
        for (int j = 0; j < kR; j++) {
            const int i = j * kOlT + tid;
            bool sel = false;
            if (i < n) sel = include_zeros || fabs(dx[i]) > 0.0 || fabs(dy[i]) > 0.0;
            src.x[j] = sel ? a[i] : nan;
            mine += sel;
        }
    } else {
        for (int i = tid; i < n; i += kOlT) {
            const double x = dx[i], y = dy[i];
            const bool sel = include_zeros || fabs(x) > 0.0 || fabs(y) > 0.0;
            g[i] = sel ? ol_magnitude(x, y) : nan;
            if (!sel) a[i] = nan;
            mine += sel;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += (uint32_t)__shfl_xor((int)mine, o);
    if (lane == 0 && mine) atomicAdd(&sh.cnt[0], mine);
    __syncthreads();                   // (kR == 0: a thread re-reads only the entries of a / g it wrote)
    const uint32_t m = sh.cnt[0];
    double med[2] = {0.0, 0.0}, mad[2] = {0.0, 0.0};
    uint32_t abits = 0;                // kR > 0: bit j: value j of this thread is flagged by the angle
    if (m > 0) {                       // workgroup-uniform
        med[0] = ol_median<false>(src, m, 0.0, sh);
        mad[0] = ol_median<true>(src, m, med[0], sh);
        if constexpr (kR > 0) {
#pragma unroll
            for (int j = 0; j < kR; j++) {
                abits |= ol_flag(src.x[j], med[0], mad[0]) ? 1u << j : 0u;
                const int i = j * kOlT + tid;
                if (src.x[j] == src.x[j]) src.x[j] = ol_magnitude(dx[i], dy[i]);     // selected: i < n
            }
        } else {
            src.v = g;
        }
        med[1] = ol_median<false>(src, m, 0.0, sh);
        mad[1] = ol_median<true>(src, m, med[1], sh);
    }
    uint32_t ca = 0, cm = 0, co = 0;
    auto emit = [&](int i, bool fa, bool fm) {      // in wave-uniform control flow
        if (i < n) fl[i] = (uint8_t)((fa ? 1 : 0) | (fm ? 2 : 0));
        ca += (uint32_t)__popcll(__ballot(fa));
        cm += (uint32_t)__popcll(__ballot(fm));
        co += (uint32_t)__popcll(__ballot(fa || fm));
    };
    if constexpr (kR > 0) {
#pragma unroll
        for (int j = 0; j < kR; j++)
            if (j * kOlT < n)          // workgroup-uniform
                emit(j * kOlT + tid, (abits >> j) & 1u, m > 0 && ol_flag(src.x[j], med[1], mad[1]));
    } else {
        for (int base = 0; base < n; base += kOlT) {     // wave-uniform trip count
            const int i = base + tid;
            bool fa = false, fm = false;
            if (i < n && m > 0) {
                fa = ol_flag(a[i], med[0], mad[0]);
                fm = ol_flag(g[i], med[1], mad[1]);
            }
            emit(i, fa, fm);
        }
    }
    if (lane == 0) {
        if (ca) atomicAdd(&sh.cnt[1], ca);
        if (cm) atomicAdd(&sh.cnt[2], cm);
        if (co) atomicAdd(&sh.cnt[3], co);
    }
    __syncthreads();
    if (tid == 0) {
        mdx_outlier_stats st;
        st.selected = (int32_t)m;
        st.flagged_angle = (int32_t)sh.cnt[1];
        st.flagged_magnitude = (int32_t)sh.cnt[2];
        st.outliers = (int32_t)sh.cnt[3];
        st.median_angle = med[0];
        st.mad_angle = mad[0];
        st.median_magnitude = med[1];
        st.mad_magnitude = mad[1];
        stats[f] = st;
    }
}

hipError_t launch_outliers(hipStream_t s, int batch, int n, const double* dxy, double* ang, double* mag,
                           int include_zeros, uint8_t* flags, mdx_outlier_stats* stats, bool in_registers)
{
    if (batch <= 0 || n <= 0 || n > MDX_OUTLIERS_MAX_POINTS) return hipErrorInvalidValue;
    const dim3 grid(batch), block(kOlT);
    if (in_registers && n <= kOlRegSmall * kOlT)
        hipLaunchKernelGGL(k_outliers<kOlRegSmall>, grid, block, 0, s, dxy, ang, mag, n, include_zeros, flags, stats);
    else if (in_registers && n <= kOlRegLarge * kOlT)
        hipLaunchKernelGGL(k_outliers<kOlRegLarge>, grid, block, 0, s, dxy, ang, mag, n, include_zeros, flags, stats);
    else
        hipLaunchKernelGGL(k_outliers<0>, grid, block, 0, s, dxy, ang, mag, n, include_zeros, flags, stats);
    return hipGetLastError();
}

}  // namespace mdx
