// mdx_dev.h -- device-only helpers shared by the stage kernel files (mdx_front.hip, mdx_lk.hip,
// mdx_lk_point.hip, mdx_hull.hip): reflect-101 indexing, 4-byte-aligned vector loads, the gray
// conversion, the per-pixel Scharr stencil (k_scharr, k_scharr_levels, k_lk_class_fused), a workgroup
// scan.  Nothing host-visible: mdx_internal.h is the one host/device interface.
#pragma once

#include "mdx_internal.h"

namespace mdx {

__device__ __forceinline__ int r101(int p, int len)
{
    // borderInterpolate(p, len, BORDER_REFLECT_101), any number of folds.
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do {
        if (p < 0) p = -p;
        else p = 2 * len - 2 - p;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}

// Front-end kernels (A1, A3, A4) work on aligned 16-byte chunks of each padded row (4 words
// for the derivative rows): a level's padded columns -40 .. w+39 sit at row bytes 24 .. 64+w+39
// and every row has >= 16 B of slack after them, so a chunk may spill into the unused margin.
// Interior chunks take vector loads; chunks that touch a border fall back to per-pixel
// reflect-101 addressing.  One aligned dwordx4 store per thread.
struct __attribute__((aligned(4))) u4a4k { uint32_t x, y, z, w; };
struct __attribute__((aligned(4))) u3a4k { uint32_t x, y, z; };
struct __attribute__((aligned(4))) u2a4k { uint32_t x, y; };
// a load from a global address held as an integer: through an address-space-1 pointer, so that it is
// a global_load (vmcnt only).  Through a generic pointer it is a flat_load, which also counts in
// lgkmcnt: every LDS wait would then wait for it, and a load issued ahead of use would be waited
// for at the next LDS access.
template <typename T>
__device__ __forceinline__ T gload(uintptr_t a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const __attribute__((address_space(1))) T*>(a);
#else
    return *reinterpret_cast<const T*>(a);   // the host pass only type-checks device code
#endif
}

// Exclusive prefix sum of v over a workgroup of T threads (a multiple of 64), in thread order; total
// receives the sum.  wsum: T / 64 ints of LDS, free again on return.  Every thread must call it.
template <int T>
__device__ __forceinline__ int block_scan_exclusive(int v, int* wsum, int& total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < T / 64; i++) {
        const int s = wsum[i];
        if (i < w) off += s;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return off + inc - v;
}

// ---- the Scharr stencil (lkpyramid.cpp calcSharrDeriv), one pixel.  Vertical t0 = 3(a+c)+10b, t1 = c-a
// over the rows above / at / below; horizontal Ix = t0[x+1]-t0[x-1], Iy = 3(t1[x-1]+t1[x+1])+10 t1[x].
// OpenCV clamps the row/col neighbours as reflect-101 (row -1 -> 1, col cols -> cols-2), which is exactly
// the padded level's border, so the stencil reads the padded image directly.  ra / rb / rc: three aligned
// words of the three rows, the pixel at byte bc (1 <= bc <= 10).  Returns (uint16)Ix | (uint16)Iy << 16.
__device__ __forceinline__ int u8_at(const uint32_t (&w)[3], int b) { return (int)((w[b >> 2] >> (8 * (b & 3))) & 255u); }

__device__ __forceinline__ uint32_t scharr_word(const uint32_t (&ra)[3], const uint32_t (&rb)[3], const uint32_t (&rc)[3],
                                                int bc)
{
    const int bm = bc - 1, bp = bc + 1;                              // bytes x-1, x+1
    const int t0m = (u8_at(ra, bm) + u8_at(rc, bm)) * 3 + u8_at(rb, bm) * 10;
    const int t0p = (u8_at(ra, bp) + u8_at(rc, bp)) * 3 + u8_at(rb, bp) * 10;
    const int t1m = u8_at(rc, bm) - u8_at(ra, bm), t1c = u8_at(rc, bc) - u8_at(ra, bc), t1p = u8_at(rc, bp) - u8_at(ra, bp);
    const int ix = t0p - t0m;
    const int iy = (t1m + t1p) * 3 + t1c * 10;
    return (uint32_t)(uint16_t)(int16_t)ix | ((uint32_t)(uint16_t)(int16_t)iy << 16);
}

__device__ __forceinline__ int gray_of(const uint8_t* s, int fmt)
{
    // color.cpp RGB2Gray<uchar>, blueIdx 0 on rgb8 data: R gets the blue weight
    if (fmt == 1) return (s[0] * 1868 + s[1] * 9617 + s[2] * 4899 + 8192) >> 14;
    return (s[2] * 1868 + s[1] * 9617 + s[0] * 4899 + 8192) >> 14;   // bgr8 -> converted to rgb8 first
}

__device__ __forceinline__ void gray_chunk(const uint8_t* s, int px0, int w, int fmt, uint32_t (&o)[4])
{
    if (px0 >= 0 && px0 + 16 <= w && fmt == 0 && (((uintptr_t)(s + px0)) & 3) == 0) {
        const u4a4k v = *reinterpret_cast<const u4a4k*>(s + px0);
        o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
    } else if (px0 >= 0 && px0 + 16 <= w && fmt != 0 && (((uintptr_t)(s + 3 * px0)) & 3) == 0) {
        uint32_t b[12];
        const u4a4k* q = reinterpret_cast<const u4a4k*>(s + 3 * px0);
#pragma unroll
        for (int t = 0; t < 3; t++) { const u4a4k v = q[t]; b[4 * t] = v.x; b[4 * t + 1] = v.y; b[4 * t + 2] = v.z; b[4 * t + 3] = v.w; }
        const uint8_t* bb = reinterpret_cast<const uint8_t*>(b);
#pragma unroll
        for (int t = 0; t < 4; t++) {
            uint32_t d = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) d |= (uint32_t)gray_of(bb + 3 * (4 * t + i), fmt) << (8 * i);
            o[t] = d;
        }
    } else {
        for (int t = 0; t < 4; t++) {
            uint32_t d = 0;
            for (int i = 0; i < 4; i++) {
                const int px = px0 + 4 * t + i;
                if (px < -kPad || px >= w + kPad) continue;           // row margin: value unused
                const int sx = r101(px, w);
                d |= (uint32_t)(fmt == 0 ? s[sx] : gray_of(s + 3 * sx, fmt)) << (8 * i);
            }
            o[t] = d;
        }
    }
}

}  // namespace mdx
