// mdx_resize.hip -- half-size ingest: the reference node's
// cv::resize(img, out, cv::Size(), 0.5, 0.5) of every frame wider than 320 px (ros/src/motion_detection_node.cpp:470-474),
// as OpenCV 2.4.8 computes it: INTER_LINEAR at an integer scale of 2 is redirected to INTER_AREA's
// resizeAreaFast_, whose 2x2 fast mode is (a + b + c + d + 2) >> 2 per channel.  Restated from the
// published algorithm; unpinned against a real build (no OpenCV 2.4 here).
//
//   destination size   cvRound(w * 0.5) x cvRound(h * 0.5), half to even (mdx_half_size)
//   full cell          2dx + 1 < w and 2dy + 1 < h: (sum of the 2x2 block + 2) >> 2
//   partial cell       an odd side that rounded up: cvRound((float)sum / count) over the in-frame pixels
//                      of the block (count 2 on an edge, 1 in the corner), half to even
//   dropped pixels     an odd side that rounded down: the last source column / row is read by nothing
//
// One launch serves a batch.  A workgroup owns kHalfRows destination rows of one frame, kHalfWgPx
// destination pixels wide; a lane owns kHalfPx adjacent destination pixels of each of them.  It is a
// streaming kernel (every source byte read once, every destination byte written once), so the vector
// path's loads and stores are non-temporal.
//   vector path   (every base and pitch a multiple of 4) a lane whose kHalfPx cells are all full loads
//                 its 2 * kHalfPx source pixels of both rows as dwords and stores kHalfPx * channels
//                 bytes as dwords; the lanes at the partial or dropped edge, and the partial last row,
//                 take the byte path's cell
//   byte path     (anything else: rgb rows at an arbitrary pitch are 1-byte aligned) every cell by
//                 guarded byte loads and a byte store
// No lane reads a byte outside w * channels of a row or outside the h rows, and none writes past
// dw * channels of a destination row: a vector lane's loads end at pixel 8u + 8 <= w and its stores at
// pixel 4u + 4 <= dw; the byte path tests every tap.
#include "mdx_internal.h"

namespace mdx {

namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// rows are 4-byte aligned on the vector path, no more
typedef u32x2 u32x2_a4 __attribute__((aligned(4)));
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));

struct HalfArgs {
    const uint8_t* src;
    uint8_t* dst;
    int w, h, dw, dh;
    int stride, dst_stride;
    size_t frame_stride, dst_frame_stride;
};

// one destination byte by guarded byte loads: any cell, full or partial
__device__ __forceinline__ uint8_t half_cell(const uint8_t* __restrict__ src, int stride, int w, int h, int cn, int dx,
                                             int dy, int c)
{
    const bool x1 = 2 * dx + 1 < w, y1 = 2 * dy + 1 < h;
    const uint8_t* p = src + (size_t)(2 * dy) * stride + (size_t)(2 * dx) * cn + c;   // 2dx < w, 2dy < h always
    int s = p[0];
    if (x1) s += p[cn];
    if (y1) s += p[stride];
    if (x1 && y1) return (uint8_t)((s + p[stride + cn] + 2) >> 2);
    if (!x1 && !y1) return (uint8_t)s;
    const int q = s >> 1;                 // cvRound(s / 2.f): a tie goes to the even neighbour
    return (uint8_t)(q + (s & q & 1));
}

template <int N> __device__ __forceinline__ uint32_t byte_of(const uint32_t (&v)[N], int i)
{
    return (v[i >> 2] >> (8 * (i & 3))) & 255u;
}

// 2 * kHalfPx source pixels of one row, as dwords
template <int CN> __device__ __forceinline__ void load_row(const uint8_t* p, uint32_t (&v)[2 * CN])
{
    if constexpr (CN == 1) {
        const u32x2 a = __builtin_nontemporal_load(reinterpret_cast<const u32x2_a4*>(p));
        v[0] = a[0], v[1] = a[1];
    } else {
        const u32x4 a = __builtin_nontemporal_load(reinterpret_cast<const u32x4_a4*>(p));
        const u32x2 b = __builtin_nontemporal_load(reinterpret_cast<const u32x2_a4*>(p + 16));
        v[0] = a[0], v[1] = a[1], v[2] = a[2], v[3] = a[3], v[4] = b[0], v[5] = b[1];
    }
}

}  // namespace

// grid (ceil(dw / kHalfWgPx), ceil(dh / kHalfRows), batch), 256 threads
template <int CN, bool VEC> __global__ __launch_bounds__(256) void k_half(HalfArgs a)
{
    const int dx0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * kHalfPx;
    if (dx0 >= a.dw) return;
    const uint8_t* __restrict__ src = a.src + (size_t)blockIdx.z * a.frame_stride;
    uint8_t* __restrict__ dst = a.dst + (size_t)blockIdx.z * a.dst_frame_stride;
    const int dy0 = (int)blockIdx.y * kHalfRows;
    // all kHalfPx cells of the lane are full in x, and its 2 * kHalfPx source pixels exist
    const bool wide = VEC && 2 * (dx0 + kHalfPx) <= a.w;
    uint32_t top[kHalfRows][2 * CN], bot[kHalfRows][2 * CN];
    if (wide) {   // every full row's loads first, so that they are all in flight together
#pragma unroll
        for (int r = 0; r < kHalfRows; r++) {
            const int dy = dy0 + r;
            if (dy < a.dh && 2 * dy + 1 < a.h) {
                const uint8_t* p = src + (size_t)(2 * dy) * a.stride + (size_t)(2 * dx0) * CN;
                load_row<CN>(p, top[r]);
                load_row<CN>(p + a.stride, bot[r]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kHalfRows; r++) {
        const int dy = dy0 + r;
        if (dy >= a.dh) break;
        uint8_t* o = dst + (size_t)dy * a.dst_stride + (size_t)dx0 * CN;
        if (wide && 2 * dy + 1 < a.h) {
            uint32_t out[CN] = {};
#pragma unroll
            for (int j = 0; j < kHalfPx * CN; j++) {
                const int i = 2 * (j / CN) * CN + j % CN;   // the cell's left pixel, channel j % CN
                const uint32_t s = byte_of(top[r], i) + byte_of(top[r], i + CN) + byte_of(bot[r], i) + byte_of(bot[r], i + CN);
                out[j >> 2] |= ((s + 2) >> 2) << (8 * (j & 3));
            }
            if constexpr (CN == 1) {
                __builtin_nontemporal_store(out[0], reinterpret_cast<uint32_t*>(o));
            } else {
                const u32x2 lo = {out[0], out[1]};
                __builtin_nontemporal_store(lo, reinterpret_cast<u32x2_a4*>(o));
                __builtin_nontemporal_store(out[2], reinterpret_cast<uint32_t*>(o + 8));
            }
        } else {
            for (int px = 0; px < kHalfPx && dx0 + px < a.dw; px++)
                for (int c = 0; c < CN; c++) o[px * CN + c] = half_cell(src, a.stride, a.w, a.h, CN, dx0 + px, dy, c);
        }
    }
}

bool half_vector_path(int batch, const void* src, int stride, size_t frame_stride, const void* dst, int dst_stride,
                      size_t dst_frame_stride)
{
    size_t m = (size_t)(uintptr_t)src | (size_t)stride | (size_t)(uintptr_t)dst | (size_t)dst_stride;
    if (batch > 1) m |= frame_stride | dst_frame_stride;
    return (m & 3) == 0;
}

hipError_t launch_half(hipStream_t s, int batch, const uint8_t* src, int w, int h, int stride, size_t frame_stride,
                       int channels, uint8_t* dst, int dst_stride, size_t dst_frame_stride)
{
    int dw = 0, dh = 0;
    if (mdx_half_size(w, h, &dw, &dh) != MDX_OK || (channels != 1 && channels != 3) || batch < 1)
        return hipErrorInvalidValue;
    for (int b0 = 0; b0 < batch; b0 += kHalfMaxBatch) {
        const int nb = std::min(kHalfMaxBatch, batch - b0);
        const HalfArgs a{src + (size_t)b0 * frame_stride, dst + (size_t)b0 * dst_frame_stride, w, h, dw, dh,
                         stride, dst_stride, frame_stride, dst_frame_stride};
        const dim3 grid((dw + kHalfWgPx - 1) / kHalfWgPx, (dh + kHalfRows - 1) / kHalfRows, nb);
        const bool vec = half_vector_path(nb, a.src, stride, frame_stride, a.dst, dst_stride, dst_frame_stride);
        if (channels == 1) {
            if (vec) hipLaunchKernelGGL((k_half<1, true>), grid, dim3(256), 0, s, a);
            else hipLaunchKernelGGL((k_half<1, false>), grid, dim3(256), 0, s, a);
        } else {
            if (vec) hipLaunchKernelGGL((k_half<3, true>), grid, dim3(256), 0, s, a);
            else hipLaunchKernelGGL((k_half<3, false>), grid, dim3(256), 0, s, a);
        }
        if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace mdx
