// mdx_front.hip -- front-end kernels of the flow path and their launchers.
//
// Reference path: OpticalFlowCalculator::calculateOpticalFlow
// (common/src/optical_flow_calculator.cpp:30-130).
// Every kernel reproduces the arithmetic of the OpenCV 2.4 routine the reference calls, bit for bit
// (integer stages exactly; float and double stages in the same evaluation order, compiled with
// -ffp-contract=off so no expression is fused into an FMA).
//   A1-A4   k_front          cvtColor(BGR2GRAY) + level-0 REFLECT_101 padding + pyrDown to level 1
//                            in one pass; in level mode pyrDown L -> L+1 for the coarser levels
//   A1      k_gray_pad       gray + level-0 padding alone (single-level pyramids)
//   A3      k_scharr         calcSharrDeriv + CONSTANT-0 padding (prev frame); k_scharr_levels: every
//                            level in one launch
//           k_gray_rows      row bands: the frame-1 gray rows a band's warp reads
#include "mdx_dev.h"

#include <algorithm>

namespace mdx {

// ------------------------------------------------------------------ A1: gray + pad
// color.cpp RGB2Gray<uchar> with blueIdx 0 on rgb8 data (node.cpp:271 then :50):
// gray = (R*1868 + G*9617 + B*4899 + 8192) >> 14.  mono8 passes through unchanged.
// grid: x -> pairs of adjacent 16-B chunks of the padded row, y -> padded row, z = 2*pair + which
// frame.  Both of a thread's loads are in flight before its first store: 0.146 ms per step
// against 0.158 with one chunk per thread (4 adjacent chunks: 0.247; chunks interleaved across
// lanes so each load instruction is 1 KiB contiguous: 0.164-0.171).
__global__ __launch_bounds__(256) void k_gray_pad(const uint8_t* __restrict__ in1, const uint8_t* __restrict__ in2,
                                                  int w, int h, int stride, long long frame_stride, int fmt,
                                                  uint8_t* __restrict__ pyr1, uint8_t* __restrict__ pyr2,
                                                  long long img_bytes, Level L, int nchunk, int fsel)
{
    const int which = fsel ? fsel - 1 : blockIdx.z & 1, pair = fsel ? blockIdx.z : blockIdx.z >> 1;
    const int c = 2 * (blockIdx.x * blockDim.x + threadIdx.x) + 1;   // chunk 0 is all margin
    const int py = blockIdx.y - kPad;
    if (c > nchunk) return;
    const uint8_t* src = (which ? in2 : in1) + (long long)pair * frame_stride;
    const uint8_t* s = src + (long long)r101(py, h) * stride;
    uint32_t o0[4], o1[4];
    gray_chunk(s, 16 * c - kXOff, w, fmt, o0);
    const bool two = c + 1 <= nchunk;
    if (two) gray_chunk(s, 16 * (c + 1) - kXOff, w, fmt, o1);
    uint8_t* row = (which ? pyr2 : pyr1) + (long long)pair * img_bytes + L.img_off + (long long)(py + kPad) * L.pitch;
    *reinterpret_cast<uint4*>(row + 16 * c) = make_uint4(o0[0], o0[1], o0[2], o0[3]);
    if (two) *reinterpret_cast<uint4*>(row + 16 * (c + 1)) = make_uint4(o1[0], o1[1], o1[2], o1[3]);
}

// ------------------------------------------------------------------ A1 + A3/A4: k_front
// buildOpticalFlowPyramid's images (lkpyramid.cpp, called at optical_flow_calculator.cpp:71):
// pyramids.cpp pyrDown_<FixPtCast<uchar,8>>: dst(x,y) = (sum_ij k_i k_j src(r101(2y+i-2),
// r101(2x+j-2)) + 128) >> 8, k = [1 4 6 4 1], on the source ROI's own size; every level carries a
// 40-px REFLECT_101 border of its own core (copyMakeBorder ... BORDER_REFLECT_101|BORDER_ISOLATED).
//
// Frame mode (MODE 0/1): gray + level-0 padding + level 1 in one pass.  A workgroup owns RB level-1
// core rows [Y0, Y0+RB) and the level-0 core rows [2 Y0, 2 Y0 + 2 RB):
//   1  stage level-0 padded rows 2 Y0 - 2 .. 2 Y0 + 2 RB (reflect-101 in both directions, gray of
//      rgb8 on the fly) in LDS: interior 16-B chunks by LDS-DMA (mono8; rgb8/bgr8 by vector loads,
//      K per thread in flight, and the gray conversion), the border bytes one per lane;
//   2  write the band's level-0 rows, and every border row that mirrors one of them, from LDS;
//   3a level-1 core rows into an LDS row buffer: a thread owns 4 level-1 columns and walks down
//      the band, each staged row's horizontal 5-tap sums (two chained v_dot4_u32_u8 per pixel)
//      computed once and reused by the up to three level-1 rows whose vertical window covers it;
//   3a' the row buffer's reflect-101 column borders, one byte per lane;
//   3b level-1 padded rows (and mirrored border rows) out, 16 B per lane.
// Level 0 thus crosses HBM once (written) instead of three times (written, read back by a
// separate pyrDown); source halo rows are shared with the neighbouring band through L2
// (consecutive bands go to the same XCD).  Level mode (MODE 2) runs the same band schedule from
// an already padded level to the next (phase 1 = LDS-DMA copies of the padded source rows, no
// phase 2).  Measured at 1080p x 32, one frame side (scripts/micro/front_bench.hip): levels 0-1
// 40 us (4.0 TB/s of 162 MB) and levels 2-4 20 us, against 107 + 42 us for the earlier
// k_gray_pad + per-level pyrDown kernels (44 + 30 us with vector loads instead of LDS-DMA).  Per-pixel reflect-101 gathers in the hot loops cost
// ~2-5 us per workgroup (measured): borders are built byte-per-lane from data already in LDS.
struct FrontArgs {
    const uint8_t* in1;
    const uint8_t* in2;
    int w, h, stride, fmt, fsel, nbands, nz;
    int band0;       // first band of the launch (row-band mode builds only the bands a band's LK reads)
    long long frame_stride, img_bytes;
    uint8_t* pyr1;
    uint8_t* pyr2;
    Level L0, L1;
    int nchunk0;     // last 16-B chunk of a level-0 row (chunk 0 is margin)
    int nchunk1_16;  // last 16-B chunk of a level-1 row (chunk 0 is margin)
    int aligned;     // every source row starts 4-B aligned (interior chunks take vector loads)
    int lp;          // LDS bytes per staged level-0 row (16 * (nchunk0 + 1))
    int lp1;         // LDS bytes per level-1 row of the row buffer (16 * (nchunk1_16 + 1))
};

// borderInterpolate(p, len, BORDER_REFLECT_101) for -len < p < 2 len - 1 (one fold), branch-free.
// k_front only runs when level 1 exists, i.e. w, h >= 81 and the level-1 sizes are >= 41, so
// every index it folds (at most 40 outside a row or column range) needs at most one fold.
__device__ __forceinline__ int r101s(int p, int len)
{
    const int q = p < 0 ? -p : p;
    return q >= len ? 2 * len - 2 - q : q;
}

__device__ __forceinline__ int fdiv(int a, int b, float rb)
{
    // a / b for 0 <= a < 2^20 (b > 0): float estimate, corrected
    int q = (int)((float)a * rb);
    if (q * b > a) q--;
    else if ((q + 1) * b <= a) q++;
    return q;
}

typedef __attribute__((address_space(3))) void* front_lds_ptr;

// MODE 0: mono8 frames, 1: rgb8/bgr8 frames (gray + pad + level 1, as above); MODE 2: one
// pyramid level L -> L+1 (a.L0 = source level, already padded in the slab, a.L1 = destination):
// the staged rows are plain 16-B copies of the padded source rows and phase 2 is skipped.
template <int RB, int MODE, int KM = 8>
__global__ __launch_bounds__(256) void k_front(FrontArgs a)
{
    constexpr bool COLOR = MODE == 1, FRAME = MODE != 2;
    constexpr int NR = 2 * RB + 3, K = COLOR ? 2 : KM, VW = COLOR ? 12 : 4, MAXOUT0 = 2 * RB + 80, MAXOUT1 = RB + 80;
    extern __shared__ uint32_t front_lds[];
    __shared__ int out0[MAXOUT0], out1[MAXOUT1], nout[2];
    uint8_t* lds = reinterpret_cast<uint8_t*>(front_lds);
    const int tid = threadIdx.x;

    // XCD-aware order: consecutive bands of a frame go to the same XCD (8 dispatch round-robin)
    const int nb = gridDim.x;
    int task = blockIdx.x;
    if ((nb & 7) == 0) task = (blockIdx.x & 7) * (nb >> 3) + (blockIdx.x >> 3);
    const int band = a.band0 + task % a.nbands, z = task / a.nbands;
    const int which = a.fsel ? a.fsel - 1 : z & 1, pair = a.fsel ? z : z >> 1;
    const int w = a.w, h = a.h, w1 = a.L1.w, h1 = a.L1.h;
    const int Y0 = band * RB, e1 = min(Y0 + RB, h1), r0 = 2 * Y0, e0 = min(2 * Y0 + 2 * RB, h);
    const int fmt = a.fmt;
    const uint8_t* src = (which ? a.in2 : a.in1) + (long long)pair * a.frame_stride;
    uint8_t* slab = (which ? a.pyr2 : a.pyr1) + (long long)pair * a.img_bytes;

    // rows this band writes: level 0 padded rows whose core row is in [r0, e0), level 1 in [Y0, e1)
    if (tid < 2) nout[tid] = 0;
    __syncthreads();
    if (FRAME && tid < 80) {
        const int py = tid < 40 ? tid - 40 : h + tid - 40;
        const int r = r101s(py, h);
        if (r >= r0 && r < e0) out0[atomicAdd(&nout[0], 1)] = py;
    } else if (tid >= 128 && tid < 208) {
        const int t = tid - 128;
        const int py = t < 40 ? t - 40 : h1 + t - 40;
        const int r = r101s(py, h1);
        if (r >= Y0 && r < e1) out1[atomicAdd(&nout[1], 1)] = py;
    }
    __syncthreads();
    const int nb0 = nout[0], nb1 = nout[1];
    __syncthreads();
    if (FRAME && tid < e0 - r0) out0[nb0 + tid] = r0 + tid;
    if (tid >= 128 && tid - 128 < e1 - Y0) out1[nb1 + tid - 128] = Y0 + tid - 128;

    // phase 1: level-0 padded rows r0-2 .. r0+2RB into LDS (chunks 1 .. nchunk0).  Interior chunks
    // [cA, cB] (inside the source row, every row 4-B aligned per the host) take plain 16-B (mono8)
    // or 48-B (rgb8/bgr8) loads, K per thread in flight; the few border chunks go through the
    // per-pixel reflect-101 path in a loop of their own.
    const int nc0 = a.nchunk0;
    const int cA = kXOff / 16;
    int cB = a.aligned ? (w + kXOff - 16) / 16 : cA - 1;
    if (cB < cA) cB = cA - 1;
    const int ni = cB - cA + 1;
    if constexpr (MODE != 1) {
        // mono8 frames and level mode: LDS-DMA (buffer_load ... lds) straight into the staged rows.
        // Flat 16-B slot f is row f / (nc0 + 1), chunk f % (nc0 + 1) (LDS byte 16 f); one wave
        // instruction fills 64 consecutive slots.  Frame mode loads the interior chunks [cA, cB]
        // and leaves the rest to the border-byte pass below (an out-of-range offset lands zeros
        // there first); level mode copies whole padded rows.
        const int spr = nc0 + 1, nslot = NR * spr;
        const float rs = 1.f / (float)spr;
        const uint8_t* rbase = FRAME ? src : slab + a.L0.img_off;
        // a mono8 frame ends with its last row's w pixels (a pitched view owns no byte past them)
        const long long rbytes = FRAME ? (long long)(h - 1) * a.stride + w : (long long)a.L0.rows * a.L0.pitch;
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint8_t*>(rbase), (short)0, (int)min(rbytes, (long long)0x7fffffff), 0x00020000);
        const int wave = tid >> 6, wl = tid & 63;
        for (int b0 = 64 * wave; b0 < nslot; b0 += 256) {
            const int f = b0 + wl;
            if (f < nslot) {
                const int i = fdiv(f, spr, rs), c = f - i * spr;
                uint32_t off = 0x80000000u;
                if constexpr (FRAME) {
                    if (c >= cA && c <= cB) off = (uint32_t)(r101s(r0 - 2 + i, h) * a.stride + 16 * c - kXOff);
                } else {
                    off = (uint32_t)((r0 - 2 + i + kPad) * a.L0.pitch + 16 * c);
                }
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (front_lds_ptr)(lds + 16 * b0), 16, (int)off, 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(0x0F70);               // vmcnt(0): this wave's DMA has landed
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (FRAME) __syncthreads();             // before any wave rewrites border slots
    }
    if (MODE == 1 && ni > 0) {
        const float rci = 1.f / (float)ni;
        const int n1 = NR * ni;
        for (int base = 0; base < n1; base += 256 * K) {
            uint32_t v[K][VW];
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int item = base + k * 256 + tid;
                if (item < n1) {
                    const int i = fdiv(item, ni, rci), c = cA + item - i * ni;
                    const uint8_t* s = src + (long long)r101s(r0 - 2 + i, h) * a.stride + (16 * c - kXOff) * (COLOR ? 3 : 1);
                    const u4a4k* q = reinterpret_cast<const u4a4k*>(s);
                    const u4a4k t0 = q[0];
                    v[k][0] = t0.x; v[k][1] = t0.y; v[k][2] = t0.z; v[k][3] = t0.w;
                    if constexpr (COLOR) {
                        const u4a4k t1 = q[1], t2 = q[2];
                        v[k][4] = t1.x; v[k][5] = t1.y; v[k][6] = t1.z; v[k][7] = t1.w;
                        v[k][8] = t2.x; v[k][9] = t2.y; v[k][10] = t2.z; v[k][11] = t2.w;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int item = base + k * 256 + tid;
                if (item >= n1) continue;
                const int i = fdiv(item, ni, rci), c = cA + item - i * ni;
                uint32_t o[4] = {v[k][0], v[k][1], v[k][2], v[k][3]};
                if constexpr (COLOR) {
                    const uint8_t* bb = reinterpret_cast<const uint8_t*>(v[k]);
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        uint32_t d = 0;
#pragma unroll
                        for (int j = 0; j < 4; j++) d |= (uint32_t)gray_of(bb + 3 * (4 * t + j), fmt) << (8 * j);
                        o[t] = d;
                    }
                }
                *reinterpret_cast<uint4*>(lds + i * a.lp + 16 * c) = make_uint4(o[0], o[1], o[2], o[3]);
            }
        }
    }
    if constexpr (FRAME) {
        // border bytes one per lane: columns -48 .. 16 cA - 65 and 16 (cB + 1) - 64 .. 16 nc0 - 49
        const int nl = 16 * (cA - 1), nb = nl + 16 * (nc0 - cB);
        const float rcb = 1.f / (float)nb;
#pragma unroll 4
        for (int item = tid; item < NR * nb; item += 256) {
            const int i = fdiv(item, nb, rcb), e = item - i * nb;
            const int x = e < nl ? e - 48 : 16 * (cB + 1) - kXOff + (e - nl);
            const bool in = x >= -kPad && x < w + kPad;                     // row margin: left 0
            const uint8_t* sp = src + (long long)r101s(r0 - 2 + i, h) * a.stride;
            const int sx = in ? r101s(x, w) : 0;
            uint32_t v;
            if constexpr (COLOR) v = (uint32_t)gray_of(sp + 3 * sx, fmt);
            else v = sp[sx];
            lds[i * a.lp + kXOff + x] = (uint8_t)(in ? v : 0u);
        }
    }
    __syncthreads();

    // phase 2: level-0 rows out of LDS (core row r sits at LDS row r - r0 + 2)
    if constexpr (FRAME) {
        const int n0 = nb0 + (e0 - r0), n2 = n0 * nc0;
        const float rc0 = 1.f / (float)nc0;
        uint8_t* base0 = slab + a.L0.img_off;
        for (int item = tid; item < n2; item += 256) {
            const int j = fdiv(item, nc0, rc0), c = 1 + item - j * nc0;
            const int py = out0[j];
            const int i = r101s(py, h) - r0 + 2;
            *reinterpret_cast<uint4*>(base0 + (long long)(py + kPad) * a.L0.pitch + 16 * c) =
                *reinterpret_cast<const uint4*>(lds + i * a.lp + 16 * c);
        }
    }

    // phase 3a: the band's level-1 core rows into an LDS row buffer.  A thread owns one dword
    // chunk (4 level-1 pixels) of every row and walks down the band: each staged level-0 row's
    // horizontal 5-tap sums (two chained v_dot4_u32_u8 per pixel) are computed once and kept in
    // registers for the up to three level-1 rows whose vertical window covers it.
    uint8_t* l1buf = lds + NR * a.lp;
    {
        const int nq = (w1 + 3) >> 2;
        for (int q = tid; q < nq; q += 256) {
            const int px0 = 4 * q;
            const uint8_t* col = lds + kXOff + 2 * px0 - 4;      // level-0 columns 2 px0 - 4 .. 2 px0 + 11
            uint32_t hr[5][4];
            auto hsum = [&](int r, uint32_t (&o)[4]) {
                const uint32_t* p = reinterpret_cast<const uint32_t*>(col + r * a.lp);
                const uint32_t wd[4] = {p[0], p[1], p[2], p[3]};
#pragma unroll
                for (int jj = 0; jj < 4; jj++) {
                    const int b0 = 2 * jj + 2, qq = b0 >> 2;
                    const uint32_t lo = (b0 & 3) ? __builtin_amdgcn_alignbit(wd[qq + 1], wd[qq], 16) : wd[qq];
                    const uint32_t hi = (b0 & 3) ? (wd[qq + 1] >> 16) : wd[qq + 1];
                    o[jj] = __builtin_amdgcn_udot4(hi, 1u, __builtin_amdgcn_udot4(lo, 0x04060401u, 0u, false), false);
                }
            };
            hsum(0, hr[0]);
            hsum(1, hr[1]);
            hsum(2, hr[2]);
#pragma unroll
            for (int yy = 0; yy < RB; yy++) {
                if (Y0 + yy >= e1) break;
                hsum(2 * yy + 3, hr[3]);
                hsum(2 * yy + 4, hr[4]);
                uint32_t o = 0;
#pragma unroll
                for (int jj = 0; jj < 4; jj++) {
                    const uint32_t acc = hr[0][jj] + hr[1][jj] * 4u + hr[2][jj] * 6u + hr[3][jj] * 4u + hr[4][jj];
                    o |= ((acc + 128) >> 8) << (8 * jj);
                }
                *reinterpret_cast<uint32_t*>(l1buf + yy * a.lp1 + kXOff + px0) = o;
#pragma unroll
                for (int jj = 0; jj < 4; jj++) {
                    hr[0][jj] = hr[2][jj];
                    hr[1][jj] = hr[3][jj];
                    hr[2][jj] = hr[4][jj];
                }
            }
        }
    }
    __syncthreads();
    // phase 3a': the row buffer's reflect-101 borders (and zeroed margins), one byte per lane
    {
        const int nl = 48, nb = nl + 16 * (a.nchunk1_16 + 1) - kXOff - w1;   // columns -48..-1, w1..
        const float rcb = 1.f / (float)nb;
        const int nrow = e1 - Y0;
        for (int item = tid; item < nrow * nb; item += 256) {
            const int i = fdiv(item, nb, rcb), e = item - i * nb;
            const int x = e < nl ? e - 48 : w1 + (e - nl);
            const bool in = x >= -kPad && x < w1 + kPad;
            uint8_t* row = l1buf + i * a.lp1 + kXOff;
            const uint8_t v = row[in ? r101s(x, w1) : 0];
            row[x] = in ? v : (uint8_t)0;
        }
    }
    __syncthreads();

    // phase 3b: level-1 padded rows out of the row buffer, 16 B per lane (borders by reflect-101
    // in LDS; bytes 16..23 of a row are margin, written with zeros)
    {
        const int nc16 = a.nchunk1_16;                                // 16-B chunks 1 .. nc16
        const float rc16 = 1.f / (float)nc16;
        const int n3 = (nb1 + (e1 - Y0)) * nc16;
        uint8_t* base1 = slab + a.L1.img_off;
        for (int item = tid; item < n3; item += 256) {
            const int j = fdiv(item, nc16, rc16), c = 1 + item - j * nc16;
            const int py = out1[j];
            const uint8_t* row = l1buf + (r101s(py, h1) - Y0) * a.lp1 + kXOff;
            const int px0 = 16 * c - kXOff;
            const uint4 o = *reinterpret_cast<const uint4*>(row + px0);
            *reinterpret_cast<uint4*>(base1 + (long long)(py + kPad) * a.L1.pitch + 16 * c) = o;
        }
    }
}

// ------------------------------------------------------------------ A3: Scharr derivs
// lkpyramid.cpp calcSharrDeriv.  Vertical t0 = 3(a+c)+10b, t1 = c-a; horizontal
// Ix = t0[x+1]-t0[x-1], Iy = 3(t1[x-1]+t1[x+1])+10 t1[x].  OpenCV clamps the row/col
// neighbours as reflect-101 (row -1 -> 1, col cols -> cols-2), which is exactly the padded
// level's border, so the stencil reads the padded image directly.  Border = 0
// (copyMakeBorder ... BORDER_CONSTANT).  Per thread 4 pixels (one 16-B store); each of the
// three source rows is one dwordx3 load of bytes x0-4 .. x0+7.
__global__ __launch_bounds__(256) void k_scharr(const uint8_t* __restrict__ pyr1, uint32_t* __restrict__ der,
                                                long long img_bytes, long long der_words, Level L, int nchunk,
                                                int prow0)
{
    const int pair = blockIdx.z;
    const int c = blockIdx.x * blockDim.x + threadIdx.x + 4;         // word chunks 0..3 are margin
    const int py = prow0 + blockIdx.y - kPad;                        // padded rows prow0 + blockIdx.y
    if (c > nchunk) return;
    const int px0 = 4 * c - kXOff;
    uint32_t o[4] = {0, 0, 0, 0};
    if (py >= 0 && py < L.h && px0 + 4 > 0 && px0 < L.w) {
        const uint8_t* s = pyr1 + (long long)pair * img_bytes + L.img_off + L.core() + (long long)py * L.pitch + px0 - 4;
        const int p = L.pitch;
        uint32_t rw[3][3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const u3a4k v = *reinterpret_cast<const u3a4k*>(s + (long long)(r - 1) * p);
            rw[r][0] = v.x; rw[r][1] = v.y; rw[r][2] = v.z;
        }
        auto B = [&](int r, int b) -> int { return (int)((rw[r][b >> 2] >> (8 * (b & 3))) & 255u); };
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int px = px0 + i;
            if (px < 0 || px >= L.w) continue;
            const int bm = 3 + i, bc = 4 + i, bp = 5 + i;               // bytes x-1, x, x+1
            const int t0m = (B(0, bm) + B(2, bm)) * 3 + B(1, bm) * 10;
            const int t0p = (B(0, bp) + B(2, bp)) * 3 + B(1, bp) * 10;
            const int t1m = B(2, bm) - B(0, bm), t1c = B(2, bc) - B(0, bc), t1p = B(2, bp) - B(0, bp);
            const int ix = t0p - t0m;
            const int iy = (t1m + t1p) * 3 + t1c * 10;
            o[i] = (uint32_t)(uint16_t)(int16_t)ix | ((uint32_t)(uint16_t)(int16_t)iy << 16);
        }
    }
    uint32_t* row = der + (long long)pair * der_words + L.der_off + (long long)(py + kPad) * L.pitch;
    *reinterpret_cast<uint4*>(row + 4 * c) = make_uint4(o[0], o[1], o[2], o[3]);
}

// Rows [fit->src_y0, fit->src_y1) of frame 1 -> gray, into the padded level-0 core (what k_front
// writes there): block (bx, by) converts 256 columns of rows src_y0 + by, + gridDim.y, ...
__global__ __launch_bounds__(64) void k_gray_rows(const uint8_t* __restrict__ img1, int w, int stride, int fmt,
                                                  uint8_t* __restrict__ g, int pitch, const PairFit* __restrict__ fit,
                                                  int built0, int built1)
{
    const int r0 = fit->src_y0, r1 = fit->src_y1;
    const int x = (blockIdx.x * 64 + threadIdx.x) * 4;
    if (x >= w) return;
    for (int y = r0 + (int)blockIdx.y; y < r1; y += gridDim.y) {
        if (y >= built0 && y < built1) continue;   // the band's flow built these rows

        const uint8_t* sp = img1 + (long long)y * stride;
        uint8_t* dp = g + (long long)y * pitch + x;
        const int n = min(4, w - x);
        uint32_t d = 0;
        for (int i = 0; i < n; i++) {
            const int v = fmt == 0 ? sp[x + i] : gray_of(sp + 3 * (x + i), fmt);
            d |= (uint32_t)v << (8 * i);
        }
        if (n == 4) *reinterpret_cast<uint32_t*>(dp) = d;   // x and the core are 4-B aligned
        else for (int i = 0; i < n; i++) dp[i] = (uint8_t)(d >> (8 * i));
    }
}

hipError_t launch_gray_rows(hipStream_t s, const uint8_t* img1, int w, int h, int stride, int fmt, uint8_t* gray1_l0,
                            int pitch, const PairFit* fit, int built0, int built1)
{
    (void)h;
    const dim3 grid((w + 255) / 256, 64);
    hipLaunchKernelGGL(k_gray_rows, grid, dim3(64), 0, s, img1, w, stride, fmt, gray1_l0, pitch, fit, built0, built1);
    return hipGetLastError();
}

// ------------------------------------------------------------------ launchers
// last 16-B chunk index of a padded row (columns -40 .. w+39 at row bytes 24 .. 64+w+39)
static inline int last_chunk16(int w) { return (kXOff + w + kPad - 1) / 16; }

hipError_t launch_gray_pad(hipStream_t s, int batch, const uint8_t* in1, const uint8_t* in2, int w, int h, int stride,
                           long long frame_stride, int fmt, uint8_t* pyr1, uint8_t* pyr2, const Geometry& g, int fsel)
{
    const int nchunk = last_chunk16(w);
    const dim3 grid((nchunk + 127) / 128, h + 2 * kPad, fsel ? batch : 2 * batch);   // two chunks per thread
    hipLaunchKernelGGL(k_gray_pad, grid, dim3(64), 0, s, in1, in2, w, h, stride, frame_stride, fmt, pyr1, pyr2,
                       g.img_bytes, g.lv[0], nchunk, fsel);
    return hipGetLastError();
}

// k_front's band height: 4 destination rows at 1080p (27 KB of LDS, 5-6 bands per CU): one frame
// side of gray + pad + level 1 takes 44 us there against 56 with 8 rows and 107 for the earlier
// k_gray_pad + k_pyrdown (scripts/micro/front_bench.hip).
static hipError_t launch_front_bands(hipStream_t s, FrontArgs& a, int mode, int rlo = 0, int rhi = -1)
{
    // the band height: 4 destination rows while a band's LDS fits 32 KB, else 2 (8K frames: 62 KB),
    // else 1; beyond 64 KB (rows wider than ~8.7K px at RB = 1) the launch asks for the larger
    // dynamic LDS explicitly (up to the CU's 160 KB)
    auto lds_of = [&](int rb) { return (size_t)(2 * rb + 3) * a.lp + (size_t)rb * a.lp1; };
    int rb = lds_of(4) <= 32 * 1024 ? 4 : lds_of(2) <= 64 * 1024 ? 2 : 1;
    // a single frame (the live ring's push): 4-row bands are a few hundred workgroups, under two
    // per CU; one-row bands re-read more source rows (5 per destination row against 2.75) but
    // spread the frame over the chip
    if (rb == 4 && (long long)a.nz * ((a.L1.h + 3) / 4) < 512) rb = 1;
    const size_t lds = lds_of(rb);
    // k_front's static arrays (out0, out1, nout) share the CU's 160 KB with the dynamic rows
    const size_t lds_static = (size_t)(2 * rb + 80 + rb + 80 + 2) * sizeof(int);
    if (lds + lds_static > 160 * 1024) return hipErrorInvalidValue;   // rows wider than ~31K px
    // destination rows [rlo, rhi) of the level built (all by default): the bands covering them
    if (rhi < 0 || rhi > a.L1.h) rhi = a.L1.h;
    rlo = std::max(0, std::min(rlo, rhi));
    a.band0 = rlo / rb;
    a.nbands = (rhi + rb - 1) / rb - a.band0;
    if (a.nbands <= 0) return hipSuccess;
    const dim3 grid((unsigned)(a.nbands * a.nz));
#define MDX_FRONT_CASE(M, R)                                                                             \
    if (mode == M && rb == R) {                                                                          \
        if (lds + lds_static > 64 * 1024)                                                                \
            if (hipError_t e = hipFuncSetAttribute((const void*)k_front<R, M>,                           \
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) \
                return e;                                                                                \
        hipLaunchKernelGGL((k_front<R, M>), grid, dim3(256), lds, s, a);                                 \
    }
    MDX_FRONT_CASE(0, 4) MDX_FRONT_CASE(0, 2) MDX_FRONT_CASE(0, 1)
    MDX_FRONT_CASE(1, 4) MDX_FRONT_CASE(1, 2) MDX_FRONT_CASE(1, 1)
    MDX_FRONT_CASE(2, 4) MDX_FRONT_CASE(2, 2) MDX_FRONT_CASE(2, 1)
#undef MDX_FRONT_CASE
    return hipGetLastError();
}

static FrontArgs front_args(int batch, uint8_t* pyr1, uint8_t* pyr2, const Geometry& g, int src_level, int fsel)
{
    FrontArgs a{};
    a.fsel = fsel;
    a.img_bytes = g.img_bytes;
    a.pyr1 = pyr1;
    a.pyr2 = pyr2;
    a.L0 = g.lv[src_level];
    a.L1 = g.lv[src_level + 1];
    a.w = a.L0.w;
    a.h = a.L0.h;
    a.nchunk0 = last_chunk16(a.L0.w);
    a.nchunk1_16 = last_chunk16(a.L1.w);
    a.lp = 16 * (a.nchunk0 + 1);
    a.lp1 = 16 * (a.nchunk1_16 + 1);
    a.nz = fsel ? batch : 2 * batch;
    return a;
}

hipError_t launch_front(hipStream_t s, int batch, const uint8_t* in1, const uint8_t* in2, int w, int h, int stride,
                        long long frame_stride, int fmt, uint8_t* pyr1, uint8_t* pyr2, const Geometry& g, int fsel,
                        const RowSpan* rows)
{
    if (g.nlev < 2) return launch_gray_pad(s, batch, in1, in2, w, h, stride, frame_stride, fmt, pyr1, pyr2, g, fsel);
    FrontArgs a = front_args(batch, pyr1, pyr2, g, 0, fsel);
    a.in1 = in1;
    a.in2 = in2;
    a.stride = stride;
    a.fmt = fmt;
    a.frame_stride = frame_stride;
    a.aligned = ((((uintptr_t)in1 | (uintptr_t)in2) & 3) == 0 && (stride & 3) == 0 && (frame_stride & 3) == 0) ? 1 : 0;
    // level-1 rows: those wanted at level 1 and those whose bands write the wanted level-0 rows
    int r1lo = 0, r1hi = -1;
    if (rows) {
        r1lo = std::min(rows[1].lo, rows[0].lo / 2);
        r1hi = std::max(rows[1].hi, (rows[0].hi + 1) / 2);
    }
    return launch_front_bands(s, a, fmt == MDX_FMT_GRAY8 ? 0 : 1, r1lo, r1hi);
}

hipError_t launch_pyr_levels(hipStream_t s, int batch, uint8_t* pyr1, uint8_t* pyr2, const Geometry& g, int fsel,
                             const RowSpan* rows)
{
    for (int l = 2; l < g.nlev; l++) {
        FrontArgs a = front_args(batch, pyr1, pyr2, g, l - 1, fsel);
        if (hipError_t e = launch_front_bands(s, a, 2, rows ? rows[l].lo : 0, rows ? rows[l].hi : -1)) return e;
    }
    return hipSuccess;
}

// Every level's Scharr planes in one launch (blockIdx.y runs over the levels' padded rows, level by
// level): the live ring's push builds one frame's five levels, whose launches are each a few
// microseconds of mostly launch overhead.
struct ScharrLevels {
    Level L[kMaxLevels];
    int nchunk[kMaxLevels];
    int row0[kMaxLevels + 1];   // first blockIdx.y of each level
    int nlev;
};
__global__ __launch_bounds__(256) void k_scharr_levels(const uint8_t* __restrict__ pyr1, uint32_t* __restrict__ der,
                                                       long long img_bytes, long long der_words, ScharrLevels sl)
{
    int l = 0;
    while (l + 1 < sl.nlev && (int)blockIdx.y >= sl.row0[l + 1]) l++;
    const Level L = sl.L[l];
    const int nchunk = sl.nchunk[l];
    const int pair = blockIdx.z;
    const int c = blockIdx.x * blockDim.x + threadIdx.x + 4;         // word chunks 0..3 are margin
    const int py = (int)blockIdx.y - sl.row0[l] - kPad;
    if (c > nchunk) return;
    const int px0 = 4 * c - kXOff;
    uint32_t o[4] = {0, 0, 0, 0};
    if (py >= 0 && py < L.h && px0 + 4 > 0 && px0 < L.w) {
        const uint8_t* s = pyr1 + (long long)pair * img_bytes + L.img_off + L.core() + (long long)py * L.pitch + px0 - 4;
        const int p = L.pitch;
        uint32_t rw[3][3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const u3a4k v = *reinterpret_cast<const u3a4k*>(s + (long long)(r - 1) * p);
            rw[r][0] = v.x; rw[r][1] = v.y; rw[r][2] = v.z;
        }
        auto B = [&](int r, int b) -> int { return (int)((rw[r][b >> 2] >> (8 * (b & 3))) & 255u); };
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int px = px0 + i;
            if (px < 0 || px >= L.w) continue;
            const int bm = 3 + i, bc = 4 + i, bp = 5 + i;               // bytes x-1, x, x+1
            const int t0m = (B(0, bm) + B(2, bm)) * 3 + B(1, bm) * 10;
            const int t0p = (B(0, bp) + B(2, bp)) * 3 + B(1, bp) * 10;
            const int t1m = B(2, bm) - B(0, bm), t1c = B(2, bc) - B(0, bc), t1p = B(2, bp) - B(0, bp);
            const int ix = t0p - t0m;
            const int iy = (t1m + t1p) * 3 + t1c * 10;
            o[i] = (uint32_t)(uint16_t)(int16_t)ix | ((uint32_t)(uint16_t)(int16_t)iy << 16);
        }
    }
    uint32_t* row = der + (long long)pair * der_words + L.der_off + (long long)(py + kPad) * L.pitch;
    *reinterpret_cast<uint4*>(row + 4 * c) = make_uint4(o[0], o[1], o[2], o[3]);
}

hipError_t launch_scharr_levels(hipStream_t s, int batch, const uint8_t* pyr1, uint32_t* der, const Geometry& g)
{
    ScharrLevels sl{};
    sl.nlev = g.nlev;
    int rows = 0, maxc = 0;
    for (int l = 0; l < g.nlev; l++) {
        sl.L[l] = g.lv[l];
        sl.nchunk[l] = (kXOff + g.lv[l].w + kPad - 1) / 4;
        sl.row0[l] = rows;
        rows += g.lv[l].rows;
        maxc = std::max(maxc, sl.nchunk[l]);
    }
    sl.row0[g.nlev] = rows;
    if (rows == 0) return hipSuccess;
    const dim3 grid((maxc - 4 + 1 + 63) / 64, rows, batch);
    hipLaunchKernelGGL(k_scharr_levels, grid, dim3(64), 0, s, pyr1, der, g.img_bytes, g.der_words, sl);
    return hipGetLastError();
}

hipError_t launch_scharr(hipStream_t s, int batch, const uint8_t* pyr1, uint32_t* der, const Geometry& g, int level,
                         int prow0, int prow1)
{
    const Level& L = g.lv[level];
    const int nchunk = (kXOff + L.w + kPad - 1) / 4;                 // last 4-word chunk
    if (prow1 < 0 || prow1 > L.rows) prow1 = L.rows;
    prow0 = std::max(0, std::min(prow0, prow1));
    if (prow1 == prow0) return hipSuccess;
    const dim3 grid((nchunk - 4 + 1 + 63) / 64, prow1 - prow0, batch);
    hipLaunchKernelGGL(k_scharr, grid, dim3(64), 0, s, pyr1, der, g.img_bytes, g.der_words, L, nchunk, prow0);
    return hipGetLastError();
}

}  // namespace mdx
