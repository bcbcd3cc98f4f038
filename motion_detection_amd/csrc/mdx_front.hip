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
// Frame modes (kFrontMono, kFrontColor): gray + level-0 padding + level 1 in one pass.  A workgroup
// owns RB level-1 core rows [Y0, Y0+RB) and the level-0 core rows [2 Y0, 2 Y0 + 2 RB); k_front's
// body is this sequence; what two steps share, and the DMA staging, are the functions above it:
//   1  stage level-0 padded rows 2 Y0 - 2 .. 2 Y0 + 2 RB (reflect-101 in both directions, gray of
//      rgb8 on the fly) in LDS: interior 16-B chunks by LDS-DMA (mono8: stage_dma; rgb8/bgr8 by
//      vector loads, K per thread in flight, and the gray conversion, in the body), the border
//      bytes one per lane (stage_border_bytes, on border_cols' column mapping);
//   2  write the band's level-0 rows, and every border row that mirrors one of them (the row list),
//      from LDS (rows_out);
//   3a level-1 core rows into an LDS row buffer (in the body): a thread owns 4 level-1 columns and
//      walks down the band, each staged row's horizontal 5-tap sums (two chained v_dot4_u32_u8 per
//      pixel) computed once and reused by the up to three level-1 rows whose vertical window covers it;
//   3a' the row buffer's reflect-101 column borders, one byte per lane (border_cols again);
//   3b level-1 padded rows (and mirrored border rows) out, 16 B per lane (rows_out again).
// Level 0 thus crosses HBM once (written) instead of three times (written, read back by a
// separate pyrDown); source halo rows are shared with the neighbouring band through L2
// (consecutive bands go to the same XCD).  Level mode (kFrontLevel) runs the same band schedule
// from an already padded level to the next (phase 1 = LDS-DMA copies of the padded source rows, no
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

// frame modes: gray + pad + level 1, as above, of mono8 or of rgb8/bgr8 frames; level mode: one pyramid level
// L -> L+1 (a.L0 = source, already padded in the slab, a.L1 = destination): staged rows are copies, no phase 2.
enum FrontMode : int { kFrontMono = 0, kFrontColor = 1, kFrontLevel = 2 };

// Row list: the padded rows py of a level of h core rows that the band owning core rows [lo, hi) writes -- first
// the border rows (py in [-40, 0) or [h, h + 40)) that mirror one of its core rows, in any order, then the core rows.
// Threads t = 0 .. 79 take one border row each and count into *n; after a barrier, threads t < hi - lo append at out + *n.
__device__ __forceinline__ void row_list_borders(int t, int h, int lo, int hi, int* out, int* n)
{
    const int py = t < kPad ? t - kPad : h + t - kPad;
    const int r = r101s(py, h);
    if (r >= lo && r < hi) out[atomicAdd(n, 1)] = py;
}
__device__ __forceinline__ void row_list_core(int t, int lo, int hi, int* out) { if (t < hi - lo) out[t] = lo + t; }

// Rows out: the n listed padded rows x 16-B chunks 1 .. nc from LDS rows (pitch lp; LDS row 0
// holds core row lrow0, a border row is read from the core row it mirrors) to the level's padded
// buffer in the slab.
__device__ __forceinline__ void rows_out(int tid, const int* list, int n, int nc, int h, int lrow0, const uint8_t* lrows,
                                         int lp, uint8_t* dst, int pitch)
{
    const float rc = 1.f / (float)nc;
    for (int item = tid; item < n * nc; item += 256) {
        const int j = fdiv(item, nc, rc), c = 1 + item - j * nc;
        const int py = list[j];
        const int i = r101s(py, h) - lrow0;
        *reinterpret_cast<uint4*>(dst + (long long)(py + kPad) * pitch + 16 * c) =
            *reinterpret_cast<const uint4*>(lrows + i * lp + 16 * c);
    }
}

// Border column mapping of the byte-per-lane passes over nrow LDS rows: item e of a row is column e - 48
// (left margin and border, -48 .. -1) or one of the nright columns from xr on (to the row's last byte).
// put(row, x, in): in = x lies inside the padded extent [-kPad, len + kPad) (else margin, which gets 0).
// UNROLL 4: the frame pass, whose source is global memory; 1 leaves the loop to the compiler (the
// row-buffer pass; "#pragma unroll 1" there costs SGPRs in the colour kernels).
template <int UNROLL, typename F>
__device__ __forceinline__ void border_cols(int tid, int nrow, int xr, int nright, int len, F&& put)
{
    const int nl = kXOff - 16, nb = nl + nright;
    const float rcb = 1.f / (float)nb;
    auto one = [&](int item) {
        const int i = fdiv(item, nb, rcb), e = item - i * nb;
        const int x = e < nl ? e - nl : xr + (e - nl);
        put(i, x, x >= -kPad && x < len + kPad);
    };
    if constexpr (UNROLL > 1) {
#pragma unroll UNROLL
        for (int item = tid; item < nrow * nb; item += 256) one(item);
    } else {
        for (int item = tid; item < nrow * nb; item += 256) one(item);
    }
}

typedef __attribute__((address_space(3))) void* front_lds_ptr;

// Staging by LDS-DMA (buffer_load ... lds) straight into the NR staged rows: mono8 frames and level
// mode.  Flat 16-B slot f is row f / (nc0 + 1), chunk f % (nc0 + 1) (LDS byte 16 f); one wave instruction
// fills 64 consecutive slots.  Frame mode loads the interior chunks [cA, cB] of the reflected source rows
// and leaves the rest to the border-byte pass (an out-of-range offset lands zeros there first); level
// mode copies whole padded rows.  rbase: the frame, or the source level's padded buffer.
template <int NR, bool FRAME>
__device__ __forceinline__ void stage_dma(const FrontArgs& a, int tid, uint8_t* lds, const uint8_t* rbase, int r0, int cA,
                                          int cB)
{
    const int spr = a.nchunk0 + 1, nslot = NR * spr;
    const float rs = 1.f / (float)spr;
    // a mono8 frame ends with its last row's w pixels (a pitched view owns no byte past them)
    const long long rbytes = FRAME ? (long long)(a.h - 1) * a.stride + a.w : (long long)a.L0.rows * a.L0.pitch;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t*>(rbase), (short)0, (int)min(rbytes, (long long)0x7fffffff), 0x00020000);
    const int wave = tid >> 6, wl = tid & 63;
    for (int b0 = 64 * wave; b0 < nslot; b0 += 256) {
        const int f = b0 + wl;
        if (f < nslot) {
            const int i = fdiv(f, spr, rs), c = f - i * spr;
            uint32_t off = 0x80000000u;
            if constexpr (FRAME) {
                if (c >= cA && c <= cB) off = (uint32_t)(r101s(r0 - 2 + i, a.h) * a.stride + 16 * c - kXOff);
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

// Staging of a frame's border bytes, one per lane: columns -48 .. -1 and 16 (cB + 1) - 64 .. of every
// staged row, from the reflected source pixel (gray of rgb8 on the fly); row margin: 0.
template <int NR, bool COLOR>
__device__ __forceinline__ void stage_border_bytes(const FrontArgs& a, int tid, uint8_t* lds, const uint8_t* src, int r0,
                                                   int cB)
{
    border_cols<4>(tid, NR, 16 * (cB + 1) - kXOff, 16 * (a.nchunk0 - cB), a.w, [&](int i, int x, bool in) {
        const uint8_t* sp = src + (long long)r101s(r0 - 2 + i, a.h) * a.stride;
        const int sx = in ? r101s(x, a.w) : 0;
        uint32_t v;
        if constexpr (COLOR) v = (uint32_t)gray_of(sp + 3 * sx, a.fmt);
        else v = sp[sx];
        lds[i * a.lp + kXOff + x] = (uint8_t)(in ? v : 0u);
    });
}

template <int RB, FrontMode MODE>
__global__ __launch_bounds__(256) void k_front(FrontArgs a)
{
    constexpr bool FRAME = MODE != kFrontLevel;
    constexpr int NR = 2 * RB + 3, MAXOUT0 = 2 * RB + 80, MAXOUT1 = RB + 80;
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
    const uint8_t* src = (which ? a.in2 : a.in1) + (long long)pair * a.frame_stride;
    uint8_t* slab = (which ? a.pyr2 : a.pyr1) + (long long)pair * a.img_bytes;

    // rows this band writes: level 0 rows of core rows [r0, e0) (threads 0 ..), level 1 of [Y0, e1) (128 ..)
    if (tid < 2) nout[tid] = 0;
    __syncthreads();
    if (FRAME && tid < 2 * kPad) row_list_borders(tid, h, r0, e0, out0, &nout[0]);
    else if (tid >= 128 && tid < 128 + 2 * kPad) row_list_borders(tid - 128, h1, Y0, e1, out1, &nout[1]);
    __syncthreads();
    const int nb0 = nout[0], nb1 = nout[1];
    __syncthreads();
    if constexpr (FRAME) row_list_core(tid, r0, e0, out0 + nb0);
    if (tid >= 128) row_list_core(tid - 128, Y0, e1, out1 + nb1);

    // phase 1: level-0 padded rows r0-2 .. r0+2RB into LDS (chunks 1 .. nchunk0).  Interior chunks [cA, cB]
    // (inside the source row, every row 4-B aligned per the host) by LDS-DMA (mono8) or 48-B loads (rgb8/bgr8);
    // the few border chunks per pixel, reflect-101, in a pass of their own.  Level mode: whole rows by LDS-DMA.
    const int cA = kXOff / 16;
    int cB = a.aligned ? (w + kXOff - 16) / 16 : cA - 1;
    if (cB < cA) cB = cA - 1;
    if constexpr (MODE != kFrontColor) stage_dma<NR, FRAME>(a, tid, lds, FRAME ? src : slab + a.L0.img_off, r0, cA, cB);
    const int ni = cB - cA + 1;
    if (MODE == kFrontColor && ni > 0) {
        // rgb8/bgr8 frames: the interior chunks by 48-B vector loads and the gray conversion, K chunks per
        // thread in flight (in the kernel body: as a function it costs a VGPR, front_refactor_codegen_check.txt)
        constexpr int K = 2, VW = 12;                 // chunks in flight; dwords of a chunk's 16 pixels
        const float rci = 1.f / (float)ni;
        const int n1 = NR * ni;
        for (int base = 0; base < n1; base += 256 * K) {
            uint32_t v[K][VW];
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int item = base + k * 256 + tid;
                if (item < n1) {
                    const int i = fdiv(item, ni, rci), c = cA + item - i * ni;
                    const uint8_t* s = src + (long long)r101s(r0 - 2 + i, h) * a.stride + (16 * c - kXOff) * 3;
                    const u4a4k* q = reinterpret_cast<const u4a4k*>(s);
#pragma unroll
                    for (int t = 0; t < 3; t++) {
                        const u4a4k u = q[t];
                        v[k][4 * t] = u.x; v[k][4 * t + 1] = u.y; v[k][4 * t + 2] = u.z; v[k][4 * t + 3] = u.w;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int item = base + k * 256 + tid;
                if (item >= n1) continue;
                const int i = fdiv(item, ni, rci), c = cA + item - i * ni;
                const uint8_t* bb = reinterpret_cast<const uint8_t*>(v[k]);
                uint32_t o[4];
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    uint32_t d = 0;
#pragma unroll
                    for (int j = 0; j < 4; j++) d |= (uint32_t)gray_of(bb + 3 * (4 * t + j), a.fmt) << (8 * j);
                    o[t] = d;
                }
                *reinterpret_cast<uint4*>(lds + i * a.lp + 16 * c) = make_uint4(o[0], o[1], o[2], o[3]);
            }
        }
    }
    if constexpr (FRAME) stage_border_bytes<NR, MODE == kFrontColor>(a, tid, lds, src, r0, cB);
    __syncthreads();

    // phase 2: level-0 rows out of LDS (LDS row 0 holds core row r0 - 2)
    if constexpr (FRAME) rows_out(tid, out0, nb0 + (e0 - r0), a.nchunk0, h, r0 - 2, lds, a.lp, slab + a.L0.img_off, a.L0.pitch);

    // phase 3a: the band's level-1 core rows into an LDS row buffer, the pyrDown row walk.  A thread
    // owns one dword chunk (4 level-1 pixels) of every row and walks down the band: each staged
    // level-0 row's horizontal 5-tap sums (two chained v_dot4_u32_u8 per pixel) are computed once and
    // kept in registers for the up to three level-1 rows whose vertical window covers it.  (In the kernel
    // body: as a function it costs level mode 2 VGPRs and 2 SGPRs, profiles/front_refactor_codegen_check.txt.)
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
    border_cols<1>(tid, e1 - Y0, w1, 16 * (a.nchunk1_16 + 1) - kXOff - w1, w1, [&](int i, int x, bool in) {
        uint8_t* row = l1buf + i * a.lp1 + kXOff;
        const uint8_t v = row[in ? r101s(x, w1) : 0];
        row[x] = in ? v : (uint8_t)0;
    });
    __syncthreads();

    // phase 3b: level-1 padded rows out of the row buffer, 16 B per lane (bytes 16..23: margin, zeros)
    rows_out(tid, out1, nb1 + (e1 - Y0), a.nchunk1_16, h1, Y0, l1buf, a.lp1, slab + a.L1.img_off, a.L1.pitch);
}

// ------------------------------------------------------------------ A3: Scharr derivs
// lkpyramid.cpp calcSharrDeriv on the padded level (the stencil: scharr_word, mdx_dev.h), border = 0
// (copyMakeBorder ... BORDER_CONSTANT).  Per thread one word chunk c of padded row py + kPad: 4
// pixels (one 16-B store); each of the three source rows is one dwordx3 load of bytes x0-4 .. x0+7.
// Not __forceinline__, Level by value, on purpose: inlined by the optimizer's own inliner (it is, in both
// kernels) the chunk takes 20 VGPRs, force-inlined ahead of it 26 (profiles/front_refactor_codegen_check.txt).
__device__ static inline void scharr_chunk(const uint8_t* pyr1, uint32_t* der, long long img_bytes, long long der_words,
                                           int pair, int c, int py, Level L, int nchunk)
{
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
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int px = px0 + i;
            if (px < 0 || px >= L.w) continue;
            o[i] = scharr_word(rw[0], rw[1], rw[2], 4 + i);             // px is byte 4 + i
        }
    }
    uint32_t* row = der + (long long)pair * der_words + L.der_off + (long long)(py + kPad) * L.pitch;
    *reinterpret_cast<uint4*>(row + 4 * c) = make_uint4(o[0], o[1], o[2], o[3]);
}

// padded rows prow0 + blockIdx.y of one level
__global__ __launch_bounds__(256) void k_scharr(const uint8_t* __restrict__ pyr1, uint32_t* __restrict__ der,
                                                long long img_bytes, long long der_words, Level L, int nchunk,
                                                int prow0)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x + 4;         // word chunks 0..3 are margin
    scharr_chunk(pyr1, der, img_bytes, der_words, blockIdx.z, c, prow0 + blockIdx.y - kPad, L, nchunk);
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

hipError_t launch_gray_rows(hipStream_t s, const uint8_t* img1, int w, int stride, int fmt, uint8_t* gray1_l0,
                            int pitch, const PairFit* fit, int built0, int built1)
{
    const dim3 grid((w + 255) / 256, 64);
    hipLaunchKernelGGL(k_gray_rows, grid, dim3(64), 0, s, img1, w, stride, fmt, gray1_l0, pitch, fit, built0, built1);
    return hipGetLastError();
}

// ------------------------------------------------------------------ launchers
// last 16-B chunk index of a padded row (columns -40 .. w+39 at row bytes 24 .. 64+w+39)
static inline int last_chunk16(int w) { return (kXOff + w + kPad - 1) / 16; }
// last 4-word chunk index of a padded derivative row
static inline int last_chunk4(int w) { return (kXOff + w + kPad - 1) / 4; }

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
// k_front's static arrays (out0, out1, nout) share the CU's 160 KB with the dynamic rows
static constexpr size_t front_lds_static(int rb) { return (size_t)(2 * rb + 80 + rb + 80 + 2) * sizeof(int); }

template <int R, FrontMode M>
static hipError_t launch_k_front(dim3 grid, size_t lds, hipStream_t s, const FrontArgs& a)
{
    if (lds + front_lds_static(R) > 64 * 1024)
        if (hipError_t e = hipFuncSetAttribute((const void*)k_front<R, M>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)lds))
            return e;
    hipLaunchKernelGGL((k_front<R, M>), grid, dim3(256), lds, s, a);
    return hipGetLastError();
}
template <FrontMode M>
static hipError_t launch_k_front_rb(int rb, dim3 grid, size_t lds, hipStream_t s, const FrontArgs& a)
{
    return rb == 4 ? launch_k_front<4, M>(grid, lds, s, a) : rb == 2 ? launch_k_front<2, M>(grid, lds, s, a)
                                                           : launch_k_front<1, M>(grid, lds, s, a);
}

static hipError_t launch_front_bands(hipStream_t s, FrontArgs& a, FrontMode mode, int rlo = 0, int rhi = -1)
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
    if (lds + front_lds_static(rb) > 160 * 1024) return hipErrorInvalidValue;   // rows wider than ~31K px
    // destination rows [rlo, rhi) of the level built (all by default): the bands covering them
    if (rhi < 0 || rhi > a.L1.h) rhi = a.L1.h;
    rlo = std::max(0, std::min(rlo, rhi));
    a.band0 = rlo / rb;
    a.nbands = (rhi + rb - 1) / rb - a.band0;
    if (a.nbands <= 0) return hipSuccess;
    const dim3 grid((unsigned)(a.nbands * a.nz));
    switch (mode) {
    case kFrontMono: return launch_k_front_rb<kFrontMono>(rb, grid, lds, s, a);
    case kFrontColor: return launch_k_front_rb<kFrontColor>(rb, grid, lds, s, a);
    default: return launch_k_front_rb<kFrontLevel>(rb, grid, lds, s, a);
    }
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
    return launch_front_bands(s, a, fmt == MDX_FMT_GRAY8 ? kFrontMono : kFrontColor, r1lo, r1hi);
}

hipError_t launch_pyr_levels(hipStream_t s, int batch, uint8_t* pyr1, uint8_t* pyr2, const Geometry& g, int fsel,
                             const RowSpan* rows)
{
    for (int l = 2; l < g.nlev; l++) {
        FrontArgs a = front_args(batch, pyr1, pyr2, g, l - 1, fsel);
        if (hipError_t e = launch_front_bands(s, a, kFrontLevel, rows ? rows[l].lo : 0, rows ? rows[l].hi : -1)) return e;
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
    const int c = blockIdx.x * blockDim.x + threadIdx.x + 4;         // word chunks 0..3 are margin
    scharr_chunk(pyr1, der, img_bytes, der_words, blockIdx.z, c, (int)blockIdx.y - sl.row0[l] - kPad, sl.L[l], sl.nchunk[l]);
}

hipError_t launch_scharr_levels(hipStream_t s, int batch, const uint8_t* pyr1, uint32_t* der, const Geometry& g)
{
    ScharrLevels sl{};
    sl.nlev = g.nlev;
    int rows = 0, maxc = 0;
    for (int l = 0; l < g.nlev; l++) {
        sl.L[l] = g.lv[l];
        sl.nchunk[l] = last_chunk4(g.lv[l].w);
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
    const int nchunk = last_chunk4(L.w);
    if (prow1 < 0 || prow1 > L.rows) prow1 = L.rows;
    prow0 = std::max(0, std::min(prow0, prow1));
    if (prow1 == prow0) return hipSuccess;
    const dim3 grid((nchunk - 4 + 1 + 63) / 64, prow1 - prow0, batch);
    hipLaunchKernelGGL(k_scharr, grid, dim3(64), 0, s, pyr1, der, g.img_bytes, g.der_words, L, nchunk, prow0);
    return hipGetLastError();
}

}  // namespace mdx
