// mdx_lk_point.hip -- the per-point LK (k_lk: one wave tracks its points through every pyramid level)
// and the trajectory bookkeeping, with their launchers.
// Every kernel reproduces the arithmetic of the OpenCV 2.4 routine the reference calls, bit for bit
// (integer stages exactly; float and double stages in the same evaluation order, compiled with
// -ffp-contract=off so no expression is fused into an FMA).
//   A5      k_lk             calcOpticalFlowPyrLK (LKTrackerInvoker, SSE2 summation order): the pair
//                            path of very sparse grids, and the chained trajectory passes
//           k_traj_init / k_traj_update   calculateOpticalFlowTrajectory's grid and per-pass update
#include "mdx_dev.h"

#include <float.h>

namespace mdx {

// ------------------------------------------------------------------ A5: LK tracker
//
// One 64-lane wave = one workgroup tracks PPW = 64/LPP grid points through every pyramid
// level (LPP lanes per point).  Per level and point the 40x40 window is cut into 5 chunks of
// R = 8 rows; each lane owns EC = 320/LPP window elements per chunk and keeps its
// interpolated I*32, Ix, Iy for the whole level in registers (NE = 5*EC elements).
//
// Exact summation order.  OpenCV's SSE2 path accumulates every sum in four float lanes:
// lane k takes window columns x = 4g+k in (row, g) order; A = ((P0+P1)+P2)+P3 and
// b = (P0+P2)+(P1+P3).  A GPU reduction tree would round differently, so the kernel keeps
// the reference's order: the lanes compute the per-element products (exact integer
// products rounded once to float) in parallel and store them chain-ordered in LDS; then one
// lane per chain (12 chains for A11/A12/A22, 8 for b1/b2) adds its 80 terms of the chunk in
// order.  The result is bit-identical to the x86 reference, not merely within tolerance.
typedef short s2k __attribute__((ext_vector_type(2)));
// v_dot2_i32_i16 (VOP3P) with its accumulator in an SGPR.  The builtin with a constant accumulator
// compiles to v_mov + v_dot2c_i32_i16 (the constant rematerialised in a VGPR per dot product): one
// more VALU per chain (the trajectory LK's rounding biases 256 and 8192).
__device__ __forceinline__ int sdot2_sacc(s2k a, s2k b, int c)
{
    int r;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
    return r;
}

// ---- arithmetic shared by every window layout
// the W_BITS 14 bilinear weights (w00, w01, w10, w11) of the fractional offset (fa, fb)
__device__ __forceinline__ int4 lk_weights(float fa, float fb)
{
    const int w00 = __float2int_rn((1.f - fa) * (1.f - fb) * 16384.f);
    const int w01 = __float2int_rn(fa * (1.f - fb) * 16384.f);
    const int w10 = __float2int_rn((1.f - fa) * fb * 16384.f);
    return make_int4(w00, w01, w10, 16384 - w00 - w01 - w10);
}
__device__ __forceinline__ int lk_tap_dot(s2k up, s2k lo, s2k W0, s2k W1)
{
    return __builtin_amdgcn_sdot2(up, W0, sdot2_sacc(lo, W1, 256), false) >> 9;
}
__device__ __forceinline__ int lk_deriv_dot(s2k up, s2k lo, s2k W0, s2k W1)
{
    return __builtin_amdgcn_sdot2(up, W0, sdot2_sacc(lo, W1, 8192), false) >> 14;
}

// (byte b, byte b + 1) of the 8 bytes (hi, lo) as a 16-bit pair; the Ix and the Iy halves of two
// adjacent derivative words
__device__ __forceinline__ s2k lk_byte_pair(uint32_t hi, uint32_t lo, int b)
{
    return __builtin_bit_cast(s2k, __builtin_amdgcn_perm(hi, lo, 0x0c000c00u | (unsigned)b | ((unsigned)(b + 1) << 16)));
}
__device__ __forceinline__ s2k lk_ix_pair(uint32_t d1, uint32_t d0)
{
    return __builtin_bit_cast(s2k, __builtin_amdgcn_perm(d1, d0, 0x05040100u));
}
__device__ __forceinline__ s2k lk_iy_pair(uint32_t d1, uint32_t d0)
{
    return __builtin_bit_cast(s2k, __builtin_amdgcn_perm(d1, d0, 0x07060302u));
}
// 4 (N + 1) bytes of a row from byte address p, realigned: w[0 .. N-1] = bytes p .. p + 4 N - 1
__device__ __forceinline__ void lk_row_words(const uint8_t* p, uint32_t (&w)[2])
{
    const uintptr_t u = reinterpret_cast<uintptr_t>(p);
    const u3a4k v = gload<u3a4k>(u & ~(uintptr_t)3);
    const uint32_t o = (uint32_t)(u & 3);
    w[0] = __builtin_amdgcn_alignbyte(v.y, v.x, o);
    w[1] = __builtin_amdgcn_alignbyte(v.z, v.y, o);
}
__device__ __forceinline__ void lk_row_words(const uint8_t* p, uint32_t (&w)[3])
{
    const uintptr_t u = reinterpret_cast<uintptr_t>(p);
    const u4a4k v = gload<u4a4k>(u & ~(uintptr_t)3);
    const uint32_t o = (uint32_t)(u & 3);
    w[0] = __builtin_amdgcn_alignbyte(v.y, v.x, o);
    w[1] = __builtin_amdgcn_alignbyte(v.z, v.y, o);
    w[2] = __builtin_amdgcn_alignbyte(v.w, v.z, o);
}
// 6 or 11 derivative words from q (4-B aligned)
__device__ __forceinline__ void lk_deriv_words(const uint32_t* q, uint32_t (&d)[6])
{
    const u4a4k a = *reinterpret_cast<const u4a4k*>(q);
    const u2a4k b = *reinterpret_cast<const u2a4k*>(q + 4);
    d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w; d[4] = b.x; d[5] = b.y;
}
__device__ __forceinline__ void lk_deriv_words(const uint32_t* q, uint32_t (&d)[11])
{
    const u4a4k a0 = *reinterpret_cast<const u4a4k*>(q);
    const u4a4k a1 = *reinterpret_cast<const u4a4k*>(q + 4);
    const u3a4k a2 = *reinterpret_cast<const u3a4k*>(q + 8);
    d[0] = a0.x; d[1] = a0.y; d[2] = a0.z; d[3] = a0.w;
    d[4] = a1.x; d[5] = a1.y; d[6] = a1.z; d[7] = a1.w;
    d[8] = a2.x; d[9] = a2.y; d[10] = a2.z;
}

// (byte i, byte i + 1) of a realigned run of RW words as a 16-bit pair (i is a constant once the
// element loops are unrolled)
template <int RW>
__device__ __forceinline__ s2k lk_run_pair(const uint32_t (&w)[RW], int i)
{
    if constexpr (RW == 2) return lk_byte_pair(w[1], w[0], i);
    const uint32_t hi = (i >> 2) + 1 < RW ? w[(i >> 2) + 1 < RW ? (i >> 2) + 1 : RW - 1] : 0u;
    return lk_byte_pair(hi, w[i >> 2], i & 3);
}

// ---- per-element bookkeeping of the two phases (k = the element's index in the lane's level-long
// arrays, wp = its slot in the LDS chains)
constexpr int kLkStride = 88;   // floats per chain (80 used; 4*odd => b128 conflict-free)
// A sums: keep I*32 (si, two per word) and (Ix, Iy) (sd) for the iterations; Ix*Ix, Ix*Iy, Iy*Iy to the chains
template <int NE>
__device__ __forceinline__ void lk_keep(int k, int ival, int ixv, int iyv, uint32_t (&sd)[NE], uint32_t (&si)[(NE + 1) / 2],
                                        float* wp)
{
    sd[k] = ((uint32_t)ixv & 0xffffu) | ((uint32_t)iyv << 16);
    if (k & 1) si[k >> 1] = (si[k >> 1] & 0xffffu) | ((uint32_t)ival << 16);
    else si[k >> 1] = (uint32_t)ival;
    // |Ix|, |Iy| <= 4080: 24-bit multiplies (v_mul_i32_i24, full rate; a 32-bit v_mul_lo_u32 is
    // quarter rate), products exact in int32
    wp[0] = (float)__mul24(ixv, ixv);
    wp[4 * kLkStride] = (float)__mul24(ixv, iyv);
    wp[8 * kLkStride] = (float)__mul24(iyv, iyv);
}
// iterations: (J - I) * 32 times Ix and Iy to the b chains
template <int NE>
__device__ __forceinline__ void lk_mismatch(int k, int jv, const uint32_t (&sd)[NE], const uint32_t (&si)[(NE + 1) / 2],
                                            float* wp)
{
    const int iv = (k & 1) ? (int)(si[k >> 1] >> 16) : (int)(si[k >> 1] & 0xffffu);
    const int diff = jv - iv;
    const uint32_t dv = sd[k];
    // |diff| <= 8160, |Ix|, |Iy| <= 4080: exact 24-bit multiplies
    wp[0] = (float)__mul24(diff, (int)(int16_t)dv);
    wp[4 * kLkStride] = (float)__mul24(diff, (int)dv >> 16);
}

// ---- one 8-row chunk of a run layout's window elements, A sums (I) and iterations (J).  o: offset
// of the lane's first element of the chunk from the level's core origin (jp: its J address); w: the
// bilinear weights; k0: index of that element in sd / si; woff: the elements' LDS chain slots.  (The
// block layout's chunk code stays inside k_lk: as functions of this kind it cost k_lk<16, true> 8
// VGPRs, and with the A-phase one an occupancy step.)
//
// A run of RUN adjacent window columns of one row (one or two points per wave): two realigned row
// loads for the taps and two vector-loaded rows of derivative words, instead of 4 byte loads per element.
template <int RUN, int NE>
__device__ __forceinline__ void lk_run_chunk_I(const uint8_t* Ib, const uint32_t* Db, int o, int pitch, int4 w, int k0,
                                               uint32_t (&sd)[NE], uint32_t (&si)[(NE + 1) / 2], float* ch,
                                               const int (&woff)[RUN])
{
    uint32_t i0w[(RUN + 4) / 4], i1w[(RUN + 4) / 4], dr0[RUN + 1], dr1[RUN + 1];
    lk_row_words(Ib + o, i0w);
    lk_row_words(Ib + o + pitch, i1w);
    lk_deriv_words(Db + o, dr0);
    lk_deriv_words(Db + o + pitch, dr1);
    const s2k W0 = {(short)w.x, (short)w.y}, W1 = {(short)w.z, (short)w.w};
#pragma unroll
    for (int i = 0; i < RUN; i++) {
        const int ival = lk_tap_dot(lk_run_pair(i0w, i), lk_run_pair(i1w, i), W0, W1);
        const s2k x0 = lk_ix_pair(dr0[i + 1], dr0[i]), x1 = lk_ix_pair(dr1[i + 1], dr1[i]);
        const s2k y0 = lk_iy_pair(dr0[i + 1], dr0[i]), y1 = lk_iy_pair(dr1[i + 1], dr1[i]);
        const int ixv = lk_deriv_dot(x0, x1, W0, W1);
        const int iyv = lk_deriv_dot(y0, y1, W0, W1);
        lk_keep(k0 + i, ival, ixv, iyv, sd, si, ch + woff[i]);
    }
}
template <int RUN, int NE>
__device__ __forceinline__ void lk_run_chunk_J(const uint8_t* jp, int pitch, int4 w, int k0,
                                               const uint32_t (&sd)[NE], const uint32_t (&si)[(NE + 1) / 2], float* ch,
                                               const int (&woff)[RUN])
{
    uint32_t j0w[(RUN + 4) / 4], j1w[(RUN + 4) / 4];
    lk_row_words(jp, j0w);
    lk_row_words(jp + pitch, j1w);
    const s2k W0 = {(short)w.x, (short)w.y}, W1 = {(short)w.z, (short)w.w};
#pragma unroll
    for (int i = 0; i < RUN; i++) {
        const int jv = lk_tap_dot(lk_run_pair(j0w, i), lk_run_pair(j1w, i), W0, W1);
        lk_mismatch(k0 + i, jv, sd, si, ch + woff[i]);
    }
}
// ---- trajectory pass bookkeeping
// One pass j -> j+1 of one point (optical_flow_calculator.cpp:178-242): a tracked point moves (and
// its trajectory grows) only when it lands strictly inside the 10-px border; lost or border points
// stay.  On the last pass the Vec4d of :183-206 / :220-230 and num_vectors (order-free integer
// count), and the pass's start point.  (sx, sy): where the pass started; status: the point's LK
// status (nonzero: tracked); end: where the LK left it.  Both are references: each is read where the
// reference reads it.  AGENT: cur and tlen are handed between the chained passes' waves (k_lk chain
// mode), so they are accessed past the caches, with agent-scope atomics.
template <bool AGENT, typename S>
__device__ __forceinline__ void traj_pass_point(int i, float sx, float sy, const S& status, const float* end, bool last,
                                                float* cur, float* traj, int* tlen, int nimg, int w, int h,
                                                double min_vector_size, double* vectors, float* start_pts, int* num)
{
    double* v = (last && vectors) ? vectors + 4LL * i : nullptr;
    if (last && start_pts) {
        start_pts[2 * i] = sx;
        start_pts[2 * i + 1] = sy;
    }
    if (status) {
        const float ex = end[0], ey = end[1];
        if (last) {
            const float xd = ex - sx, yd = ey - sy;
            if (fabs((double)fabsf(xd)) > min_vector_size || fabs((double)fabsf(yd)) > min_vector_size) {
                if (v) { v[0] = sx; v[1] = sy; v[2] = xd; v[3] = yd; }
                atomicAdd(num, 1);
            } else if (v) {
                v[0] = sx; v[1] = sy; v[2] = 0.0; v[3] = 0.0;
            }
        }
        if (ex > 10.0f && ey > 10.0f && ex < (float)(w - 10) && ey < (float)(h - 10)) {
            int l;
            if constexpr (AGENT) {
                __hip_atomic_store(reinterpret_cast<unsigned long long*>(cur) + i,
                                   __builtin_bit_cast(unsigned long long, make_float2(ex, ey)), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
                l = __hip_atomic_load(tlen + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                cur[2 * i] = ex;
                cur[2 * i + 1] = ey;
                l = tlen[i];
            }
            traj[((long long)i * nimg + l) * 2] = ex;
            traj[((long long)i * nimg + l) * 2 + 1] = ey;
            if constexpr (AGENT) __hip_atomic_store(tlen + i, l + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else tlen[i] = l + 1;
        }
    } else if (v) {
        v[0] = -1.0; v[1] = -1.0; v[2] = 0.0; v[3] = 0.0;
    }
}

// k_lk<LPP, true>: the chained trajectory passes (TrajChain); grid = nimg-1 passes x npts points,
// pass-major, one point per wave.
constexpr int kChainSpinMax = 1 << 19;   // ~0.1 s of s_sleep(8) polls: a lost hand-off gives wrong
                                         // results, never a hung launch

template <int LPP, bool CHAIN>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 8))) void k_lk(LkArgs a, TrajChain t)
{
    constexpr int WIN = 40, R = 8, NCH = WIN / R, EC = R * WIN / LPP, NE = NCH * EC, PPW = 64 / LPP;
    constexpr int STRIDE = kLkStride;
    constexpr int PT_FLOATS = 12 * STRIDE + 16;
    constexpr float HALFW = 19.5f;             // (winSize.width-1)*0.5f
    constexpr float FLT_SCALE = 1.f / (1 << 20);
    __shared__ float4 lds4[PPW * PT_FLOATS / 4];

    static_assert(LPP == 64 || LPP == 32 || LPP == 16, "one, two or four points per wave");
    // Window layouts, per 8-row chunk.  One or two points per wave: lane s owns a run of RUN adjacent
    // window columns of one row (row s / (40 / RUN), columns RUN (s % (40 / RUN)) .. + RUN - 1), so its
    // taps of a chunk are two realigned row loads (v_perm + v_dot2 tap pairs) and its derivative words
    // two vector-loaded rows, instead of 4 byte loads per element.  Four points per wave (BLK): a block
    // of 4 rows x 5 columns (rows 4 (s / 8) .. + 3, columns 5 (s % 8) .. + 4), which shares tap rows
    // between its rows: 5 row loads and 75 pair-building v_perm per chunk (I taps, Ix and Iy pairs)
    // instead of the 2 x 2 loads and 120 of a run of 20, and its rows for the next chunk (derivative
    // rows in the A sums, J rows in the iterations) are loaded while the current one is summed: two
    // waves per SIMD hide little of a global load's latency (ring callback 2.37 against 2.49 ms,
    // profiles/r06_ab_traj_blk.txt).  Two points per wave: 144 VGPRs, 3 waves per SIMD.
    constexpr bool BLK = LPP == 16;
    constexpr int RUN = LPP == 64 ? 5 : 10;    // (unused by the block layout)
    const int lane = threadIdx.x;
    const int p = lane / LPP, s = lane % LPP;
    // chain mode: block b = pass * nbp + points (dispatch order: every block a wave waits for was
    // dispatched before it, and pass 0 never waits, so the waits always drain)
    const unsigned nbp = (unsigned)((a.npts + PPW - 1) / PPW);       // blocks per pass
    const int pass = CHAIN ? (int)(blockIdx.x / nbp) : 0;
    const int pt = CHAIN ? (int)(blockIdx.x - (unsigned)pass * nbp) * PPW + p : (int)blockIdx.x * PPW + p;
    const int pair = CHAIN ? 0 : blockIdx.y;
    const bool valid = pt < a.npts;
    float* ch = reinterpret_cast<float*>(lds4) + p * PT_FLOATS;
    float* res = ch + 12 * STRIDE;

    // element geometry (level independent): window row and column, LDS chain slot
    static_assert(BLK ? EC == 20 : EC == RUN, "the point's lanes cover a chunk");
    int woff[EC], ex[EC], ey[EC];
#pragma unroll
    for (int i = 0; i < EC; i++) {
        const int e = BLK ? (4 * (s / 8) + i / 5) * WIN + 5 * (s % 8) + i % 5
                    : (s / (WIN / RUN)) * WIN + RUN * (s % (WIN / RUN)) + i;
        ey[i] = e / WIN;
        ex[i] = e % WIN;
        woff[i] = (ex[i] & 3) * STRIDE + ey[i] * 10 + (ex[i] >> 2);
    }
    const int gx = valid ? pt / a.ny : 0, gy = valid ? pt % a.ny : 0;
    float px0 = (float)(gx * a.pixel_step), py0 = (float)(gy * a.pixel_step);
    if constexpr (CHAIN) {
        // the point pass - 1 left (k_traj_init's grid point for pass 0): wait for that pass, then
        // read it past the caches (the MI355X_MICROARCH.md hand-off: the writer stores sc1, waits
        // vmcnt(0), then bumps the flag)
        if (valid) {
            if (pass > 0) {
                int n = 0;
                while (__hip_atomic_load(t.flag + pt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < pass &&
                       n < kChainSpinMax) {
                    __builtin_amdgcn_s_sleep(8);
                    n++;
                }
                if (n >= kChainSpinMax && s == 0) atomicAdd(t.num + 1, 1);   // reported as an error by the host
                // the point's load stays below the poll (wavefront scope: no instruction; the load
                // is sc1 and issues only once the poll has matched)
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            const float2 c = __builtin_bit_cast(
                float2, __hip_atomic_load(reinterpret_cast<const unsigned long long*>(t.cur) + pt, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT));
            px0 = c.x;
            py0 = c.y;
        }
    } else if (a.prev_pts && valid) {   // trajectory passes: arbitrary start points (flags 0: nextPt = prevPt)
        const float* pp = a.prev_pts + ((long long)pair * a.npts + pt) * 2;
        px0 = pp[0];
        py0 = pp[1];
    }
    float npx = 0.f, npy = 0.f;   // nextPts[ptidx]
    int status = 1;

    uint32_t sd[NE];              // (Ix & 0xffff) | Iy << 16
    uint32_t si[(NE + 1) / 2];    // I*32 values, two per word

    const uint8_t* slab1 = CHAIN ? t.pyr[pass] : a.pyr1 + (long long)pair * a.g.img_bytes;
    const uint8_t* slab2 = CHAIN ? t.pyr[pass + 1] : a.pyr2 + (long long)pair * a.g.img_bytes;
    const uint32_t* dslab = CHAIN ? t.der[pass] : a.der + (long long)pair * a.g.der_words;

    for (int level = a.maxl; level >= 0; --level) {
        const Level L = a.g.lv[level];
        const int pitch = L.pitch;
        const uint8_t* Ib = slab1 + L.img_off + L.core();
        const uint8_t* Jb = slab2 + L.img_off + L.core();
        const uint32_t* Db = dslab + L.der_off + L.core();

        const float scale = (float)(1. / (1 << level));
        float ppx = px0 * scale, ppy = py0 * scale;
        if (level == a.maxl) { npx = ppx; npy = ppy; }
        else { npx = npx * 2.f; npy = npy * 2.f; }
        ppx = ppx - HALFW;
        ppy = ppy - HALFW;
        const int ipx = (int)floorf(ppx), ipy = (int)floorf(ppy);
        bool ok = valid && !(ipx < -WIN || ipx >= L.w || ipy < -WIN || ipy >= L.h);
        if (valid && !ok && level == 0) status = 0;

        int w00 = 0, w01 = 0, w10 = 0, w11 = 0;
        if (ok) {
            const int4 w = lk_weights(ppx - (float)ipx, ppy - (float)ipy);
            w00 = w.x; w01 = w.y; w10 = w.z; w11 = w.w;
        }
        int toff[EC];
#pragma unroll
        for (int i = 0; i < EC; i++) toff[i] = ey[i] * pitch + ex[i];
        const int ibase = ipy * pitch + ipx;

        // ---- window extraction + A sums (chains q*4+k, q: 0 A11, 1 A12, 2 A22)
        float acc = 0.f;
        u4a4k dpa[BLK ? 5 : 1] = {};
        u2a4k dpb[BLK ? 5 : 1] = {};
        if (BLK && ok)
#pragma unroll
            for (int ar = 0; ar < (BLK ? 5 : 1); ar++) {
                const uint32_t* q = Db + (ibase + toff[0]) + ar * pitch;
                dpa[ar] = *reinterpret_cast<const u4a4k*>(q);
                dpb[ar] = *reinterpret_cast<const u2a4k*>(q + 4);
            }
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            if constexpr (BLK) {
                if (ok) {
                    // 4 x 5 block: rows a = 0 .. 4 of the block (4 element rows + the lower tap row),
                    // each 6 I bytes and 6 derivative words; row a's tap / Ix / Iy pairs serve element row
                    // a as its upper taps and element row a - 1 as its lower ones
                    const int o = ibase + c * R * pitch + toff[0];
                    const s2k W0 = {(short)w00, (short)w01}, W1 = {(short)w10, (short)w11};
                    s2k pu[5], xu[5], yu[5];
#pragma unroll
                    for (int ar = 0; ar <= 4; ar++) {
                        uint32_t iw[2];
                        lk_row_words(Ib + o + ar * pitch, iw);
                        const u4a4k v = dpa[BLK ? ar : 0];
                        const u2a4k w2 = dpb[BLK ? ar : 0];
                        const uint32_t d[6] = {v.x, v.y, v.z, v.w, w2.x, w2.y};
                        s2k pl[5], xl[5], yl[5];
#pragma unroll
                        for (int b = 0; b < 5; b++) {
                            pl[b] = lk_byte_pair(iw[1], iw[0], b);
                            xl[b] = lk_ix_pair(d[b + 1], d[b]);
                            yl[b] = lk_iy_pair(d[b + 1], d[b]);
                        }
                        if (ar > 0) {
#pragma unroll
                            for (int b = 0; b < 5; b++) {
                                const int i = 5 * (ar - 1) + b;
                                const int ival = lk_tap_dot(pu[b], pl[b], W0, W1);
                                const int ixv = lk_deriv_dot(xu[b], xl[b], W0, W1);
                                const int iyv = lk_deriv_dot(yu[b], yl[b], W0, W1);
                                lk_keep(c * EC + i, ival, ixv, iyv, sd, si, ch + woff[i]);
                            }
                        }
#pragma unroll
                        for (int b = 0; b < 5; b++) { pu[b] = pl[b]; xu[b] = xl[b]; yu[b] = yl[b]; }
                    }
                    if (c + 1 < NCH)
#pragma unroll
                        for (int ar = 0; ar < (BLK ? 5 : 1); ar++) {
                            const uint32_t* q = Db + (ibase + (c + 1) * R * pitch + toff[0]) + ar * pitch;
                            dpa[ar] = *reinterpret_cast<const u4a4k*>(q);
                            dpb[ar] = *reinterpret_cast<const u2a4k*>(q + 4);
                        }
                }
            } else if (ok) {
                lk_run_chunk_I<RUN>(Ib, Db, ibase + c * R * pitch + toff[0], pitch, make_int4(w00, w01, w10, w11), c * EC, sd,
                                    si, ch, woff);
            }
            __syncthreads();
            if (ok && s < 12) {
                const float4* cp = reinterpret_cast<const float4*>(ch + s * STRIDE);
#pragma unroll
                for (int t = 0; t < 20; t++) {
                    const float4 v = cp[t];
                    acc = acc + v.x; acc = acc + v.y; acc = acc + v.z; acc = acc + v.w;
                }
            }
            __syncthreads();
        }
        if (ok && s < 12) res[s] = acc;
        __syncthreads();

        float A11 = 0.f, A12 = 0.f, A22 = 0.f, Dinv = 0.f;
        if (ok) {
            const float4 r0 = reinterpret_cast<const float4*>(res)[0];
            const float4 r1 = reinterpret_cast<const float4*>(res)[1];
            const float4 r2 = reinterpret_cast<const float4*>(res)[2];
            A11 = ((r0.x + r0.y) + r0.z) + r0.w;
            A12 = ((r1.x + r1.y) + r1.z) + r1.w;
            A22 = ((r2.x + r2.y) + r2.z) + r2.w;
            A11 = A11 * FLT_SCALE;
            A12 = A12 * FLT_SCALE;
            A22 = A22 * FLT_SCALE;
            const float D = A11 * A22 - A12 * A12;
            const float minEig = (A22 + A11 - __builtin_sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) /
                                 (float)(2 * WIN * WIN);
            if (minEig < a.min_eig || D < FLT_EPSILON) {
                ok = false;
                if (level == 0) status = 0;
            } else {
                Dinv = 1.f / D;
            }
        }
        __syncthreads();   // res is rewritten by the iteration phase

        // ---- Newton iterations
        float nx = npx - HALFW, ny = npy - HALFW;
        float pdx = 0.f, pdy = 0.f;
        bool act = ok;
        for (int j = 0; j < a.max_iters; j++) {
            if (!__any(act)) break;
            int jbase = 0, v00 = 0, v01 = 0, v10 = 0, v11 = 0;
            if (act) {
                const int inx = (int)floorf(nx), iny = (int)floorf(ny);
                if (inx < -WIN || inx >= L.w || iny < -WIN || iny >= L.h) {
                    act = false;
                    if (level == 0) status = 0;
                } else {
                    const int4 w = lk_weights(nx - (float)inx, ny - (float)iny);
                    v00 = w.x; v01 = w.y; v10 = w.z; v11 = w.w;
                    jbase = iny * pitch + inx;
                }
            }
            float bacc = 0.f;
            // BLK: the block's five J rows of chunk c + 1 are loaded while chunk c is summed (two waves
            // per SIMD hide little of a global load's latency); pitch is a multiple of 64, so one
            // realignment shift serves every row and chunk
            u3a4k jr[BLK ? 5 : 1] = {};
            uint32_t jsh = 0;
            const uint8_t* jb0 = nullptr;
            if (BLK && act) {
                const uintptr_t u = reinterpret_cast<uintptr_t>(Jb + (jbase + toff[0]));
                jsh = (uint32_t)(u & 3);
                jb0 = reinterpret_cast<const uint8_t*>(u & ~(uintptr_t)3);
#pragma unroll
                for (int ar = 0; ar < (BLK ? 5 : 1); ar++) jr[ar] = gload<u3a4k>(reinterpret_cast<uintptr_t>(jb0 + ar * pitch));
            }
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                if constexpr (BLK) {
                    if (act) {
                        const s2k W0 = {(short)v00, (short)v01}, W1 = {(short)v10, (short)v11};
                        s2k pu[5];
#pragma unroll
                        for (int ar = 0; ar <= 4; ar++) {
                            const uint32_t lo = __builtin_amdgcn_alignbyte(jr[BLK ? ar : 0].y, jr[BLK ? ar : 0].x, jsh);
                            const uint32_t hi = __builtin_amdgcn_alignbyte(jr[BLK ? ar : 0].z, jr[BLK ? ar : 0].y, jsh);
                            s2k pl[5];
#pragma unroll
                            for (int b = 0; b < 5; b++) pl[b] = lk_byte_pair(hi, lo, b);
                            if (ar > 0) {
#pragma unroll
                                for (int b = 0; b < 5; b++) {
                                    const int i = 5 * (ar - 1) + b;
                                    lk_mismatch(c * EC + i, lk_tap_dot(pu[b], pl[b], W0, W1), sd, si, ch + woff[i]);
                                }
                            }
#pragma unroll
                            for (int b = 0; b < 5; b++) pu[b] = pl[b];
                        }
                        if (c + 1 < NCH)
#pragma unroll
                            for (int ar = 0; ar < (BLK ? 5 : 1); ar++)
                                jr[ar] = gload<u3a4k>(reinterpret_cast<uintptr_t>(jb0 + ((c + 1) * R + ar) * pitch));
                    }
                } else if (act) {
                    lk_run_chunk_J<RUN>(Jb + (jbase + c * R * pitch + toff[0]), pitch, make_int4(v00, v01, v10, v11), c * EC,
                                        sd, si, ch, woff);
                }
                __syncthreads();
                if (act && s < 8) {
                    const float4* cp = reinterpret_cast<const float4*>(ch + s * STRIDE);
#pragma unroll
                    for (int t = 0; t < 20; t++) {
                        const float4 v = cp[t];
                        bacc = bacc + v.x; bacc = bacc + v.y; bacc = bacc + v.z; bacc = bacc + v.w;
                    }
                }
                __syncthreads();
            }
            if (act && s < 8) res[s] = bacc;
            __syncthreads();
            if (act) {
                const float4 q1 = reinterpret_cast<const float4*>(res)[0];
                const float4 q2 = reinterpret_cast<const float4*>(res)[1];
                float b1 = (q1.x + q1.z) + (q1.y + q1.w);
                float b2 = (q2.x + q2.z) + (q2.y + q2.w);
                b1 = b1 * FLT_SCALE;
                b2 = b2 * FLT_SCALE;
                const float dx = (A12 * b2 - A22 * b1) * Dinv;
                const float dy = (A12 * b1 - A11 * b2) * Dinv;
                nx = nx + dx;
                ny = ny + dy;
                npx = nx + HALFW;
                npy = ny + HALFW;
                if ((double)dx * dx + (double)dy * dy <= a.eps2) {
                    act = false;
                } else if (j > 0 && fabs((double)fabsf(dx + pdx)) < 0.01 && fabs((double)fabsf(dy + pdy)) < 0.01) {
                    npx = npx - dx * 0.5f;
                    npy = npy - dy * 0.5f;
                    act = false;
                }
                pdx = dx;
                pdy = dy;
            }
            __syncthreads();
        }

        if (level == 0 && valid && status) {
            // err pass of LKTrackerInvoker: its final bounds check is observable (status).
            const int fx = (int)floorf(npx - HALFW), fy = (int)floorf(npy - HALFW);
            if (fx < -WIN || fx >= L.w || fy < -WIN || fy >= L.h) status = 0;
        }
    }

    if constexpr (CHAIN) {
        // this point's pass bookkeeping (k_traj_update's), then the hand-off to the next pass
        if (valid && s == 0) {
            const bool last = pass == t.nimg - 2;
            // outputs: the caller's mapped page-locked arrays when given, else the device ones
            float* tj = t.htraj ? t.htraj : t.traj;
            double* vv = t.hvec ? t.hvec : t.vectors;
            float* sp0 = t.hstart ? t.hstart : t.start_pts;
            if (t.htraj && pass == 0) {   // k_traj_init wrote the device row's start
                tj[(long long)pt * t.nimg * 2] = px0;
                tj[(long long)pt * t.nimg * 2 + 1] = py0;
            }
            const float end[2] = {npx, npy};
            traj_pass_point<true>(pt, px0, py0, status, end, last, t.cur, tj, t.tlen, t.nimg, t.w, t.h, t.mvs, vv,
                                  sp0, t.num);
            if (last && t.htraj) {
                // the mapped row's entries past traj_len (the device rows were zeroed by k_traj_init;
                // every entry of a mapped row is written once) and traj_len itself
                const int lf = __hip_atomic_load(t.tlen + pt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                for (int k = lf; k < t.nimg; k++) {
                    tj[((long long)pt * t.nimg + k) * 2] = 0.f;
                    tj[((long long)pt * t.nimg + k) * 2 + 1] = 0.f;
                }
                t.htlen[pt] = lf;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(t.flag + pt, pass + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else if (valid && s == 0) {
        const long long o = (long long)pair * a.npts + pt;
        a.next_pts[2 * o] = npx;
        a.next_pts[2 * o + 1] = npy;
        a.status[o] = (uint8_t)status;
    }
}

// ------------------------------------------------------------ trajectory tracking
// OpticalFlowCalculator::calculateOpticalFlowTrajectory (optical_flow_calculator.cpp:133-257).
// init: points = the grid (:148-158, x-major), every trajectory = its grid point.
__global__ void k_traj_init(int npts, int ny, int pixel_step, int nimg, float* __restrict__ cur,
                            float* __restrict__ traj, int* __restrict__ tlen, int* __restrict__ num,
                            int* __restrict__ flag)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        num[0] = 0;
        if (flag) num[1] = 0;   // chain mode: hand-off timeouts
    }
    if (i >= npts) return;
    if (flag) flag[i] = 0;
    const float x = (float)((i / ny) * pixel_step), y = (float)((i % ny) * pixel_step);
    cur[2 * i] = x;
    cur[2 * i + 1] = y;
    traj[(long long)i * nimg * 2] = x;
    traj[(long long)i * nimg * 2 + 1] = y;
    for (int k = 2; k < 2 * nimg; k++) traj[(long long)i * nimg * 2 + k] = 0.f;   // entries past traj_len: 0
    tlen[i] = 1;
}

// One pass j -> j+1 as a launch of its own (MDX_TRAJ_CHAIN=0, or more frames than the chain holds):
// the pass bookkeeping of every point, after the pass's k_lk<64, false>.
__global__ void k_traj_update(int npts, const float* __restrict__ next_pts, const uint8_t* __restrict__ status,
                              float* __restrict__ cur, float* __restrict__ traj, int* __restrict__ tlen, int nimg, int w,
                              int h, int last, double min_vector_size, double* __restrict__ vectors,
                              float* __restrict__ start_pts, int* __restrict__ num)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npts) return;
    traj_pass_point<false>(i, cur[2 * i], cur[2 * i + 1], status[i], next_pts + 2 * i, last != 0, cur, traj, tlen,
                           nimg, w, h, min_vector_size, vectors, start_pts, num);
}

hipError_t launch_traj_init(hipStream_t s, int npts, int ny, int pixel_step, int nimg, float* cur, float* traj,
                            int* tlen, int* num, int* flag)
{
    hipLaunchKernelGGL(k_traj_init, dim3((npts + 255) / 256 > 0 ? (npts + 255) / 256 : 1), dim3(256), 0, s, npts, ny,
                       pixel_step, nimg, cur, traj, tlen, num, flag);
    return hipGetLastError();
}

hipError_t launch_lk_chain(hipStream_t s, const LkArgs& a, const TrajChain& t, int ppw)
{
    const long long blocks = (long long)(t.nimg - 1) * ((a.npts + ppw - 1) / ppw);
    if (t.nimg < 2 || t.nimg > kMaxTrajImgs || a.npts <= 0 || blocks > 0x7fffffffLL || (ppw != 1 && ppw != 2 && ppw != 4))
        return hipErrorInvalidValue;
    if (ppw == 4) hipLaunchKernelGGL((k_lk<16, true>), dim3((unsigned)blocks), dim3(64), 0, s, a, t);
    else if (ppw == 2) hipLaunchKernelGGL((k_lk<32, true>), dim3((unsigned)blocks), dim3(64), 0, s, a, t);
    else hipLaunchKernelGGL((k_lk<64, true>), dim3((unsigned)blocks), dim3(64), 0, s, a, t);
    return hipGetLastError();
}

hipError_t launch_traj_update(hipStream_t s, int npts, const float* next_pts, const uint8_t* status, float* cur,
                              float* traj, int* tlen, int nimg, int w, int h, int last, double min_vector_size,
                              double* vectors, float* start_pts, int* num)
{
    if (npts <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_traj_update, dim3((npts + 255) / 256), dim3(256), 0, s, npts, next_pts, status, cur, traj,
                       tlen, nimg, w, h, last, min_vector_size, vectors, start_pts, num);
    return hipGetLastError();
}

hipError_t launch_lk(hipStream_t s, int batch, const LkArgs& a)
{
    // one point per wave: 124 VGPRs, 4 waves per SIMD (two points per wave took 172 VGPRs, 2 waves
    // per SIMD, and ran the trajectory passes 1.5x slower)
    constexpr int LPP = 64, PPW = 64 / LPP;
    const dim3 grid((a.npts + PPW - 1) / PPW, batch);
    hipLaunchKernelGGL((k_lk<LPP, false>), grid, dim3(64), 0, s, a, TrajChain{});
    return hipGetLastError();
}

}  // namespace mdx
