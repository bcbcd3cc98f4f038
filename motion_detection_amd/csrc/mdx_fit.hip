// mdx_fit.hip -- classification and the perspective fit, the RANSAC fit
// option and the row-band records, with their launchers.
// Every kernel reproduces the arithmetic of the OpenCV 2.4 routine the reference calls, bit for bit
// (integer stages exactly; float and double stages in the same evaluation order, compiled with
// -ffp-contract=off so no expression is fused into an FMA).
//
// The kernels, in launch order (launch_classify_fit; batch pairs of npts grid points, nblk blocks of
// 256 points each):
//   k_classify        one workgroup per block: the Vec4d of its points (optical_flow_calculator.cpp
//                     :78-117) -> vectors; accepted count and first four accepted indices ->
//                     BlockSummary.  Reads next_pts, status.
//   k_fit             one wave per pair: scan of the BlockSummary counts -> accepted total and the
//                     first four accepted points overall (the blocks are in the reference's point
//                     order); first-4: the whole wave solves getPerspectiveTransform on them
//                     (dev_perspective_fit_wave) and lane 0 writes the pair's PairFit; external H:
//                     the record from H_ext; RANSAC: count and status only, and each block's
//                     offset -> BlockSummary::ransac_off.
//   k_band_record     row bands, in k_fit's place: the same scan; count and first four points ->
//                     the band's mdx_band_cand.  No fit.
//   k_ransac_compact, k_ransac_hyp, k_ransac_score, k_ransac_pick
//                     MDX_FIT_RANSAC only, after k_fit: see the inventory above them.
//   k_band_fit        row bands, one wave (launch_band_fit): merges every band's record -> the
//                     frame's first four -> the same wave solve -> PairFit with the band's source rows.
//   k_set_fit_external, k_export_fit
//                     one thread per pair: PairFit from a given H (the warp-only entry); H and
//                     num_vectors of the PairFit records to the caller's arrays.
// Written once for all of them: grid_src / gather4 (grid index -> position, four correspondences),
// classify_point (the acceptance test), block_rank, scan_blocks, write_fitted / write_no_fit.
#include "mdx_internal.h"

#include <float.h>
#include <limits.h>

namespace mdx {

// ------------------------------------------------------------------ A7: perspective fit
// fdlibm __ieee754_hypot (what OpenCV's JacobiSVD reaches through ::hypot on glibc).
__device__ double dev_hypot(double x, double y)
{
    auto hi = [](double d) { return (int)(__double_as_longlong(d) >> 32); };
    auto lo = [](double d) { return (unsigned)(__double_as_longlong(d) & 0xffffffffll); };
    auto set_hi = [](double d, int h) {
        unsigned long long u = (unsigned long long)__double_as_longlong(d);
        u = ((unsigned long long)(unsigned)h << 32) | (u & 0xffffffffull);
        return __longlong_as_double((long long)u);
    };
    double a, b, t1, t2, y1, y2, w;
    int j, k, ha, hb;
    ha = hi(x) & 0x7fffffff;
    hb = hi(y) & 0x7fffffff;
    if (hb > ha) { a = y; b = x; j = ha; ha = hb; hb = j; }
    else { a = x; b = y; }
    a = set_hi(a, ha);
    b = set_hi(b, hb);
    if ((ha - hb) > 0x3c00000) return a + b;
    k = 0;
    if (ha > 0x5f300000) {
        if (ha >= 0x7ff00000) {
            w = a + b;
            if (((ha & 0xfffff) | lo(a)) == 0) w = a;
            if ((((unsigned)hb ^ 0x7ff00000u) | lo(b)) == 0) w = b;
            return w;
        }
        ha -= 0x25800000; hb -= 0x25800000; k += 600;
        a = set_hi(a, ha);
        b = set_hi(b, hb);
    }
    if (hb < 0x20b00000) {
        if (hb <= 0x000fffff) {
            if ((hb | (int)lo(b)) == 0) return a;
            t1 = set_hi(0.0, 0x7fd00000);
            b *= t1;
            a *= t1;
            k -= 1022;
        } else {
            ha += 0x25800000; hb += 0x25800000; k -= 600;
            a = set_hi(a, ha);
            b = set_hi(b, hb);
        }
    }
    w = a - b;
    if (w > b) {
        t1 = set_hi(0.0, ha);
        t2 = a - t1;
        w = __builtin_sqrt(t1 * t1 - (b * (-b) - t2 * (a + t1)));
    } else {
        a = a + a;
        y1 = set_hi(0.0, hb);
        y2 = b - y1;
        t1 = set_hi(0.0, ha + 0x00100000);
        t2 = a - t1;
        w = __builtin_sqrt(t1 * y1 - (w * (-w) - (t1 * y2 + t2 * b)));
    }
    if (k != 0) {
        t1 = set_hi(1.0, hi(1.0) + (k << 20));
        return t1 * w;
    }
    return w;
}

// The 8 x 8 DLT system of getPerspectiveTransform from four correspondences: rows i (x equations)
// and i + 4 (y equations); put(row, col, value) stores A[row][col], col 8 the right-hand side b[row].
// Entries it does not store are zero.
template <typename Put>
__device__ __forceinline__ void dlt_fill(const float* src, const float* dst, Put&& put)
{
    for (int i = 0; i < 4; i++) {
        const float sx = src[2 * i], sy = src[2 * i + 1], dx = dst[2 * i], dy = dst[2 * i + 1];
        put(i, 0, sx); put(i, 1, sy); put(i, 2, 1.0);
        put(i + 4, 3, sx); put(i + 4, 4, sy); put(i + 4, 5, 1.0);
        put(i, 6, (double)(-sx * dx));
        put(i, 7, (double)(-sy * dx));
        put(i + 4, 6, (double)(-sx * dy));
        put(i + 4, 7, (double)(-sy * dy));
        put(i, 8, dx);
        put(i + 4, 8, dy);
    }
}
// JacobiSVDImpl_'s rotation of two columns with squared norms aa, bb and dot product p
__device__ __forceinline__ double2 jacobi_rotation(double aa, double bb, double p)   // (c, s)
{
    p *= 2;
    const double beta = aa - bb, gamma = dev_hypot(p, beta);
    double c, s;
    if (beta < 0) {
        const double delta = (gamma - beta) * 0.5;
        s = __builtin_sqrt(delta / gamma);
        c = p / (gamma * s * 2);
    } else {
        c = __builtin_sqrt((gamma + beta) / (gamma * 2));
        s = p / (gamma * c * 2);
    }
    return make_double2(c, s);
}

// getPerspectiveTransform(src, dst) = solve(A, b, DECOMP_SVD) on the 8x8 DLT system:
// lapack.cpp JacobiSVDImpl_<double> (one-sided Jacobi on A's columns, eps 10*DBL_EPSILON,
// max(m,30) sweeps, descending sort) then SVBkSb (threshold 2*DBL_EPSILON*sum(w)).
// One lane runs this solve (k_ransac_hyp: one hypothesis per lane); its working arrays (At[64],
// Vt[64], W[8], bv[8], x[8]) live in LDS, lane-interleaved: lane l's element e at fw[e * S + l]
// (S = lanes, conflict-free across lanes).  As private arrays they were scratch memory.
// k_fit / k_band_fit run the wave-parallel form below (dev_perspective_fit_wave).
constexpr int kFitWorkDoubles = 152;
template <int S>
__device__ __forceinline__ void dev_perspective_fit_s(const float* src, const float* dst, double* M, double* fw)
{
#define AT(e) fw[(e) * S]
#define VT(e) fw[(64 + (e)) * S]
#define WV(e) fw[(128 + (e)) * S]
#define BV(e) fw[(136 + (e)) * S]
#define XV(e) fw[(144 + (e)) * S]
    for (int i = 0; i < 64; i++) AT(i) = 0.0;
    // A[r][c] stored as At[c*8 + r]
    dlt_fill(src, dst, [&](int r, int c, double v) {
        if (c == 8) BV(r) = v;
        else AT(c * 8 + r) = v;
    });
    const int m = 8, n = 8;
    const double eps = DBL_EPSILON * 10;
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const double t = AT(i * m + k); sd += t * t; }
        WV(i) = sd;
        for (int k = 0; k < n; k++) VT(i * n + k) = 0;
        VT(i * n + i) = 1;
    }
    for (int iter = 0; iter < 30; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                double aa = WV(i), p = 0, bb = WV(j);
                for (int k = 0; k < m; k++) p += AT(i * m + k) * AT(j * m + k);
                if (fabs(p) <= eps * __builtin_sqrt(aa * bb)) continue;
                const double2 cs = jacobi_rotation(aa, bb, p);
                const double c = cs.x, s = cs.y;
                aa = bb = 0;
                for (int k = 0; k < m; k++) {
                    const double ai = AT(i * m + k), aj = AT(j * m + k);
                    const double t0 = c * ai + s * aj;
                    const double t1 = -s * ai + c * aj;
                    AT(i * m + k) = t0; AT(j * m + k) = t1;
                    aa += t0 * t0; bb += t1 * t1;
                }
                WV(i) = aa; WV(j) = bb;
                changed = true;
                for (int k = 0; k < n; k++) {
                    const double vi = VT(i * n + k), vj = VT(j * n + k);
                    const double t0 = c * vi + s * vj;
                    const double t1 = -s * vi + c * vj;
                    VT(i * n + k) = t0; VT(j * n + k) = t1;
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const double t = AT(i * m + k); sd += t * t; }
        WV(i) = __builtin_sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++) if (WV(j) < WV(k)) j = k;
        if (i != j) {
            double t = WV(i); WV(i) = WV(j); WV(j) = t;
            for (int k = 0; k < m; k++) { t = AT(i * m + k); AT(i * m + k) = AT(j * m + k); AT(j * m + k) = t; }
            for (int k = 0; k < n; k++) { t = VT(i * n + k); VT(i * n + k) = VT(j * n + k); VT(j * n + k) = t; }
        }
    }
    // Left singular vectors: rows with W[i] <= DBL_MIN are skipped by the back-substitution
    // threshold below, so only the normalisation of the others matters.
    for (int i = 0; i < n; i++) {
        if (WV(i) <= DBL_MIN) continue;
        const double s = 1 / WV(i);
        for (int k = 0; k < m; k++) AT(i * m + k) *= s;
    }
    double threshold = 0;
    for (int i = 0; i < n; i++) { XV(i) = 0; threshold += WV(i); }
    threshold *= DBL_EPSILON * 2;
    for (int i = 0; i < n; i++) {
        double wi = WV(i);
        if (fabs(wi) <= threshold) continue;
        wi = 1 / wi;
        double s = 0;
        for (int j = 0; j < m; j++) s += AT(i * m + j) * BV(j);
        s *= wi;
        for (int j = 0; j < n; j++) XV(j) = XV(j) + s * VT(i * n + j);
    }
    for (int i = 0; i < 8; i++) M[i] = XV(i);
    M[8] = 1.;
#undef AT
#undef VT
#undef WV
#undef BV
#undef XV
}
// The same solve by one wave (k_fit, k_band_fit: every lane of a 64-lane workgroup calls it with
// the same src / dst).  Each rotation, and every other step, computes what dev_perspective_fit_s
// does, in the same order within each sum, so the result is bit-identical; what changes is the
// schedule.  Rotation (i, j) of sweep s (r-th in the reference's order) needs only the latest
// earlier rotations on columns i and j, which puts it at dependency depth 8 s + d_r (d_r = 0..12):
// depth L holds sweep L/8's rotations at d = L%8 and sweep L/8 - 1's at d = L%8 + 8, at most four,
// on disjoint columns (kJacSlot: i | j << 3 | previous-sweep << 6).  A sweep is complete at depth
// 8 s + 12; if it changed nothing, the next sweep's rotations already run saw the same columns and
// skipped too, so stopping there leaves the reference's state.
// Element-parallel rotations: slot q of a depth runs on the 16-lane DPP row q, lane e holding
// element e of A's column (e < 8) or element e - 8 of Vt's row (e >= 8) for both columns, so the
// update is one step; the 8-term dot products (p, and the new column norms) are summed in the
// reference's order from row_newbcast broadcasts of lanes 0..7 (v_mov_b64 DPP, then the add), and
// the scalar part (hypot, square roots, divisions) runs once per row.  The column-wise steps after
// the sweeps run one lane per column.  fw: kFitWaveDoubles of LDS.  M: the 9 entries, in every lane.
__constant__ uint8_t kJacSlot[8][4] = {{0x08, 0x7a, 0x73, 0x6c}, {0x10, 0x7b, 0x74, 0xff}, {0x18, 0x11, 0x7c, 0x75},
                                       {0x20, 0x19, 0x7d, 0xff}, {0x28, 0x21, 0x1a, 0x7e}, {0x30, 0x29, 0x22, 0xff},
                                       {0x38, 0x31, 0x2a, 0x23}, {0x39, 0x32, 0x2b, 0xff}};
constexpr int kFitWaveDoubles = 168;   // X 8 x 16 (A column | Vt row), W 8, b 8, s 8, use 8, x 8
constexpr int kJacSweeps = 30;

// ((((0 + v0) + v1) + ...) + v7) over lanes 0..7 of the lane's 16-lane DPP row: a column's sum in the
// reference's order.  The eight broadcasts (v_mov_b64 row_newbcast; v_add_f64 has no DPP form on
// gfx950) in one block behind s_nop 4: five wait states cover both DPP hazards, a VALU write of the
// source VGPR (two) and of EXEC (five), whatever the compiler schedules before the block.
__device__ __forceinline__ double rowsum8(double v)
{
    double b0, b1, b2, b3, b4, b5, b6, b7;
    asm volatile("s_nop 4\n\t"
                 "v_mov_b64_dpp %0, %8 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mov_b64_dpp %1, %8 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mov_b64_dpp %2, %8 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mov_b64_dpp %3, %8 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mov_b64_dpp %4, %8 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mov_b64_dpp %5, %8 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mov_b64_dpp %6, %8 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
                 "v_mov_b64_dpp %7, %8 row_newbcast:7 row_mask:0xf bank_mask:0xf"
                 : "=&v"(b0), "=&v"(b1), "=&v"(b2), "=&v"(b3), "=&v"(b4), "=&v"(b5), "=&v"(b6), "=&v"(b7)
                 : "v"(v));
    double s = 0.0;
    s = s + b0; s = s + b1; s = s + b2; s = s + b3;
    s = s + b4; s = s + b5; s = s + b6; s = s + b7;
    return s;
}

__device__ void dev_perspective_fit_wave(const float* src, const float* dst, double* M, double* fw)
{
    double* X = fw;           // X[c * 16 + k]: A[k][c] (k < 8), Vt[c][k - 8] (k >= 8)
    double* W = fw + 128;
    double* bv = fw + 136;
    double* sv = fw + 144;    // back-substitution coefficient of row i
    double* uv = fw + 152;    // 1: row i passes the threshold
    double* xv = fw + 160;
    const int lane = threadIdx.x & 63, q = lane >> 4, e = lane & 15;
    const double eps = DBL_EPSILON * 10;
    if (lane < 8) {
        const int c = lane;
        for (int k = 0; k < 16; k++) X[c * 16 + k] = k == 8 + c ? 1.0 : 0.0;
    }
    __syncthreads();
    if (lane == 0) {
        // A[r][c] at X[c * 16 + r]
        dlt_fill(src, dst, [&](int r, int c, double v) {
            if (c == 8) bv[r] = v;
            else X[c * 16 + r] = v;
        });
    }
    __syncthreads();
    if (lane < 8) {
        double sd = 0;
        for (int k = 0; k < 8; k++) { const double t = X[lane * 16 + k]; sd += t * t; }
        W[lane] = sd;
    }
    __syncthreads();
    bool chg_prev = false, chg_cur = false;
    for (int L = 0; L < 8 * (kJacSweeps - 1) + 13; L++) {
        const int ph = L & 7, sweep = L >> 3;
        const int ent = kJacSlot[ph][q];
        const bool prev = (ent >> 6) & 1;
        const int s_of = sweep - (int)prev;
        bool rot = false;
        if (ent != 0xff && s_of >= 0 && s_of < kJacSweeps) {   // uniform over the row
            const int i = ent & 7, j = (ent >> 3) & 7;
            const double xi = X[i * 16 + e], xj = X[j * 16 + e];
            const double aa0 = W[i], bb0 = W[j];
            double p = rowsum8(xi * xj);
            if (!(fabs(p) <= eps * __builtin_sqrt(aa0 * bb0))) {   // uniform over the row
                const double2 cs = jacobi_rotation(aa0, bb0, p);
                const double c = cs.x, s = cs.y;
                const double t0 = c * xi + s * xj;
                const double t1 = -s * xi + c * xj;
                X[i * 16 + e] = t0;
                X[j * 16 + e] = t1;
                const double aa = rowsum8(t0 * t0), bb = rowsum8(t1 * t1);
                if (e == 0) {
                    W[i] = aa;
                    W[j] = bb;
                }
                rot = true;
            }
        }
        chg_prev = chg_prev || __ballot(rot && prev) != 0;
        chg_cur = chg_cur || __ballot(rot && !prev) != 0;
        __syncthreads();
        if (ph == 4 && sweep >= 1 && !chg_prev) break;   // sweep - 1 complete, nothing changed
        if (ph == 7) { chg_prev = chg_cur; chg_cur = false; }
    }
    // singular values = column norms; descending selection sort (the reference's comparisons, on
    // every lane), applied as a permutation of the columns
    double w[8];
    int perm[8];
    if (lane < 8) {
        double sd = 0;
        for (int k = 0; k < 8; k++) { const double t = X[lane * 16 + k]; sd += t * t; }
        W[lane] = __builtin_sqrt(sd);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; i++) { w[i] = W[i]; perm[i] = i; }
#pragma unroll
    for (int i = 0; i < 7; i++) {
        int j = i;
        double wj = w[i];
#pragma unroll
        for (int k = i + 1; k < 8; k++)
            if (wj < w[k]) { j = k; wj = w[k]; }
        int pj = perm[i];
#pragma unroll
        for (int k = i + 1; k < 8; k++)
            if (k == j) pj = perm[k];
#pragma unroll
        for (int k = i + 1; k < 8; k++)
            if (k == j) { w[k] = w[i]; perm[k] = perm[i]; }
        w[i] = wj;
        perm[i] = pj;
    }
    double a[8], v[8];
    if (lane < 8) {
        int src_c = perm[0];
#pragma unroll
        for (int k = 1; k < 8; k++) if (lane == k) src_c = perm[k];
#pragma unroll
        for (int k = 0; k < 8; k++) { a[k] = X[src_c * 16 + k]; v[k] = X[src_c * 16 + 8 + k]; }
    }
    __syncthreads();
    double threshold = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) threshold += w[i];
    threshold *= DBL_EPSILON * 2;
    if (lane < 8) {
        double wl = w[0];
#pragma unroll
        for (int k = 1; k < 8; k++) if (lane == k) wl = w[k];
        // left singular vectors (rows with W <= DBL_MIN fail the threshold below anyway)
        if (!(wl <= DBL_MIN)) {
            const double s = 1 / wl;
#pragma unroll
            for (int k = 0; k < 8; k++) a[k] *= s;
        }
#pragma unroll
        for (int k = 0; k < 8; k++) X[lane * 16 + 8 + k] = v[k];
        const bool use = !(fabs(wl) <= threshold);
        double s = 0;
        if (use) {
            const double wi = 1 / wl;
#pragma unroll
            for (int k = 0; k < 8; k++) s += a[k] * bv[k];
            s *= wi;
        }
        sv[lane] = s;
        uv[lane] = use ? 1.0 : 0.0;
    }
    __syncthreads();
    if (lane < 8) {
        double x = 0;
#pragma unroll
        for (int i = 0; i < 8; i++)
            if (uv[i] != 0.0) x = x + sv[i] * X[i * 16 + 8 + lane];
        xv[lane] = x;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; i++) M[i] = xv[i];
    M[8] = 1.;
}

// lapack.cpp invert(DECOMP_LU) for 3x3 CV_64F: cofactors times 1/det3; det == 0 -> zeros.
__device__ void dev_invert3x3(const double* m, double* out)
{
    const double d0 = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) +
                      m[2] * (m[3] * m[7] - m[4] * m[6]);
    if (d0 != 0.) {
        const double d = 1. / d0;
        out[0] = (m[4] * m[8] - m[5] * m[7]) * d;
        out[1] = (m[2] * m[7] - m[1] * m[8]) * d;
        out[2] = (m[1] * m[5] - m[2] * m[4]) * d;
        out[3] = (m[5] * m[6] - m[3] * m[8]) * d;
        out[4] = (m[0] * m[8] - m[2] * m[6]) * d;
        out[5] = (m[2] * m[3] - m[0] * m[5]) * d;
        out[6] = (m[3] * m[7] - m[4] * m[6]) * d;
        out[7] = (m[1] * m[6] - m[0] * m[7]) * d;
        out[8] = (m[0] * m[4] - m[1] * m[3]) * d;
    } else {
        for (int i = 0; i < 9; i++) out[i] = 0.0;
    }
}

// ------------------------------------------------------------------ shared pieces
// Grid index -> grid position: the grid is x-major, point i at column i / ny, row i % ny.
__device__ __forceinline__ float2 grid_src(int i, int ny, int pixel_step)
{
    return make_float2((float)((i / ny) * pixel_step), (float)((i % ny) * pixel_step));
}

// The correspondence of grid point i of the pair whose points start at pair_base: src its grid
// position, dst where the LK left it; gather4: of the four points idx (getPerspectiveTransform's
// operands).
__device__ __forceinline__ void gather_point(const float* next_pts, long long pair_base, int ny, int pixel_step, int i,
                                             float* src, float* dst)
{
    const float2 s = grid_src(i, ny, pixel_step);
    const float2 e = reinterpret_cast<const float2*>(next_pts)[pair_base + i];
    src[0] = s.x;
    src[1] = s.y;
    dst[0] = e.x;
    dst[1] = e.y;
}
__device__ __forceinline__ void gather4(const float* next_pts, long long pair_base, int ny, int pixel_step,
                                        const int* idx, float* src, float* dst)
{
    for (int r = 0; r < 4; r++) gather_point(next_pts, pair_base, ny, pixel_step, idx[r], src + 2 * r, dst + 2 * r);
}

// The reference's classification of grid point i (optical_flow_calculator.cpp:78-117; o = the point's
// offset in next_pts / status) and its Vec4d: untracked (-1, -1, 0, 0); tracked with both float
// differences within min_vector_size (x, y, 0, 0); accepted (x, y, dx, dy).  Every kernel that asks
// takes this one: the RANSAC list and scores must accept exactly the points k_classify counted.
struct PointFlow {
    float2 s, e;      // grid position, tracked position
    bool accepted;
    double4 vec;
};
__device__ __forceinline__ PointFlow classify_point(const float* next_pts, const uint8_t* status, long long o, int i,
                                                    int ny, int pixel_step, double mvs)
{
    PointFlow p;
    p.s = grid_src(i, ny, pixel_step);
    p.e = reinterpret_cast<const float2*>(next_pts)[o];
    p.accepted = false;
    p.vec = make_double4(-1.0, -1.0, 0.0, 0.0);
    if (status[o]) {
        const float xd = p.e.x - p.s.x, yd = p.e.y - p.s.y;       // float differences (:82-83)
        p.accepted = fabs((double)fabsf(xd)) > mvs || fabs((double)fabsf(yd)) > mvs;
        p.vec = p.accepted ? make_double4(p.s.x, p.s.y, xd, yd) : make_double4(p.s.x, p.s.y, 0.0, 0.0);
    }
    return p;
}

// Rank of this thread's accepted point among the accepted points of its 256-point block (block
// order).  s_wcnt: 4 ints of LDS, the waves' counts.  Every thread of the block calls it; after it
// block_total(s_wcnt) is the block's number of accepted points.
__device__ __forceinline__ int block_rank(bool acc, int* s_wcnt)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long bal = __ballot(acc);
    if (lane == 0) s_wcnt[wave] = __popcll(bal);
    __syncthreads();
    int before = 0;
    for (int w2 = 0; w2 < wave; w2++) before += s_wcnt[w2];
    return before + __popcll(bal & ((1ull << lane) - 1ull));
}
__device__ __forceinline__ int block_total(const int* s_wcnt) { return s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3]; }

// One wave's scan over a pair's nblk block summaries S, 64 blocks at a time (block order = the
// reference's point order): the accepted total and the first four accepted points overall (-1 where
// there are fewer), both wave-uniform.  per_block(b, excl) runs in the lane of every block b with
// excl = the accepted points in the blocks before it.
struct BlockScan {
    int total;
    int pick[4];
};
template <typename Summary, typename PerBlock>
__device__ __forceinline__ BlockScan scan_blocks(Summary* S, int nblk, PerBlock&& per_block)
{
    const int lane = threadIdx.x;
    int carry = 0;          // accepted points in blocks before the current chunk
    int pick[4] = {-1, -1, -1, -1};
    for (int b0 = 0; b0 < nblk; b0 += 64) {
        const int b = b0 + lane;
        const int cnt = b < nblk ? S[b].count : 0;
        int incl = cnt;     // inclusive prefix over the chunk
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d);
            if (lane >= d) incl += t;
        }
        const int excl = carry + incl - cnt;
        if (b < nblk) per_block(b, excl);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            // the block holding overall rank r (one lane at most), then broadcast its index
            const bool here = cnt > 0 && r >= excl && r < excl + cnt;
            const unsigned long long m = __ballot(here);
            if (m) {
                const int src = __ffsll((long long)m) - 1;
                const int v = here ? S[b].first[r - excl] : 0;
                const int got = __shfl(v, src);
                if (pick[r] < 0) pick[r] = got;
            }
        }
        carry += __shfl(incl, 63);
    }
    return {carry, {pick[0], pick[1], pick[2], pick[3]}};
}

// A pair's record, by one thread: its matrices and status.  num_vectors stays with the callers (the
// scan's total; k_ransac_pick keeps k_fit's, k_set_fit_external has none).
// Fitted: H, the matrix the warp samples with, status 0.
__device__ __forceinline__ void write_fitted(PairFit& f, const double* H)
{
    for (int k = 0; k < 9; k++) f.H[k] = H[k];
    dev_invert3x3(H, f.Hinv);
    f.fit_status = 0;
}
// No fit (total < 4 accepted vectors): all-zero matrices (the warp then yields a zero mask), status 1 / 2.
__device__ __forceinline__ void write_no_fit(PairFit& f, int total)
{
    for (int k = 0; k < 9; k++) { f.H[k] = 0.0; f.Hinv[k] = 0.0; }
    f.fit_status = total == 0 ? 1 : 2;
}

// ------------------------------------------------------------------ A6 + A7: classify, first-4 fit
__global__ __launch_bounds__(256) void k_classify(const float* __restrict__ next_pts, const uint8_t* __restrict__ status,
                                                  int npts, int ny, int gy0, int gy1, int pixel_step, double mvs,
                                                  double* __restrict__ vectors, BlockSummary* __restrict__ summ)
{
    const int pair = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    __shared__ int s_wcnt[4];
    const int i = blk * 256 + tid;
    bool acc = false;
    const int gyi = i % ny;
    if (i < npts && gyi >= gy0 && gyi < gy1) {   // grid rows of the band (all rows: the full path)
        const PointFlow p = classify_point(next_pts, status, (long long)pair * npts + i, i, ny, pixel_step, mvs);
        acc = p.accepted;
        if (vectors) reinterpret_cast<double4*>(vectors)[(long long)pair * npts + i] = p.vec;
    }
    const int rank = block_rank(acc, s_wcnt);
    BlockSummary& S = summ[(long long)pair * gridDim.x + blk];
    if (acc && rank < 4) S.first[rank] = i;
    if (tid == 0) S.count = block_total(s_wcnt);
}

__global__ __launch_bounds__(64) void k_fit(const float* __restrict__ next_pts, int npts, int ny, int pixel_step,
                                            BlockSummary* __restrict__ summ, int nblk, PairFit* __restrict__ fits,
                                            int fit_mode, const double* __restrict__ H_ext)
{
    const int pair = blockIdx.x, lane = threadIdx.x;
    BlockSummary* S = summ + (long long)pair * nblk;
    const BlockScan scan = scan_blocks(S, nblk, [&](int b, int excl) {
        if (fit_mode == MDX_FIT_RANSAC) S[b].ransac_off = excl;   // k_ransac_compact's block offsets
    });
    // the scan's result is wave-uniform: the whole wave runs the fit, lane 0 writes the record
    __shared__ double fw[kFitWaveDoubles];
    PairFit& f = fits[pair];
    const int total = scan.total;
    if (fit_mode != MDX_FIT_EXTERNAL && fit_mode != MDX_FIT_RANSAC && total >= 4) {
        float src[8], dst[8];
        gather4(next_pts, (long long)pair * npts, ny, pixel_step, scan.pick, src, dst);
        double H[9];
        dev_perspective_fit_wave(src, dst, H, fw);
        if (lane != 0) return;
        write_fitted(f, H);
        f.num_vectors = total;
        return;
    }
    if (lane != 0) return;
    f.num_vectors = total;
    if (fit_mode == MDX_FIT_EXTERNAL) write_fitted(f, H_ext + (long long)pair * 9);
    else if (fit_mode == MDX_FIT_RANSAC && total >= 4) f.fit_status = 0;   // H / Hinv: k_ransac_pick
    else write_no_fit(f, total);
}

// ------------------------------------------------------------------ MDX_FIT_RANSAC (not in the reference)
// Deterministic RANSAC over every accepted vector (include/mdx.h MDX_FIT_RANSAC, DESIGN.md §7d;
// restated by oracle/mdx_oracle.c ora_fit_ransac, which the GPU equals bit for bit):
//   k_ransac_compact  the accepted vectors' grid indices in x-major order (the reference's
//                     src / dst order, optical_flow_calculator.cpp:78-117), from k_fit's block offsets
//   k_ransac_hyp      one lane per hypothesis: 4 distinct draws from splitmix64(seed, h, draw, retry)
//                     and the reference's getPerspectiveTransform on them (dev_perspective_fit_s,
//                     the lane's working set interleaved in LDS)
//   k_ransac_score    every accepted vector against every hypothesis: inlier iff
//                     |H src - dst * w|^2 <= t^2 w^2 in FP64 (w the projective denominator), counts
//                     added per workgroup
//   k_ransac_pick     the hypothesis with the most inliers (lowest index on ties), its inverse
__device__ __forceinline__ uint64_t ransac_mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void k_ransac_compact(const float* __restrict__ next_pts,
                                                        const uint8_t* __restrict__ status, int npts, int ny,
                                                        int pixel_step, double mvs,
                                                        const BlockSummary* __restrict__ summ, int* __restrict__ list)
{
    const int pair = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    __shared__ int s_wcnt[4];
    const int i = blk * 256 + tid;
    const bool acc = i < npts &&
        classify_point(next_pts, status, (long long)pair * npts + i, i, ny, pixel_step, mvs).accepted;
    const int rank = block_rank(acc, s_wcnt);
    const int off = summ[(long long)pair * gridDim.x + blk].ransac_off;
    if (acc) list[(long long)pair * npts + off + rank] = i;
}

constexpr int kRansacLanes = 32;   // hypotheses per workgroup (LDS: 32 interleaved fit working sets)
__global__ __launch_bounds__(64) void k_ransac_hyp(const float* __restrict__ next_pts, int npts, int ny, int pixel_step,
                                                   const int* __restrict__ list, const PairFit* __restrict__ fits,
                                                   int iters, uint32_t seed, double* __restrict__ hyps,
                                                   int* __restrict__ counts)
{
    __shared__ double s_fw[kFitWorkDoubles * kRansacLanes];
    const int pair = blockIdx.y, lane = threadIdx.x, h = blockIdx.x * kRansacLanes + lane;
    if (lane >= kRansacLanes || h >= iters) return;
    counts[(long long)pair * iters + h] = 0;
    const int n = fits[pair].num_vectors;
    if (fits[pair].fit_status != 0 || n < 4) return;
    int idx[4];
    for (int j = 0; j < 4; j++) {
        for (uint32_t c = 0;; c++) {
            const uint64_t x = ((uint64_t)seed << 32) | ((uint64_t)h << 20) | ((uint64_t)j << 16) | (uint64_t)(c & 0xffffu);
            const int v = (int)(ransac_mix64(x) % (uint64_t)n);
            bool dup = false;
            for (int q = 0; q < j; q++) dup = dup || idx[q] == v;
            if (!dup || c >= 0xffffu) {
                idx[j] = v;
                break;
            }
        }
    }
    for (int j = 0; j < 4; j++) idx[j] = list[(long long)pair * npts + idx[j]];   // draw -> grid index
    float src[8], dst[8];
    gather4(next_pts, (long long)pair * npts, ny, pixel_step, idx, src, dst);
    double Hh[9];
    dev_perspective_fit_s<kRansacLanes>(src, dst, Hh, s_fw + lane);
    for (int k = 0; k < 9; k++) hyps[((long long)pair * iters + h) * 9 + k] = Hh[k];
}

__global__ __launch_bounds__(256) void k_ransac_score(const float* __restrict__ next_pts,
                                                     const uint8_t* __restrict__ status, int npts, int ny,
                                                     int pixel_step, double mvs, const double* __restrict__ hyps,
                                                     int iters, double t2, const PairFit* __restrict__ fits,
                                                     int* __restrict__ counts)
{
    __shared__ int s_cnt[kRansacMaxIters];
    const int pair = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    if (fits[pair].fit_status != 0 || fits[pair].num_vectors < 4) return;   // uniform per workgroup
    for (int h = tid; h < iters; h += 256) s_cnt[h] = 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + tid;
    bool acc = false;
    double sx = 0.0, sy = 0.0, dx = 0.0, dy = 0.0;
    if (i < npts) {
        const PointFlow p = classify_point(next_pts, status, (long long)pair * npts + i, i, ny, pixel_step, mvs);
        acc = p.accepted;
        sx = p.s.x; sy = p.s.y; dx = p.e.x; dy = p.e.y;
    }
    const double* Hp = hyps + (long long)pair * iters * 9;
    for (int h = 0; h < iters; h++) {
        const double* H = Hp + 9 * h;                 // uniform: scalar loads
        const double nx = H[0] * sx + H[1] * sy + H[2];
        const double nyv = H[3] * sx + H[4] * sy + H[5];
        const double dd = H[6] * sx + H[7] * sy + H[8];
        const double ex = nx - dx * dd, ey = nyv - dy * dd;
        const bool in = acc && ex * ex + ey * ey <= t2 * (dd * dd);
        const unsigned long long bal = __ballot(in);
        if (lane == 0 && bal) atomicAdd(&s_cnt[h], __popcll(bal));
    }
    __syncthreads();
    for (int h = tid; h < iters; h += 256)
        if (s_cnt[h]) atomicAdd(&counts[(long long)pair * iters + h], s_cnt[h]);
}

__global__ __launch_bounds__(64) void k_ransac_pick(const double* __restrict__ hyps, const int* __restrict__ counts,
                                                    int iters, PairFit* __restrict__ fits)
{
    const int pair = blockIdx.x, lane = threadIdx.x;
    PairFit& f = fits[pair];
    if (f.fit_status != 0 || f.num_vectors < 4) return;
    int bc = -1, bh = 0;
    for (int h = lane; h < iters; h += 64) {
        const int cnt = counts[(long long)pair * iters + h];
        if (cnt > bc) { bc = cnt; bh = h; }            // first max of this lane's (increasing) h
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const int oc = __shfl_xor(bc, m), oh = __shfl_xor(bh, m);
        if (oc > bc || (oc == bc && oh < bh)) { bc = oc; bh = oh; }
    }
    if (lane != 0) return;
    write_fitted(f, hyps + ((long long)pair * iters + bh) * 9);   // status is 0 already, the count k_fit's
}

// Row-band mode: the same block scan as k_fit, but the band's count and first four accepted
// points go to its record (the fit waits for every band's record, k_band_fit).
__global__ __launch_bounds__(64) void k_band_record(const float* __restrict__ next_pts, int npts, int ny, int pixel_step,
                                                    const BlockSummary* __restrict__ summ, int nblk,
                                                    mdx_band_cand* __restrict__ cand)
{
    const int pair = blockIdx.x, lane = threadIdx.x;
    const BlockScan scan = scan_blocks(summ + (long long)pair * nblk, nblk, [](int, int) {});
    if (lane != 0) return;
    mdx_band_cand& c = cand[pair];
    const int n = scan.total < 4 ? scan.total : 4;
    c.count = scan.total;
    c.n = n;
    for (int r = 0; r < 4; r++) {
        const int i = r < n ? scan.pick[r] : -1;
        c.idx[r] = i;
        if (i >= 0) gather_point(next_pts, (long long)pair * npts, ny, pixel_step, i, c.src + 2 * r, c.dst + 2 * r);
        else c.src[2 * r] = c.src[2 * r + 1] = c.dst[2 * r] = c.dst[2 * r + 1] = 0.f;
    }
    c.pad_[0] = c.pad_[1] = 0;
}

// Merge the bands' records: the four smallest indices over all records are the frame's first four
// accepted points (each band lists its own first four, and bands partition the points), so the
// fit below is bit-identical to the full path's k_fit.
// Frame-1 rows the warp of destination rows [y0, y1) reads: under M (= Hinv) a rectangle whose
// corners all have W of one sign maps to the convex quadrilateral of the corners' images, so
// their Y bound the source rows (+-2 for the reference's 1/32-px rounding and the lower tap);
// otherwise every row.  M all zero (singular fit): the constant warp reads row 0 (and 1).
__device__ void band_source_rows(const double* M, int w, int h, int y0, int y1, int& r0, int& r1)
{
    bool zero = true;
    for (int k = 0; k < 9; k++) zero = zero && M[k] == 0.0;
    r0 = 0;
    r1 = h;
    if (zero) {
        r1 = min(h, 2);
        return;
    }
    double ymin = 0.0, ymax = 0.0;
    int sgn = 0;
    for (int q = 0; q < 4; q++) {
        const double x = (q & 1) ? (double)(w - 1) : 0.0, y = (q & 2) ? (double)(y1 - 1) : (double)y0;
        const double W = M[6] * x + M[7] * y + M[8];
        const int sq = W > 0.0 ? 1 : W < 0.0 ? -1 : 0;
        if (sq == 0 || (q && sq != sgn)) return;
        sgn = sq;
        const double Y = (M[3] * x + M[4] * y + M[5]) / W;
        if (!(Y == Y) || __builtin_isinf(Y)) return;
        ymin = q ? fmin(ymin, Y) : Y;
        ymax = q ? fmax(ymax, Y) : Y;
    }
    if (ymax < -4.0 || ymin > (double)h + 4.0) {   // footprint outside the frame: nothing to read
        r0 = r1 = 0;
        return;
    }
    r0 = (int)fmax(0.0, floor(ymin) - 2.0);
    r1 = (int)fmin((double)h, floor(ymax) + 3.0);
    if (r1 < r0) r1 = r0;
}

__global__ __launch_bounds__(64) void k_band_fit(const mdx_band_cand* __restrict__ cands, int nrec,
                                                 PairFit* __restrict__ fit, int w, int h, int y0, int y1)
{
    // every lane merges the records (uniform loads), the wave runs the fit, lane 0 writes
    int total = 0;
    int best[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX};
    float bs[8] = {}, bd[8] = {};
    for (int r = 0; r < nrec; r++) {
        const mdx_band_cand& c = cands[r];
        total += c.count;
        for (int q = 0; q < c.n && q < 4; q++) {
            int i = c.idx[q];
            float sx = c.src[2 * q], sy = c.src[2 * q + 1], dx = c.dst[2 * q], dy = c.dst[2 * q + 1];
            for (int k = 0; k < 4; k++) {   // insertion into the sorted four
                if (i < best[k]) {
                    const int ti = best[k];
                    const float t0 = bs[2 * k], t1 = bs[2 * k + 1], t2 = bd[2 * k], t3 = bd[2 * k + 1];
                    best[k] = i; bs[2 * k] = sx; bs[2 * k + 1] = sy; bd[2 * k] = dx; bd[2 * k + 1] = dy;
                    i = ti; sx = t0; sy = t1; dx = t2; dy = t3;
                }
            }
        }
    }
    PairFit& f = *fit;
    __shared__ double fw[kFitWaveDoubles];
    if (total >= 4) {
        double H[9];
        dev_perspective_fit_wave(bs, bd, H, fw);
        if (threadIdx.x != 0) return;
        write_fitted(f, H);
        band_source_rows(f.Hinv, w, h, y0, y1, f.src_y0, f.src_y1);
    } else {
        if (threadIdx.x != 0) return;
        write_no_fit(f, total);
        f.src_y0 = f.src_y1 = 0;   // no warp (zero mask)
    }
    f.num_vectors = total;
}

__global__ void k_set_fit_external(const double* __restrict__ H_ext, PairFit* __restrict__ fits, int batch)
{
    const int pair = blockIdx.x * blockDim.x + threadIdx.x;
    if (pair >= batch) return;
    write_fitted(fits[pair], H_ext + (long long)pair * 9);
    fits[pair].num_vectors = 0;
}

__global__ void k_export_fit(const PairFit* __restrict__ fits, int batch, double* H, int* num)
{
    const int pair = blockIdx.x * blockDim.x + threadIdx.x;
    if (pair >= batch) return;
    if (H) for (int k = 0; k < 9; k++) H[(long long)pair * 9 + k] = fits[pair].H[k];
    if (num) num[pair] = fits[pair].num_vectors;
}

hipError_t launch_classify_fit(hipStream_t s, int batch, const FitArgs& a)
{
    const int npts = a.npts, ny = a.ny, ps = a.pixel_step, nblk = classify_blocks(npts);
    const double mvs = a.min_vector_size;
    BlockSummary* summ = reinterpret_cast<BlockSummary*>(a.scratch);
    if (nblk > 0)
        hipLaunchKernelGGL(k_classify, dim3(nblk, batch), dim3(256), 0, s, a.next_pts, a.status, npts, ny, a.gy0, a.gy1,
                           ps, mvs, a.vectors, summ);
    if (a.cand)
        hipLaunchKernelGGL(k_band_record, dim3(batch), dim3(64), 0, s, a.next_pts, npts, ny, ps, summ, nblk, a.cand);
    else
        hipLaunchKernelGGL(k_fit, dim3(batch), dim3(64), 0, s, a.next_pts, npts, ny, ps, summ, nblk, a.fits, a.fit_mode,
                           a.H_external);
    if (a.fit_mode == MDX_FIT_RANSAC && !a.cand) {
        const RansacArgs& r = a.ransac;
        if (!r.list || nblk == 0 || r.iters < 1 || r.iters > kRansacMaxIters) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_ransac_compact, dim3(nblk, batch), dim3(256), 0, s, a.next_pts, a.status, npts, ny, ps, mvs,
                           summ, r.list);
        hipLaunchKernelGGL(k_ransac_hyp, dim3((r.iters + kRansacLanes - 1) / kRansacLanes, batch), dim3(64), 0, s,
                           a.next_pts, npts, ny, ps, r.list, a.fits, r.iters, r.seed, r.hyps, r.counts);
        hipLaunchKernelGGL(k_ransac_score, dim3(nblk, batch), dim3(256), 0, s, a.next_pts, a.status, npts, ny, ps, mvs,
                           r.hyps, r.iters, r.thresh * r.thresh, a.fits, r.counts);
        hipLaunchKernelGGL(k_ransac_pick, dim3(batch), dim3(64), 0, s, r.hyps, r.counts, r.iters, a.fits);
    }
    return hipGetLastError();
}

hipError_t launch_band_fit(hipStream_t s, int nrec, const mdx_band_cand* cands, PairFit* fit, int w, int h, int y0,
                           int y1)
{
    hipLaunchKernelGGL(k_band_fit, dim3(1), dim3(64), 0, s, cands, nrec, fit, w, h, y0, y1);
    return hipGetLastError();
}

hipError_t launch_set_fit_external(hipStream_t s, int batch, const double* H_external, PairFit* fits)
{
    hipLaunchKernelGGL(k_set_fit_external, dim3((batch + 63) / 64), dim3(64), 0, s, H_external, fits, batch);
    return hipGetLastError();
}

hipError_t launch_export_fit(hipStream_t s, int batch, const PairFit* fits, double* H, int* num)
{
    hipLaunchKernelGGL(k_export_fit, dim3((batch + 63) / 64), dim3(64), 0, s, fits, batch, H, num);
    return hipGetLastError();
}

}  // namespace mdx
