// mdx_hull.hip -- convex hulls of the kept clusters (showClusterContours' cv::convexHull).
//
// k_hull: one workgroup per requested cluster, one launch per call.
//   Stage 1  the members, streamed once from HBM and converted with cv_round, leave per pixel column
//            col = x - xmin the lowest and the highest y in LDS (ds_min_i32 / ds_max_i32): after the
//            conversion no other member of a column can be a hull vertex.  No sort.
//   Stage 2  the non-empty columns, in x order, are two x-monotone candidate chains (max y, min y), kept
//            as lists of column indices.  A round removes every candidate that does not turn strictly
//            the right way between its current neighbours -- all of them at once: a candidate on or under
//            the segment between two members is never a vertex -- and compacts both lists in place by one
//            workgroup scan.  Rounds end when one removes nothing.
//   Tail     rounds are bounded by kHullRounds: an input whose candidates become removable one per round
//            ((x, -x^2) under one far point: 8,191 rounds) is finished by a sequential monotone chain,
//            one lane per list, over what the rounds left -- O(columns) whatever the input.
//   Output   the vertices in cv::convexHull(.., clockwise=false)'s order into the cluster's own slice
//            of the staging block (8-byte stores), the vertex count by one lane.
// All arithmetic is integer and exact: cross products of (column, y) differences in int64.
#include "mdx_dev.h"

namespace mdx {

namespace {

constexpr int kHullT = 1024;                         // threads of k_hull
constexpr int kHullE = MDX_HULL_MAX_SPAN / kHullT;   // list entries (and columns) a lane owns per pass
constexpr int kHullRounds = 32;                      // simultaneous rounds before the sequential tail
static_assert(kHullE * kHullT == MDX_HULL_MAX_SPAN, "a pass covers every column");
static_assert(MDX_HULL_MAX_SPAN <= 65536, "column indices are stored as uint16");

// (b - a) x (c - a) of candidates given as (column, y): < 0 where b lies strictly above a -> c
__device__ __forceinline__ long long hull_cross(int ax, int ay, int bx, int by, int cx, int cy)
{
    return (long long)(bx - ax) * ((long long)cy - ay) - ((long long)by - ay) * (long long)(cx - ax);
}

// One round on one list: the owned entries' keep flags.  y: the list's column extremes; up: the
// max-y chain (keep on cross < 0), else the min-y chain (keep on cross > 0).
__device__ __forceinline__ int hull_round_flags(const uint16_t* __restrict__ idx, int len, const int* __restrict__ y,
                                                bool up, uint16_t (&own)[kHullE])
{
    const int base = (int)threadIdx.x * kHullE;
    int keep = 0;
    if (base >= len) return 0;
    int px = base > 0 ? idx[base - 1] : 0, py = base > 0 ? y[px] : 0;
    int cx = idx[base], cy = y[cx];
#pragma unroll
    for (int j = 0; j < kHullE; j++) {
        const int p = base + j;
        if (p >= len) break;
        own[j] = (uint16_t)cx;
        int nx = 0, ny = 0;
        bool k = true;
        if (p + 1 < len) {
            nx = idx[p + 1];
            ny = y[nx];
            if (p > 0) {
                const long long o = hull_cross(px, py, cx, cy, nx, ny);
                k = up ? o < 0 : o > 0;
            }
        }
        keep |= (int)k << j;
        px = cx, py = cy, cx = nx, cy = ny;
    }
    return keep;
}

// the kept entries of `own`, written from position `pos` on
__device__ __forceinline__ void hull_compact(uint16_t* __restrict__ idx, int pos, int keep, const uint16_t (&own)[kHullE])
{
#pragma unroll
    for (int j = 0; j < kHullE; j++)
        if (keep >> j & 1) idx[pos++] = own[j];
}

// Sequential monotone chain over idx[0 .. len), in place (the stack never passes the read position);
// returns the new length.  One lane.
__device__ int hull_chain_tail(uint16_t* __restrict__ idx, int len, const int* __restrict__ y, bool up)
{
    int top = 0, ax = 0, ay = 0, bx = 0, by = 0;      // a, b: the stack's two top entries, kept in registers
    for (int i = 0; i < len; i++) {
        const int cx = idx[i], cy = y[cx];
        while (top >= 2) {
            const long long o = hull_cross(ax, ay, bx, by, cx, cy);
            if (up ? o < 0 : o > 0) break;
            top--;                                    // b goes; only a pop reads the stack back
            bx = ax, by = ay;
            if (top >= 2) ax = idx[top - 2], ay = y[ax];
        }
        idx[top++] = (uint16_t)cx;
        ax = bx, ay = by, bx = cx, by = cy;
    }
    return top;
}

}  // namespace

__global__ __launch_bounds__(kHullT) void k_hull(const HullCluster* __restrict__ recs, const float2* __restrict__ pts,
                                                 int ncols_lds, int32_t* __restrict__ counts, int2* __restrict__ staging)
{
    extern __shared__ int32_t hull_lds[];
    __shared__ int wsum[kHullT / 64];
    __shared__ int tail_len[2];
    const int tid = threadIdx.x;
    const HullCluster R = recs[blockIdx.x];
    const int ncols = min(R.ncols, ncols_lds);        // the host sized the LDS for the widest cluster
    int32_t* ymin = hull_lds;
    int32_t* ymax = ymin + ncols_lds;
    uint16_t* up = reinterpret_cast<uint16_t*>(ymax + ncols_lds);
    uint16_t* lo = up + ncols_lds;

    for (int c = tid; c < ncols; c += kHullT) {
        ymin[c] = INT32_MAX;
        ymax[c] = INT32_MIN;
    }
    __syncthreads();
    const float2* p = pts + R.start;
#pragma unroll 4
    for (int i = tid; i < R.count; i += kHullT) {
        const float2 v = p[i];
        const int col = cv_round(v.x) - R.xmin, yi = cv_round(v.y);
        if ((unsigned)col < (unsigned)ncols) {
            atomicMin(&ymin[col], yi);
            atomicMax(&ymax[col], yi);
        }
    }
    __syncthreads();

    // the non-empty columns, in order, start both lists
    int keep = 0;
    uint16_t own_u[kHullE], own_l[kHullE];
#pragma unroll
    for (int j = 0; j < kHullE; j++) {
        const int c = tid * kHullE + j;
        own_u[j] = (uint16_t)c;
        if (c < ncols && ymax[c] != INT32_MIN) keep |= 1 << j;
    }
    int total;
    int pos = block_scan_exclusive<kHullT>(__popc(keep), wsum, total);
    {
        int q = pos;
#pragma unroll
        for (int j = 0; j < kHullE; j++)
            if (keep >> j & 1) up[q] = lo[q] = own_u[j], q++;
    }
    int nu = total, nl = total;
    __syncthreads();

    for (int round = 0;; round++) {
        if (round == kHullRounds) {                   // the tail: one lane of two waves
            if (tid == 0) tail_len[0] = hull_chain_tail(up, nu, ymax, true);
            if (tid == 64) tail_len[1] = hull_chain_tail(lo, nl, ymin, false);
            __syncthreads();
            nu = tail_len[0], nl = tail_len[1];
            break;
        }
        const int ku = hull_round_flags(up, nu, ymax, true, own_u);
        const int kl = hull_round_flags(lo, nl, ymin, false, own_l);
        // both lists' counts through one scan: each total is at most 8192 < 2^16
        pos = block_scan_exclusive<kHullT>(__popc(ku) | __popc(kl) << 16, wsum, total);
        // every lane has read its entries and neighbours (the scan's barriers): compact in place
        hull_compact(up, pos & 0xffff, ku, own_u);
        hull_compact(lo, pos >> 16, kl, own_l);
        __syncthreads();
        const int mu = total & 0xffff, ml = total >> 16;
        const bool done = mu == nu && ml == nl;
        nu = mu, nl = ml;
        if (done) break;
    }

    // cv::convexHull(.., clockwise=false): from the greatest vertex (x, then y) along the max-y side to
    // the smallest, then along the min-y side back; an end column with one distinct y counts once
    if (nu < 1) {                                     // a cluster without members (the host rejects it)
        if (tid == 0) counts[blockIdx.x] = 0;
        return;
    }
    const int c0 = up[0], c1 = up[nu - 1];
    const int skip0 = ymin[c0] == ymax[c0], skip1 = nl > 1 && ymin[c1] == ymax[c1];   // nl == 1: one column
    const int nv = nu + nl - skip0 - skip1;
    int2* out = staging + R.out_off;
    for (int i = tid; i < nu; i += kHullT) {
        const int c = up[i], o = nu - 1 - i;
        if (o < R.bound) out[o] = make_int2(R.xmin + c, ymax[c]);
    }
    for (int i = tid; i < nl; i += kHullT) {
        if ((i == 0 && skip0) || (i == nl - 1 && skip1)) continue;
        const int c = lo[i], o = nu + i - skip0;
        if (o < R.bound) out[o] = make_int2(R.xmin + c, ymin[c]);
    }
    if (tid == 0) counts[blockIdx.x] = nv;
}

size_t hull_lds_bytes(int ncols) { return (size_t)((ncols + 63) / 64 * 64) * 12; }

hipError_t launch_hull(hipStream_t s, int k, const HullCluster* recs, const float* pts, int max_ncols,
                       int32_t* counts, int32_t* staging)
{
    if (k <= 0) return hipSuccess;
    const int ncols_lds = (max_ncols + 63) / 64 * 64;
    const size_t lds = hull_lds_bytes(max_ncols);
    if (lds > 32 * 1024)                              // with the static part, above the 64 KB default at 8192 columns
        if (hipError_t e = hipFuncSetAttribute((const void*)k_hull, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
            return e;
    hipLaunchKernelGGL(k_hull, dim3((unsigned)k), dim3(kHullT), lds, s, recs, reinterpret_cast<const float2*>(pts),
                       ncols_lds, counts, reinterpret_cast<int2*>(staging));
    return hipGetLastError();
}

}  // namespace mdx
