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
//
// k_region_hull: the same for the mask regions of mdx_mask_regions_dev.  Its stage 1 scans
// the record's rectangle in the label image; stage 2, the tail and the output are k_hull's, written once
// (hull_chains).  k_region_hull_slices in front of it and k_region_hull_pack behind it place and pack the
// hulls on the device, since the host never learns the counts.
#include "mdx_dev.h"

#include <algorithm>

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

// The dynamic LDS of both kernels, for ncols_lds columns: the column extremes, then the two lists.
struct HullLds {
    int32_t *ymin, *ymax;
    uint16_t *up, *lo;
};
__device__ __forceinline__ HullLds hull_lds_layout(int32_t* base, int ncols_lds)
{
    HullLds L;
    L.ymin = base;
    L.ymax = L.ymin + ncols_lds;
    L.up = reinterpret_cast<uint16_t*>(L.ymax + ncols_lds);
    L.lo = L.up + ncols_lds;
    return L;
}

// Stage 2, the tail and the output of one hull, by the whole workgroup (every lane calls it, behind the
// barrier that ends stage 1).  L.ymin / L.ymax [ncols]: each column's lowest and highest member y,
// INT32_MAX / INT32_MIN where the column is empty; xmin: column 0's x.  The ordered vertices go to out,
// those from `bound` on are dropped; returns the vertex count, dropped ones included (0: no member).
// wsum: kHullT / 64 ints, tail_len: 2 ints of LDS.
__device__ __forceinline__ int hull_chains(const HullLds& L, int ncols, int xmin, int* wsum, int* tail_len,
                                           int2* __restrict__ out, int bound)
{
    const int tid = threadIdx.x;
    const int32_t *ymin = L.ymin, *ymax = L.ymax;
    uint16_t *up = L.up, *lo = L.lo;

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
    if (nu < 1) return 0;                             // no member: a region record whose id has no pixel
    const int c0 = up[0], c1 = up[nu - 1];
    const int skip0 = ymin[c0] == ymax[c0], skip1 = nl > 1 && ymin[c1] == ymax[c1];   // nl == 1: one column
    for (int i = tid; i < nu; i += kHullT) {
        const int c = up[i], o = nu - 1 - i;
        if (o < bound) out[o] = make_int2(xmin + c, ymax[c]);
    }
    for (int i = tid; i < nl; i += kHullT) {
        if ((i == 0 && skip0) || (i == nl - 1 && skip1)) continue;
        const int c = lo[i], o = nu + i - skip0;
        if (o < bound) out[o] = make_int2(xmin + c, ymin[c]);
    }
    return nu + nl - skip0 - skip1;
}

// A region record's rectangle clamped to the frame (the entry cannot validate device records): columns
// [x0, x1), rows [y0, y1), empty where a side is not positive.  `bound`: no hull of members inside it has
// more vertices -- at most two per column and per row, and no more than the record claims as its area.
struct RegionBox {
    int x0, y0, x1, y1, bound;
};
__device__ __forceinline__ RegionBox region_box(const mdx_region& R, int w, int h)
{
    RegionBox B;
    B.x0 = min(max(R.x, 0), w);
    B.y0 = min(max(R.y, 0), h);
    B.x1 = (int)min(max((long long)R.x + R.width, (long long)B.x0), (long long)w);
    B.y1 = (int)min(max((long long)R.y + R.height, (long long)B.y0), (long long)h);
    const long long cw = B.x1 - B.x0, ch = B.y1 - B.y0;
    B.bound = (int)min(min(2 * cw, 2 * ch), min(cw * ch, (long long)max(R.area, 0)));
    return B;
}

constexpr int kRegionRows = 16;                      // label rows a lane has in flight

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
    const HullLds L = hull_lds_layout(hull_lds, ncols_lds);

    for (int c = tid; c < ncols; c += kHullT) {
        L.ymin[c] = INT32_MAX;
        L.ymax[c] = INT32_MIN;
    }
    __syncthreads();
    const float2* p = pts + R.start;
#pragma unroll 4
    for (int i = tid; i < R.count; i += kHullT) {
        const float2 v = p[i];
        const int col = cv_round(v.x) - R.xmin, yi = cv_round(v.y);
        if ((unsigned)col < (unsigned)ncols) {
            atomicMin(&L.ymin[col], yi);
            atomicMax(&L.ymax[col], yi);
        }
    }
    __syncthreads();
    const int nv = hull_chains(L, ncols, R.xmin, wsum, tail_len, staging + R.out_off, R.bound);
    if (tid == 0) counts[blockIdx.x] = nv;
}

// ---- the mask regions' hulls (mdx_region_hulls_dev): three launches, ordered by their
// boundaries alone -- no workgroup waits for another.

// Launch 1, one workgroup per image: each taking-part record's slice of the image's staging block,
// (first vertex, vertices), from the exclusive scan of the records' bounds.  Slices end at `cap`, the
// block's size, whatever the records claim.
__global__ __launch_bounds__(kHullT) void k_region_hull_slices(const mdx_region* __restrict__ regions, int max_regions,
                                                               const int32_t* __restrict__ num_kept, int w, int h, int cap,
                                                               int2* __restrict__ slices)
{
    __shared__ int wsum[kHullT / 64];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int r = min(max(num_kept[b], 0), max_regions);
    const mdx_region* recs = regions + (size_t)b * max_regions;
    int2* sl = slices + (size_t)b * max_regions;
    long long carry = 0;
    for (int base = 0; base < r; base += kHullT) {
        const int j = base + tid;
        const int bound = j < r ? region_box(recs[j], w, h).bound : 0;
        int total;
        const int pos = block_scan_exclusive<kHullT>(bound, wsum, total);   // <= 1024 * 2 * 8192
        if (j < r) {
            const int off = (int)min(carry + pos, (long long)cap);
            sl[j] = make_int2(off, min(bound, cap - off));
        }
        carry += total;
    }
}

// Launch 2, grid (records, images): the hull of record j's members -- the pixels of its rectangle whose
// label is its id -- into its slice.  Stage 1 scans the rectangle instead of streaming members: the 1,024
// lanes fold as (columns x row strips) by the rectangle's width.  A group of cw = min(64, 2^ceil(log2
// ncols)) adjacent lanes reads cw adjacent labels of a row (a wave of a wide rectangle: 64 labels, one
// 256-byte request); the 1024 / cw groups lie side by side over the column chunks, and the groups left
// over once every chunk has one take interleaved rows.  A lane walks its rows top to bottom with the
// first and the last matching row in registers and ends with one ds_min_i32 / ds_max_i32 pair per column.
__global__ __launch_bounds__(kHullT) void k_region_hull(const int32_t* __restrict__ labels, int w, int h,
                                                        const mdx_region* __restrict__ regions, int max_regions,
                                                        const int32_t* __restrict__ num_kept,
                                                        const int2* __restrict__ slices, int ncols_lds, int cap, int j0,
                                                        int32_t* __restrict__ counts, int2* __restrict__ staging)
{
    extern __shared__ int32_t hull_lds[];
    __shared__ int wsum[kHullT / 64];
    __shared__ int tail_len[2];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int r = min(max(num_kept[b], 0), max_regions);
    const int j = j0 + (int)blockIdx.x;
    if (j >= r) return;
    const HullLds L = hull_lds_layout(hull_lds, ncols_lds);
    const size_t rec = (size_t)b * max_regions + j;
    const mdx_region R = regions[rec];
    const RegionBox B = region_box(R, w, h);
    const int ncols = min(B.x1 - B.x0, ncols_lds);    // <= w <= ncols_lds
    for (int c = tid; c < ncols; c += kHullT) {
        L.ymin[c] = INT32_MAX;
        L.ymax[c] = INT32_MIN;
    }
    __syncthreads();
    if (ncols > 0) {
        const int cw = ncols > 32 ? 64 : ncols < 2 ? 1 : 1 << (32 - __clz(ncols - 1));
        const int groups = kHullT / cw, chunks = (ncols + cw - 1) / cw;
        const int per = min(chunks, groups);          // groups side by side along x
        const int strips = groups / per;              // row strips; a remainder of groups idles
        const int g = tid / cw, strip = g / per;
        if (strip < strips) {
            const int32_t* lab = labels + (size_t)b * w * h + B.x0;
            for (int c = (g % per) * cw + (tid & (cw - 1)); c < ncols; c += per * cw) {
                int first = INT32_MAX, last = INT32_MIN;
                for (int y = B.y0 + strip; y < B.y1; y += kRegionRows * strips) {
                    int32_t v[kRegionRows];
#pragma unroll
                    for (int u = 0; u < kRegionRows; u++)    // rows past the rectangle re-read its last one
                        v[u] = lab[(size_t)min(y + u * strips, B.y1 - 1) * w + c];
#pragma unroll
                    for (int u = 0; u < kRegionRows; u++) {
                        const int yy = y + u * strips;
                        if (yy < B.y1 && v[u] == R.id) {
                            first = min(first, yy);
                            last = yy;
                        }
                    }
                }
                if (last != INT32_MIN) {
                    atomicMin(&L.ymin[c], first);
                    atomicMax(&L.ymax[c], last);
                }
            }
        }
    }
    __syncthreads();
    const int2 sl = slices[rec];
    const int nv = hull_chains(L, ncols, B.x0, wsum, tail_len, staging + (size_t)b * cap + sl.x, sl.y);
    if (tid == 0) counts[rec] = min(nv, sl.y);
}

// Launch 3, one workgroup per image: the vertex counts scanned into `offsets` (complete: entries past
// the taking-part records repeat the total), each hull copied from its slice to its place in xy as far
// as max_vertices reaches, the total into num_vertices.
__global__ __launch_bounds__(kHullT) void k_region_hull_pack(const int32_t* __restrict__ num_kept, int max_regions,
                                                             const int2* __restrict__ slices,
                                                             const int32_t* __restrict__ counts,
                                                             const int2* __restrict__ staging, int cap,
                                                             int32_t* __restrict__ offsets, int2* __restrict__ xy,
                                                             int max_vertices, int32_t* __restrict__ num_vertices)
{
    __shared__ int wsum[kHullT / 64];
    __shared__ int s_src[kHullT], s_dst[kHullT], s_n[kHullT];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int r = num_kept ? min(max(num_kept[b], 0), max_regions) : 0;
    const int2* sl = slices + (size_t)b * max_regions;
    const int32_t* cnt = counts + (size_t)b * max_regions;
    const int2* src = staging + (size_t)b * cap;
    int32_t* off = offsets + (size_t)b * ((size_t)max_regions + 1);
    int2* dst = xy + (size_t)b * max_vertices;
    int carry = 0;                                      // <= cap <= 2^30
    for (int base = 0; base < r; base += kHullT) {
        const int j = base + tid;
        const int nv = j < r ? cnt[j] : 0;
        int total;
        const int pos = carry + block_scan_exclusive<kHullT>(nv, wsum, total);
        if (j < r) off[j] = pos;
        s_src[tid] = j < r ? sl[j].x : 0;
        s_dst[tid] = pos;
        s_n[tid] = nv;
        __syncthreads();
        const int here = min(kHullT, r - base);
        for (int q = tid >> 6; q < here; q += kHullT / 64) {   // a wave per hull
            const int n = min(s_n[q], max_vertices - s_dst[q]);
            for (int i = tid & 63; i < n; i += 64) dst[s_dst[q] + i] = src[s_src[q] + i];
        }
        __syncthreads();
        carry += total;
    }
    for (int j = r + tid; j <= max_regions; j += kHullT) off[j] = carry;
    if (tid == 0 && num_vertices) num_vertices[b] = carry;
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

// an image's staging block, in vertices: the sum of the honest records' bounds never passes it
static int region_hull_cap(int w, int h, int max_regions)
{
    return (int)std::min<long long>((long long)w * h, 2ll * std::min(w, h) * max_regions);
}

size_t region_hulls_scratch_bytes(int batch, int w, int h, int max_regions, RegionHullScratch* lay)
{
    const size_t B = (size_t)batch, M = (size_t)max_regions;
    RegionHullScratch L;
    L.slices = 0;
    L.counts = B * M * 8;
    L.staging = (B * M * 12 + 255) / 256 * 256;
    if (lay) *lay = L;
    return L.staging + B * (size_t)region_hull_cap(w, h, max_regions) * 8;
}

hipError_t launch_region_hulls(hipStream_t s, int batch, const int32_t* labels, int w, int h, const mdx_region* regions,
                               int max_regions, const int32_t* num_kept, int32_t* offsets, int32_t* xy,
                               int max_vertices, int32_t* num_vertices, void* scratch, hipEvent_t hull_begin,
                               hipEvent_t hull_end)
{
    RegionHullScratch lay;
    region_hulls_scratch_bytes(batch, w, h, max_regions, &lay);
    char* base = static_cast<char*>(scratch);
    int2* slices = reinterpret_cast<int2*>(base + lay.slices);
    int32_t* counts = reinterpret_cast<int32_t*>(base + lay.counts);
    int2* staging = reinterpret_cast<int2*>(base + lay.staging);
    const int cap = region_hull_cap(w, h, max_regions);
    if (max_regions > 0) {                            // else no record takes part: the offsets alone
        hipLaunchKernelGGL(k_region_hull_slices, dim3((unsigned)batch), dim3(kHullT), 0, s, regions, max_regions,
                           num_kept, w, h, cap, slices);
        if (hipError_t e = hipGetLastError()) return e;
        const int ncols_lds = (w + 63) / 64 * 64;
        const size_t lds = hull_lds_bytes(w);
        if (lds > 32 * 1024)
            if (hipError_t e = hipFuncSetAttribute((const void*)k_region_hull, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
                return e;
        if (hull_begin) (void)hipEventRecord(hull_begin, s);
        for (int j0 = 0; j0 < max_regions; j0 += kRegionHullGridX) {   // one launch up to kRegionHullGridX records
            hipLaunchKernelGGL(k_region_hull, dim3((unsigned)std::min(max_regions - j0, kRegionHullGridX), (unsigned)batch),
                               dim3(kHullT), lds, s, labels, w, h, regions, max_regions, num_kept, slices, ncols_lds, cap,
                               j0, counts, staging);
            if (hipError_t e = hipGetLastError()) return e;
        }
        if (hull_end) (void)hipEventRecord(hull_end, s);
    }
    hipLaunchKernelGGL(k_region_hull_pack, dim3((unsigned)batch), dim3(kHullT), 0, s, max_regions > 0 ? num_kept : nullptr,
                       max_regions, slices, counts, staging, cap, offsets, reinterpret_cast<int2*>(xy), max_vertices,
                       num_vertices);
    return hipGetLastError();
}

}  // namespace mdx
