// mdx_regions.hip -- the motion mask labelled into regions: the reference's
// BackgroundSubtractor::getMotionContours recipe (common/src/background_subtractor.cpp:31-35: erode,
// dilate with the default 3x3 element, then findContours' 8-connected foreground blobs) and
// boundingRect per blob (optical_flow_visualizer.cpp:230-236).  Restated from the source; unpinned
// against a real build (no OpenCV 2.4 here).
//
// A label is a pixel's raster index y*w + x; the label image L holds, per foreground pixel, the index
// of a parent in the same component that is never above its own (L[i] <= i), -1 for background.  A
// parent chain therefore strictly decreases and ends at a root (L[r] == r); the root of a finished
// component is its first pixel in raster order.  A call is seven launches on one stream, ordered by
// the launch boundaries alone: no workgroup ever waits for another, and every loop ends on its own
// progress (a chain walk descends; a union retries only when the word it aimed at was lowered
// meanwhile, which the index bounds).
//   k_regions_tile     one workgroup per 64 x 32 tile: foreground rows as bit words (__ballot), the
//                      3x3 opening by shifts, union-find inside the tile in LDS, then L (the tile's
//                      own root per pixel) and mask_out
//   k_regions_merge    one thread per pixel on a tile's top row or left column: union with the up to
//                      three neighbours across the border (diagonals and the tile-corner diagonals
//                      included), atomic min at agent scope on L
//   k_regions_flatten  every foreground pixel walks to its root and stores it; roots are counted per
//                      block of 256 raster indices
//   k_regions_scan     per image, an exclusive scan of those counts; its total is num_all
//   k_regions_rank     a root's rank in raster order is its component id; the root initialises its
//                      record with itself and leaves -2 - id in L
//   k_regions_stats    every other foreground pixel adds itself to its component's record: lanes
//                      that sit side by side in one component are reduced inside the wave first, then
//                      a workgroup's runs per component in an LDS table, so a record receives one
//                      set of atomics per (workgroup of 4,096 pixels, component); labels are written
//   k_regions_out      per image, the min_area filter and the kept order; records and counts
// Reads of L inside a launch that also lowers it (merge, flatten) are agent-scope atomic loads or
// the value an atomic min returned; a stale value is an older parent, still an ancestor.  Integer
// atomics only: every output is bit-reproducible.
// The second half of the file labels the background of the label image the same way and answers which
// blob lies inside which (the k_tree_* kernels).
#include "mdx_internal.h"

namespace mdx {

namespace {

constexpr int kRgTW = 64, kRgTH = 32;        // tile: one ballot word wide
constexpr int kRgRows = kRgTH + 4;           // + 2 halo rows either side (erode, then dilate)
typedef unsigned long long u64;
typedef unsigned __int128 u128;

// bits [lo, hi) of a 128-bit word, 0 <= lo, hi <= 128
__device__ __forceinline__ u128 bits128(int lo, int hi)
{
    if (hi <= lo) return 0;
    const u128 top = hi >= 128 ? ~(u128)0 : (((u128)1 << hi) - 1);
    return top & ~(((u128)1 << lo) - 1);
}

// The in-image columns of tile row y as a bit row: bit k is column x0 - 2 + k, k < 68.
__device__ __forceinline__ u128 valid_bits(int y, int h, int x0, int w)
{
    if (y < 0 || y >= h) return 0;
    return bits128(max(2 - x0, 0), min(w - x0 + 2, kRgTW + 4));
}

__device__ __forceinline__ int lds_load(const int* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ int lds_find(const int* L, int a)
{
    for (int p; (p = lds_load(L + a)) != a;) a = p;   // p < a
    return a;
}

__device__ __forceinline__ void lds_union(int* L, int a, int b)
{
    for (;;) {
        a = lds_find(L, a);
        b = lds_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) return;   // a was a root and now hangs below b
        a = old;                // lowered meanwhile (old < a): go on from there
    }
}

__device__ __forceinline__ int32_t g_load(const int32_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int32_t g_find(const int32_t* L, int32_t a)
{
    for (int32_t p; (p = g_load(L + a)) != a;) a = p;   // p < a, also when stale
    return a;
}

__device__ __forceinline__ void g_union(int32_t* L, int32_t a, int32_t b)
{
    for (;;) {
        a = g_find(L, a);
        b = g_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int32_t t = a;
            a = b, b = t;
        }
        const int32_t old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;
    }
}

struct RegionStat {   // one per component id
    int32_t seed, xmin, xmax, ymax, area;
};

}  // namespace

// grid (tiles_x * tiles_y, batch), 256 threads
__global__ __launch_bounds__(256) void k_regions_tile(const uint8_t* __restrict__ mask, int w, int h, int stride,
                                                       size_t frame_stride, int open3, int tiles_x,
                                                       int32_t* __restrict__ lab, uint8_t* __restrict__ mask_out)
{
    __shared__ u64 sF[kRgRows];                 // foreground, the tile's 64 columns
    __shared__ u64 sH[kRgRows][2];              // horizontal erosion, 68 columns
    __shared__ u64 sE[kRgRows][2];              // erosion
    __shared__ u64 sD[kRgTH + 1];               // D; [0] is the row above the tile: empty
    __shared__ int sL[kRgTH * kRgTW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * kRgTW, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * kRgTH;
    const size_t img = blockIdx.y;
    const uint8_t* m = mask + img * frame_stride;
    const size_t N = (size_t)w * h;

    // rows y0 - 2 .. y0 + kRgTH + 1, columns x0 - 2 .. x0 + 65, as bits
    for (int rr = wave; rr < kRgRows; rr += 4) {
        const int y = y0 - 2 + rr;
        const bool rowin = y >= 0 && y < h;
        const int xa = x0 - 2 + lane, xb = x0 + 62 + lane;
        const bool fa = rowin && xa >= 0 && xa < w && m[(size_t)y * stride + xa] != 0;
        const bool fb = rowin && lane < 4 && xb < w && m[(size_t)y * stride + xb] != 0;
        const u64 ba = __ballot(fa), bb = __ballot(fb);
        if (lane == 0) {
            const u128 F = (u128)ba | ((u128)bb << 64);
            const u128 Fe = F | ~valid_bits(y, h, x0, w);   // out-of-image neighbours never erode
            const u128 Hh = Fe & (Fe << 1) & (Fe >> 1);     // exact for bits 1 .. 66
            sF[rr] = (u64)(F >> 2);
            sH[rr][0] = (u64)Hh;
            sH[rr][1] = (u64)(Hh >> 64);
        }
    }
    __syncthreads();
    if (open3) {
        if (tid >= 1 && tid < kRgRows - 1) {     // E on rows y0 - 1 .. y0 + kRgTH, bits 1 .. 66
            u128 E = ~(u128)0;
            for (int d = -1; d <= 1; d++) E &= (u128)sH[tid + d][0] | ((u128)sH[tid + d][1] << 64);
            E &= valid_bits(y0 - 2 + tid, h, x0, w) & bits128(1, kRgTW + 3);   // out-of-image never dilates
            sE[tid][0] = (u64)E;
            sE[tid][1] = (u64)(E >> 64);
        }
        __syncthreads();
    }
    if (tid < kRgTH) {
        const int rr = tid + 2;
        u64 D;
        if (open3) {
            u128 Dh = 0;
            for (int d = -1; d <= 1; d++) {
                const u128 E = (u128)sE[rr + d][0] | ((u128)sE[rr + d][1] << 64);
                Dh |= E | (E << 1) | (E >> 1);
            }
            D = (u64)((Dh & valid_bits(y0 + tid, h, x0, w)) >> 2);
        } else {
            D = sF[rr];
        }
        sD[tid + 1] = D;
        if (tid == 0) sD[0] = 0;
    }
    __syncthreads();

    // every pixel starts at the first pixel of its row run; thread: column `lane`, rows wave + 4j
    for (int j = 0; j < kRgTH / 4; j++) {
        const int r = wave + 4 * j, p = r * kRgTW + lane;
        const u64 W = sD[r + 1];
        int l = -1;
        if ((W >> lane) & 1) {
            const u64 z = ~W & ((1ull << lane) - 1);
            l = r * kRgTW + (z ? 64 - __clzll((long long)z) : 0);
        }
        sL[p] = l;
        const int x = x0 + lane, y = y0 + r;
        if (mask_out && x < w && y < h) mask_out[img * N + (size_t)y * w + x] = l >= 0 ? 255 : 0;
    }
    __syncthreads();
    // join the runs of adjacent rows: one union per stretch of contact, not one per pixel (the pixel
    // to the left makes the same union when it touches the same run above)
    for (int j = 0; j < kRgTH / 4; j++) {
        const int r = wave + 4 * j, p = r * kRgTW + lane;
        const u64 W = sD[r + 1], U = sD[r];
        if (!((W >> lane) & 1)) continue;
        const bool u0 = (U >> lane) & 1;
        const bool ul = lane > 0 && ((U >> (lane - 1)) & 1), ur = lane < 63 && ((U >> (lane + 1)) & 1);
        const bool wl = lane > 0 && ((W >> (lane - 1)) & 1), wr = lane < 63 && ((W >> (lane + 1)) & 1);
        if (u0) {
            if (!(wl && ul)) lds_union(sL, p, p - kRgTW);
        } else {
            if (ul && !wl) lds_union(sL, p, p - kRgTW - 1);
            if (ur && !wr) lds_union(sL, p, p - kRgTW + 1);
        }
    }
    __syncthreads();
    for (int j = 0; j < kRgTH / 4; j++) {
        const int r = wave + 4 * j, p = r * kRgTW + lane;
        const int x = x0 + lane, y = y0 + r;
        if (x >= w || y >= h) continue;
        int l = sL[p];
        if (l >= 0) {
            l = lds_find(sL, l);
            l = (y0 + (l >> 6)) * w + x0 + (l & 63);   // the tile's first pixel of the component, as a raster index
        }
        lab[img * N + (size_t)y * w + x] = l;
    }
}

// grid (ceil(((tiles_y - 1) * w + (tiles_x - 1) * h) / 256), batch)
__global__ __launch_bounds__(256) void k_regions_merge(int32_t* __restrict__ lab, int w, int h, int tiles_x,
                                                        int tiles_y)
{
    int32_t* L = lab + (size_t)blockIdx.y * ((size_t)w * h);
    int t = (int)(blockIdx.x * 256u + threadIdx.x);
    const int nrow = (tiles_y - 1) * w, ncol = (tiles_x - 1) * h;
    int x, y, dx, dy;   // the neighbour across the border, and the direction along it
    if (t < nrow) {
        y = (t / w + 1) * kRgTH, x = t % w;
        dx = 1, dy = 0;
    } else if ((t -= nrow) < ncol) {
        x = (t / h + 1) * kRgTW, y = t % h;
        dx = 0, dy = 1;
    } else {
        return;
    }
    const int32_t i = y * w + x;
    if (g_load(L + i) < 0) return;
    const int nx = x - dy, ny = y - dx;     // straight across: above (top row) or left (left column)
    const int32_t j = ny * w + nx;
    if (g_load(L + j) >= 0) {
        g_union(L, i, j);     // its neighbours along the border are joined to it by their own tile or border
        return;
    }
    const int ax = nx - dx, ay = ny - dy, bx = nx + dx, by = ny + dy;
    if (ax >= 0 && ay >= 0 && g_load(L + ay * w + ax) >= 0) g_union(L, i, ay * w + ax);
    if (bx < w && by < h && g_load(L + by * w + bx) >= 0) g_union(L, i, by * w + bx);
}

// grid (ceil(N / 256), batch)
__global__ __launch_bounds__(256) void k_regions_flatten(int32_t* __restrict__ lab, int N, int nblk,
                                                          int32_t* __restrict__ blkcnt)
{
    __shared__ int wc[4];
    int32_t* L = lab + (size_t)blockIdx.y * (size_t)N;
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    bool root = false;
    if (i < N) {
        const int32_t l = g_load(L + i);
        if (l >= 0) {
            const int32_t r = g_find(L, l);
            root = r == i;
            if (r != l) __hip_atomic_store(L + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    const u64 b = __ballot(root);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) blkcnt[(size_t)blockIdx.y * nblk + blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// grid (batch): blkcnt -> its exclusive scan, in place; the total is the number of components
__global__ __launch_bounds__(256) void k_regions_scan(int32_t* __restrict__ blkcnt, int nblk,
                                                       int32_t* __restrict__ nall, int32_t* __restrict__ num_all)
{
    __shared__ int part[256];
    int32_t* c = blkcnt + (size_t)blockIdx.x * nblk;
    const int per = (nblk + 255) / 256;
    const int lo = min((int)threadIdx.x * per, nblk), hi = min(lo + per, nblk);
    int s = 0;
    for (int k = lo; k < hi; k++) s += c[k];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int k = 0; k < 256; k++) {
            const int v = part[k];
            part[k] = run;
            run += v;
        }
        nall[blockIdx.x] = run;
        if (num_all) num_all[blockIdx.x] = run;
    }
    __syncthreads();
    int run = part[threadIdx.x];
    for (int k = lo; k < hi; k++) {
        const int v = c[k];
        c[k] = run;
        run += v;
    }
}

// grid (ceil(N / 256), batch)
__global__ __launch_bounds__(256) void k_regions_rank(int32_t* __restrict__ lab, int w, int N, int nblk,
                                                       const int32_t* __restrict__ blkoff,
                                                       RegionStat* __restrict__ stats, int maxcomp)
{
    __shared__ int wc[4];
    int32_t* L = lab + (size_t)blockIdx.y * (size_t)N;
    const int i = (int)(blockIdx.x * 256u + threadIdx.x), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool root = i < N && L[i] == i;
    const u64 b = __ballot(root);
    if (lane == 0) wc[wave] = __popcll(b);
    __syncthreads();
    if (!root) return;
    int id = blkoff[(size_t)blockIdx.y * nblk + blockIdx.x] + __popcll(b & ((1ull << lane) - 1));
    for (int q = 0; q < wave; q++) id += wc[q];
    if (id >= maxcomp) return;   // cannot happen: two roots are never 8-neighbours
    const int x = i % w, y = i / w;
    stats[(size_t)blockIdx.y * maxcomp + id] = RegionStat{i, x, x, y, 1};
    L[i] = -2 - id;
}

// One set of atomics on a component's record.
__device__ __forceinline__ void stat_add(RegionStat* s, int cnt, int xmin, int xmax, int ymax)
{
    atomicAdd(&s->area, cnt);
    atomicMin(&s->xmin, xmin);
    atomicMax(&s->xmax, xmax);
    atomicMax(&s->ymax, ymax);   // ymin is the seed's row
}

constexpr int kRgStatIters = 16;    // k_regions_stats: a workgroup takes 16 x 256 consecutive raster indices
constexpr int kRgStatSlots = 128;   // and sums what they add per component in an LDS table of this many slots

// grid (ceil(N / (256 * kRgStatIters)), batch).  Two reductions in front of the global atomics: lanes
// side by side with one id inside the wave, then the workgroup's runs per id in LDS (a hash table
// keyed by id; a run that finds its four probe slots taken by other ids goes to memory directly).
// A component that covers the frame receives four atomics per 4,096 pixels.
__global__ __launch_bounds__(256) void k_regions_stats(const int32_t* __restrict__ lab, int w, int N,
                                                        RegionStat* __restrict__ stats, int maxcomp,
                                                        int32_t* __restrict__ labels)
{
    __shared__ int hkey[kRgStatSlots], hcnt[kRgStatSlots], hxmin[kRgStatSlots], hxmax[kRgStatSlots],
        hymax[kRgStatSlots];
    const int32_t* L = lab + (size_t)blockIdx.y * (size_t)N;
    RegionStat* st = stats + (size_t)blockIdx.y * maxcomp;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < kRgStatSlots) {
        hkey[threadIdx.x] = -1, hcnt[threadIdx.x] = 0;
        hxmin[threadIdx.x] = 0x7fffffff, hxmax[threadIdx.x] = -1, hymax[threadIdx.x] = -1;
    }
    __syncthreads();
    for (int it = 0; it < kRgStatIters; it++) {
        const long long i64 = ((long long)blockIdx.x * kRgStatIters + it) * 256 + threadIdx.x;
        const int i = (int)min(i64, (long long)N);    // N <= 2^30
        int id = -1, cnt = 0;
        if (i < N) {
            const int32_t l = L[i];
            if (l >= 0) {
                id = -2 - L[l];     // flattened: l is the root, which holds -2 - id
                cnt = 1;
            } else if (l <= -2) {
                id = -2 - l;        // a root: its record already counts it
            }
            if (labels) labels[(size_t)blockIdx.y * (size_t)N + i] = id;
        }
        // a run: lanes side by side with one id.  Its first lane ends up with the run's sums.
        const int prev = __shfl_up(id, 1);
        const u64 heads = __ballot(lane == 0 || prev != id);
        const u64 later = lane == 63 ? 0 : heads >> (lane + 1);
        const int end = later ? lane + 1 + __builtin_ctzll(later) : 64;
        const int x = i % w, y = i / w;
        int xmin = cnt ? x : 0x7fffffff, xmax = cnt ? x : -1, ymax = cnt ? y : -1;
        for (int d = 1; d < 64; d <<= 1) {
            const int c2 = __shfl_down(cnt, d), n2 = __shfl_down(xmin, d), x2 = __shfl_down(xmax, d),
                      y2 = __shfl_down(ymax, d);
            if (lane + d < end) {
                cnt += c2;
                xmin = min(xmin, n2), xmax = max(xmax, x2), ymax = max(ymax, y2);
            }
        }
        if (!((heads >> lane) & 1) || id < 0 || id >= maxcomp || cnt == 0) continue;
        int slot = (int)(((uint32_t)id * 2654435761u) >> 16) & (kRgStatSlots - 1);
        bool placed = false;
        for (int probe = 0; probe < 4 && !placed; probe++, slot = (slot + 1) & (kRgStatSlots - 1)) {
            const int old = atomicCAS(&hkey[slot], -1, id);
            if (old != -1 && old != id) continue;
            atomicAdd(&hcnt[slot], cnt);
            atomicMin(&hxmin[slot], xmin);
            atomicMax(&hxmax[slot], xmax);
            atomicMax(&hymax[slot], ymax);
            placed = true;
        }
        if (!placed) stat_add(st + id, cnt, xmin, xmax, ymax);
    }
    __syncthreads();
    if (threadIdx.x < kRgStatSlots && hkey[threadIdx.x] >= 0)
        stat_add(st + hkey[threadIdx.x], hcnt[threadIdx.x], hxmin[threadIdx.x], hxmax[threadIdx.x], hymax[threadIdx.x]);
}

// grid (batch)
__global__ __launch_bounds__(256) void k_regions_out(const RegionStat* __restrict__ stats, int maxcomp,
                                                      const int32_t* __restrict__ nall, int w, int min_area,
                                                      mdx_region* __restrict__ regions, int max_regions,
                                                      int32_t* __restrict__ num_kept)
{
    __shared__ int wc[4];
    const RegionStat* st = stats + (size_t)blockIdx.x * maxcomp;
    const int n = min(nall[blockIdx.x], maxcomp), lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int id = c0 + (int)threadIdx.x;
        RegionStat s{};
        if (id < n) s = st[id];
        const bool keep = id < n && s.area >= min_area;
        const u64 b = __ballot(keep);
        __syncthreads();     // the previous round's wc has been read
        if (lane == 0) wc[wave] = __popcll(b);
        __syncthreads();
        int pos = base + __popcll(b & ((1ull << lane) - 1));
        for (int q = 0; q < wave; q++) pos += wc[q];
        if (keep && pos < max_regions) {
            const int sx = s.seed % w, sy = s.seed / w;
            regions[(size_t)blockIdx.x * max_regions + pos] =
                mdx_region{s.xmin, sy, s.xmax - s.xmin + 1, s.ymax - sy + 1, s.area, sx, sy, id};
        }
        base += wc[0] + wc[1] + wc[2] + wc[3];
    }
    if (threadIdx.x == 0 && num_kept) num_kept[blockIdx.x] = base;
}

size_t regions_scratch_bytes(int batch, int w, int h, RegionsScratch* lay)
{
    const size_t N = (size_t)w * h, nblk = (N + 255) / 256, maxc = (size_t)((w + 1) / 2) * ((h + 1) / 2);
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    RegionsScratch s{};
    s.lab = 0;
    s.blk = up(N * 4 * batch);
    s.stats = s.blk + up(nblk * 4 * batch);
    s.nall = s.stats + up(maxc * sizeof(RegionStat) * batch);
    if (lay) *lay = s;
    return s.nall + up((size_t)4 * batch);
}

hipError_t launch_mask_regions(hipStream_t s, int batch, const uint8_t* mask, int w, int h, int stride,
                               size_t frame_stride, int open3, int min_area, mdx_region* regions, int max_regions,
                               int32_t* num_all, int32_t* num_kept, int32_t* labels, uint8_t* mask_out, void* scratch)
{
    if (batch < 1 || batch > kRegionsMaxBatch || w < 1 || h < 1 || (long long)w * h > (1ll << 30))
        return hipErrorInvalidValue;
    RegionsScratch lay;
    (void)regions_scratch_bytes(batch, w, h, &lay);
    char* base = static_cast<char*>(scratch);
    int32_t* lab = reinterpret_cast<int32_t*>(base + lay.lab);
    int32_t* blk = reinterpret_cast<int32_t*>(base + lay.blk);
    RegionStat* stats = reinterpret_cast<RegionStat*>(base + lay.stats);
    int32_t* nall = reinterpret_cast<int32_t*>(base + lay.nall);
    const int N = w * h, nblk = (N + 255) / 256, maxc = ((w + 1) / 2) * ((h + 1) / 2);
    const int tx = (w + kRgTW - 1) / kRgTW, ty = (h + kRgTH - 1) / kRgTH;
    const int nborder = (ty - 1) * w + (tx - 1) * h;
    hipLaunchKernelGGL(k_regions_tile, dim3(tx * ty, batch), dim3(256), 0, s, mask, w, h, stride, frame_stride, open3,
                       tx, lab, mask_out);
    if (nborder > 0)
        hipLaunchKernelGGL(k_regions_merge, dim3((nborder + 255) / 256, batch), dim3(256), 0, s, lab, w, h, tx, ty);
    hipLaunchKernelGGL(k_regions_flatten, dim3(nblk, batch), dim3(256), 0, s, lab, N, nblk, blk);
    hipLaunchKernelGGL(k_regions_scan, dim3(batch), dim3(256), 0, s, blk, nblk, nall, num_all);
    hipLaunchKernelGGL(k_regions_rank, dim3(nblk, batch), dim3(256), 0, s, lab, w, N, nblk, blk, stats, maxc);
    hipLaunchKernelGGL(k_regions_stats, dim3((nblk + kRgStatIters - 1) / kRgStatIters, batch), dim3(256), 0, s, lab, w, N,
                       stats, maxc, labels);
    hipLaunchKernelGGL(k_regions_out, dim3(batch), dim3(256), 0, s, stats, maxc, nall, w, min_area, regions,
                       max_regions, num_kept);
    return hipGetLastError();
}

// ---- which blob lies inside which: the background of the label image, labelled with
// 4-connectivity by the same scheme -- a parent image B with B[i] <= i for a background pixel
// (labels[i] < 0) and -1 for a foreground one -- so that the root of a finished background component
// is its first pixel in raster order.  The component that holds a background pixel of the frame's
// first or last row or column is the frame background; every other one is a hole, and the pixel
// above a hole's first pixel belongs to the blob whose hole it is.  A call is five launches on one
// stream, ordered by the launch boundaries alone, with the same loop discipline as above.
//   k_tree_tile      one workgroup per 64 x 32 tile: background rows as bit words, the runs of adjacent
//                    rows joined where a bit sits directly above a bit, union-find in LDS; B (the
//                    tile's own root per pixel) and the mark byte (2: a tile root, else 0)
//   k_tree_merge     one thread per pixel on a tile's top row or left column: union straight across
//                    the border, once per stretch of contact inside one tile edge
//   k_tree_roots     every tile root walks to its root and stores it.  On a frame-wide background the
//                    chains run tile root to tile root across the frame; only the tile roots walk them
//   k_tree_flatten   every other background pixel takes its tile root's root: two loads.  A background
//                    pixel on the frame edge sets bit 0 of its root's mark (every writer stores 3)
//   k_tree_resolve   per image, one thread per participating record: its parent, and the external
//                    records compacted in record order by ballot prefix

// grid (tiles_x * tiles_y, batch), 256 threads
__global__ __launch_bounds__(256) void k_tree_tile(const int32_t* __restrict__ labels, int w, int h, int tiles_x,
                                                    int32_t* __restrict__ bg, uint8_t* __restrict__ mark)
{
    __shared__ u64 sB[kRgTH + 1];               // background; [0] is the row above the tile: empty
    __shared__ int sL[kRgTH * kRgTW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * kRgTW, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * kRgTH;
    const size_t base = (size_t)blockIdx.y * ((size_t)w * h);
    const int x = x0 + lane;
    for (int j = 0; j < kRgTH / 4; j++) {
        const int r = wave + 4 * j, y = y0 + r;
        const bool b = x < w && y < h && labels[base + (size_t)y * w + x] < 0;
        const u64 W = __ballot(b);
        if (lane == 0) sB[r + 1] = W;
    }
    if (tid == 0) sB[0] = 0;
    __syncthreads();
    // every pixel starts at the first pixel of its row run
    for (int j = 0; j < kRgTH / 4; j++) {
        const int r = wave + 4 * j;
        const u64 W = sB[r + 1];
        int l = -1;
        if ((W >> lane) & 1) {
            const u64 z = ~W & ((1ull << lane) - 1);
            l = r * kRgTW + (z ? 64 - __clzll((long long)z) : 0);
        }
        sL[r * kRgTW + lane] = l;
    }
    __syncthreads();
    // a bit directly above a bit: one union per stretch of contact (the pixel to the left makes the
    // same union when it and the one above it are background too)
    for (int j = 0; j < kRgTH / 4; j++) {
        const int r = wave + 4 * j, p = r * kRgTW + lane;
        const u64 C = sB[r + 1] & sB[r];
        if (((C >> lane) & 1) && !(lane > 0 && ((C >> (lane - 1)) & 1))) lds_union(sL, p, p - kRgTW);
    }
    __syncthreads();
    for (int j = 0; j < kRgTH / 4; j++) {
        const int r = wave + 4 * j, p = r * kRgTW + lane, y = y0 + r;
        if (x >= w || y >= h) continue;
        int l = sL[p];
        uint8_t m = 0;
        if (l >= 0) {
            l = lds_find(sL, l);
            m = l == p ? 2 : 0;
            l = (y0 + (l >> 6)) * w + x0 + (l & 63);
        }
        bg[base + (size_t)y * w + x] = l;
        mark[base + (size_t)y * w + x] = m;
    }
}

// grid (ceil(((tiles_y - 1) * w + (tiles_x - 1) * h) / 256), batch)
__global__ __launch_bounds__(256) void k_tree_merge(int32_t* __restrict__ bg, int w, int h, int tiles_x, int tiles_y)
{
    int32_t* B = bg + (size_t)blockIdx.y * ((size_t)w * h);
    int t = (int)(blockIdx.x * 256u + threadIdx.x);
    const int nrow = (tiles_y - 1) * w, ncol = (tiles_x - 1) * h;
    int x, y, dx, dy, along;   // the pixel, the direction along the border, its place inside the tile edge
    if (t < nrow) {
        y = (t / w + 1) * kRgTH, x = t % w;
        dx = 1, dy = 0, along = x % kRgTW;
    } else if ((t -= nrow) < ncol) {
        x = (t / h + 1) * kRgTW, y = t % h;
        dx = 0, dy = 1, along = y % kRgTH;
    } else {
        return;
    }
    const int32_t i = y * w + x, j = (y - dx) * w + (x - dy);     // straight across: above, or to the left
    if (g_load(B + i) < 0 || g_load(B + j) < 0) return;
    // the pair before this one along the same tile edge makes the same union: each side's two pixels
    // are neighbours inside one tile
    if (along > 0 && g_load(B + i - dx - dy * w) >= 0 && g_load(B + j - dx - dy * w) >= 0) return;
    g_union(B, i, j);
}

// grid (ceil(N / 256), batch)
__global__ __launch_bounds__(256) void k_tree_roots(int32_t* __restrict__ bg, int N, const uint8_t* __restrict__ mark)
{
    int32_t* B = bg + (size_t)blockIdx.y * (size_t)N;
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= N || !mark[(size_t)blockIdx.y * (size_t)N + i]) return;
    const int32_t l = g_load(B + i), r = g_find(B, l);
    if (r != l) __hip_atomic_store(B + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (ceil(N / 256), batch).  Only the words of pixels that are no tile root are written, and only
// the words of tile roots are read a second time: they are final since k_tree_roots.
__global__ __launch_bounds__(256) void k_tree_flatten(int32_t* __restrict__ bg, int w, int h, uint8_t* __restrict__ mark)
{
    const int N = w * h;
    int32_t* B = bg + (size_t)blockIdx.y * (size_t)N;
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= N) return;
    const int32_t l = B[i];
    if (l < 0) return;
    const int32_t r = B[l];
    if (r != l) B[i] = r;
    const int x = i % w, y = i / w;
    if (x == 0 || y == 0 || x == w - 1 || y == h - 1) mark[(size_t)blockIdx.y * (size_t)N + r] = 3;
}

// The parent of one record (include/mdx.h): MDX_REGION_NO_PARENT, MDX_REGION_PARENT_UNKNOWN or an id.
// No access outside the frame results from a record.
__device__ __forceinline__ int32_t tree_parent(const mdx_region& rec, const int32_t* __restrict__ lab,
                                               const int32_t* __restrict__ B, const uint8_t* __restrict__ mark, int w, int h)
{
    const int sx = rec.seed_x, sy = rec.seed_y;
    if (sx < 0 || sx >= w || sy < 0 || sy >= h || rec.id < 0) return MDX_REGION_PARENT_UNKNOWN;
    if (lab[sy * w + sx] != rec.id) return MDX_REGION_PARENT_UNKNOWN;
    if (sy == 0) return MDX_REGION_NO_PARENT;
    const int32_t above = (sy - 1) * w + sx;
    if (lab[above] >= 0) return MDX_REGION_PARENT_UNKNOWN;
    const int32_t root = B[above];                    // the enclosing background's first pixel
    if (root < 0) return MDX_REGION_PARENT_UNKNOWN;   // cannot happen: B is built from these labels
    if (mark[root] & 1) return MDX_REGION_NO_PARENT;
    if (root < w) return MDX_REGION_PARENT_UNKNOWN;   // cannot happen: a hole never touches row 0
    const int32_t p = lab[root - w];
    return p >= 0 ? p : MDX_REGION_PARENT_UNKNOWN;
}

constexpr int kTreeResolveThreads = 1024;

// grid (batch), 1,024 threads
__global__ __launch_bounds__(kTreeResolveThreads) void k_tree_resolve(
    const int32_t* __restrict__ labels, const int32_t* __restrict__ bg, const uint8_t* __restrict__ mark, int w, int h,
    const mdx_region* __restrict__ regions, int max_regions, const int32_t* __restrict__ num_kept,
    int32_t* __restrict__ parent, mdx_region* __restrict__ external, int32_t* __restrict__ num_external)
{
    constexpr int kWaves = kTreeResolveThreads / 64;
    __shared__ int wc[kWaves];
    const size_t N = (size_t)w * h, img = blockIdx.x;
    const int r = max_regions > 0 ? min(max(num_kept[img], 0), max_regions) : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int c0 = 0; c0 < r; c0 += kTreeResolveThreads) {
        const int j = c0 + (int)threadIdx.x;
        mdx_region rec{};
        bool ext = false;
        if (j < r) {
            rec = regions[img * max_regions + j];
            const int32_t p = tree_parent(rec, labels + img * N, bg + img * N, mark + img * N, w, h);
            if (parent) parent[img * max_regions + j] = p;
            ext = p == MDX_REGION_NO_PARENT;
        }
        const u64 b = __ballot(ext);
        __syncthreads();     // the previous round's wc has been read
        if (lane == 0) wc[wave] = __popcll(b);
        __syncthreads();
        int pos = base + __popcll(b & ((1ull << lane) - 1)), total = 0;
        for (int q = 0; q < kWaves; q++) {
            if (q < wave) pos += wc[q];
            total += wc[q];
        }
        if (ext && external) external[img * max_regions + pos] = rec;
        base += total;
    }
    if (threadIdx.x == 0 && num_external) num_external[img] = base;
}

size_t region_parents_scratch_bytes(int batch, int w, int h, RegionTreeScratch* lay)
{
    const size_t N = (size_t)w * h;
    RegionTreeScratch s{};
    s.bg = 0;
    s.mark = (N * 4 * batch + 255) / 256 * 256;
    if (lay) *lay = s;
    return s.mark + (N * batch + 255) / 256 * 256;
}

hipError_t launch_region_parents(hipStream_t s, int batch, const int32_t* labels, int w, int h,
                                 const mdx_region* regions, int max_regions, const int32_t* num_kept, int32_t* parent,
                                 mdx_region* external, int32_t* num_external, void* scratch, hipEvent_t* ev)
{
    if (batch < 1 || batch > kRegionsMaxBatch || w < 1 || h < 1 || (long long)w * h > (1ll << 30))
        return hipErrorInvalidValue;
    RegionTreeScratch lay;
    (void)region_parents_scratch_bytes(batch, w, h, &lay);
    int32_t* bg = reinterpret_cast<int32_t*>(static_cast<char*>(scratch) + lay.bg);
    uint8_t* mark = reinterpret_cast<uint8_t*>(static_cast<char*>(scratch) + lay.mark);
    const int N = w * h, nblk = (N + 255) / 256;
    const int tx = (w + kRgTW - 1) / kRgTW, ty = (h + kRgTH - 1) / kRgTH;
    const int nborder = (ty - 1) * w + (tx - 1) * h;
    auto stamp = [&](int i) { return ev ? hipEventRecord(ev[i], s) : hipSuccess; };   // behind kernel i of the five
    if (max_regions > 0) {    // no record, no question: only num_external is written
        hipLaunchKernelGGL(k_tree_tile, dim3(tx * ty, batch), dim3(256), 0, s, labels, w, h, tx, bg, mark);
        (void)stamp(1);
        if (nborder > 0)
            hipLaunchKernelGGL(k_tree_merge, dim3((nborder + 255) / 256, batch), dim3(256), 0, s, bg, w, h, tx, ty);
        (void)stamp(2);
        hipLaunchKernelGGL(k_tree_roots, dim3(nblk, batch), dim3(256), 0, s, bg, N, mark);
        (void)stamp(3);
        hipLaunchKernelGGL(k_tree_flatten, dim3(nblk, batch), dim3(256), 0, s, bg, w, h, mark);
        (void)stamp(4);
    } else {
        for (int i = 1; i <= 4; i++) (void)stamp(i);
    }
    hipLaunchKernelGGL(k_tree_resolve, dim3(batch), dim3(kTreeResolveThreads), 0, s, labels, bg, mark, w, h, regions,
                       max_regions, num_kept, parent, external, num_external);
    (void)stamp(5);
    return hipGetLastError();
}

}  // namespace mdx
