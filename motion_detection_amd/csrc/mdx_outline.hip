// mdx_outline.hip -- the outer border polyline of each mask region (findContours' RETR_EXTERNAL,
// CHAIN_APPROX_NONE point lists; mdx_region_outlines_dev).
//
// Border following is a walk; here it is a ranking.  A state is (p, b): a member pixel p and a direction b
// in which p has a member neighbour.  The tracing rule (mdx_plan.h outline_next_dir) maps (p, b) to
// (q, t ^ 4) with q = p + D[t]; outline_prev_dir inverts it, so the rule is a bijection on the states and
// every state lies on exactly one cycle.  The outline of a record is the cycle through its start state,
// and a state's place in the outline is its distance from the start along the cycle: list ranking.
//   k_outline_mask    per pixel its 8-bit same-label-neighbour mask -- kept only where the pixel has a
//                     non-member 4-neighbour (the others are on no outer border and carry no state: their
//                     byte is 0) -- and per 256 pixels the number of states.
//   k_outline_blocks  per image the exclusive scan of those numbers; the state total; the round flags cleared.
//   k_outline_base    per pixel the index of its first state: state (p, b) is base[p] + popcount(mask(p) &
//                     ((1 << b) - 1)).
//   k_outline_pred    per state the 64-bit word (predecessor, 1); a state whose predecessor pixel carries no
//                     state is on no outer border and becomes a dead end (itself | kRes, 0).
//   k_outline_starts  per record its start state's word becomes (kNil, j): the chain ends there.
//   k_outline_round   x outline_rounds(w, h): pointer jumping in place (see the kernel).
//   k_outline_offsets per image the outline lengths scanned into `offsets`; the one-pixel outlines written.
//   k_outline_scatter per state that reached a start: xy[offsets[j] + position] = p.
// The launches are ordered by their boundaries alone: no workgroup waits for another.
//
// Records are device memory a caller may have edited.  One that names a pixel outside the frame, a pixel
// of another id or a negative id gives 0 points.  One whose seed is a member but whose cycle the ranking
// did not deliver -- the seed carries no state, two records share a start state or a cycle -- is walked by
// one lane from the label image (outline_walk): slow, exact, and never outside the frame.
#include "mdx_dev.h"

#include <algorithm>

namespace mdx {

namespace {

constexpr int kOlT = 256;                 // threads, and pixels, of a per-pixel workgroup
constexpr int kOlScanT = 1024;            // threads of the per-image workgroups
constexpr int kOlRoundBlocks = 2048;      // workgroups per image of a round (grid-stride over the states)
constexpr int kOlFlags = 64;              // round flags per image (outline_rounds <= 31)
constexpr uint32_t kNil = 0xFFFFFFFFu;    // high word of a start state
constexpr uint32_t kRes = 0x80000000u;    // high word bit: the low 31 bits are the chain's end, the low word the position

using u64 = unsigned long long;

__device__ __forceinline__ u64 pack(uint32_t hi, uint32_t lo) { return (u64)hi << 32 | lo; }
// one 8-byte access each, so a reader sees a pair some thread stored whole
__device__ __forceinline__ u64 word_load(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void word_store(u64* p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// bit d: the neighbour of (x, y) in direction d lies in the frame and carries id
__device__ __forceinline__ unsigned member_mask(const int32_t* __restrict__ lab, int w, int h, int x, int y, int32_t id)
{
    unsigned m = 0;
#pragma unroll
    for (int d = 0; d < 8; d++) {
        const int nx = x + outline_dx(d), ny = y + outline_dy(d);
        if ((unsigned)nx < (unsigned)w && (unsigned)ny < (unsigned)h && lab[(size_t)ny * w + nx] == id) m |= 1u << d;
    }
    return m;
}

__device__ __forceinline__ bool seed_ok(const mdx_region& R, const int32_t* __restrict__ lab, int w, int h)
{
    return R.id >= 0 && (unsigned)R.seed_x < (unsigned)w && (unsigned)R.seed_y < (unsigned)h &&
           lab[(size_t)R.seed_y * w + R.seed_x] == R.id;
}

// The rule walked from (sx, sy, b0) until that state returns; the first `room` points into dst (may be NULL).
__device__ long long outline_walk(const int32_t* __restrict__ lab, int w, int h, int32_t id, int sx, int sy, int b0,
                                  int2* dst, long long room)
{
    int x = sx, y = sy, b = b0;
    long long n = 0;
    do {
        if (dst && n < room) dst[n] = make_int2(x, y);
        n++;
        const int t = outline_next_dir(member_mask(lab, w, h, x, y, id), b);
        x += outline_dx(t);
        y += outline_dy(t);
        b = t ^ 4;
    } while (x != sx || y != sy || b != b0);
    return n;
}

template <int T>
__device__ __forceinline__ long long block_scan_exclusive_ll(long long v, long long* wsum, long long& total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    long long off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < T / 64; i++) {
        const long long s = wsum[i];
        if (i < w) off += s;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return off + inc - v;
}

__global__ __launch_bounds__(kOlT) void k_outline_mask(const int32_t* __restrict__ labels, int w, int h, int nblk,
                                                       uint8_t* __restrict__ nbr, int32_t* __restrict__ blk)
{
    __shared__ int wsum[kOlT / 64];
    const size_t N = (size_t)w * h, b = blockIdx.y;
    const size_t p = (size_t)blockIdx.x * kOlT + threadIdx.x;
    const int32_t* lab = labels + b * N;
    unsigned m = 0;
    if (p < N) {
        const int32_t id = lab[p];
        if (id >= 0) {
            m = member_mask(lab, w, h, (int)(p % w), (int)(p / w), id);
            if ((m & 0x55u) == 0x55u) m = 0;      // E, N, W and S are all members: on no outer border
        }
        nbr[b * N + p] = (uint8_t)m;
    }
    int total;
    block_scan_exclusive<kOlT>(__popc(m), wsum, total);
    if (threadIdx.x == 0) blk[b * nblk + blockIdx.x] = total;
}

__global__ __launch_bounds__(kOlScanT) void k_outline_blocks(int nblk, int32_t* __restrict__ blk,
                                                             int32_t* __restrict__ nstates, int32_t* __restrict__ flags)
{
    __shared__ int wsum[kOlScanT / 64];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    int32_t* v = blk + b * nblk;
    int carry = 0;                                  // <= 7 * w * h < 2^31
    for (int base = 0; base < nblk; base += kOlScanT) {
        const int i = base + tid;
        int total;
        const int pos = block_scan_exclusive<kOlScanT>(i < nblk ? v[i] : 0, wsum, total);
        if (i < nblk) v[i] = carry + pos;
        carry += total;
    }
    if (tid == 0) nstates[b] = carry;
    if (tid < kOlFlags) flags[b * kOlFlags + tid] = 0;
}

__global__ __launch_bounds__(kOlT) void k_outline_base(int w, int h, int nblk, const uint8_t* __restrict__ nbr,
                                                       const int32_t* __restrict__ blk, int32_t* __restrict__ base)
{
    __shared__ int wsum[kOlT / 64];
    const size_t N = (size_t)w * h, b = blockIdx.y;
    const size_t p = (size_t)blockIdx.x * kOlT + threadIdx.x;
    const unsigned m = p < N ? nbr[b * N + p] : 0u;
    int total;
    const int pos = block_scan_exclusive<kOlT>(__popc(m), wsum, total);
    if (p < N) base[b * N + p] = blk[b * nblk + blockIdx.x] + pos;
}

__device__ __forceinline__ uint32_t state_index(const int32_t* __restrict__ base, size_t p, unsigned m, int b)
{
    return (uint32_t)base[p] + __popc(m & ((1u << b) - 1u));
}

__global__ __launch_bounds__(kOlT) void k_outline_pred(int w, int h, const uint8_t* __restrict__ nbr_,
                                                       const int32_t* __restrict__ base_, u64* __restrict__ words)
{
    const size_t N = (size_t)w * h, b = blockIdx.y;
    const size_t p = (size_t)blockIdx.x * kOlT + threadIdx.x;
    if (p >= N) return;
    const uint8_t* nbr = nbr_ + b * N;
    const int32_t* base = base_ + b * N;
    u64* word = words + b * 7 * N;
    const unsigned m = nbr[p];
    if (!m) return;
    const int x = (int)(p % w), y = (int)(p / w);
    uint32_t idx = (uint32_t)base[p];
    for (int d = 0; d < 8; d++) {
        if (!(m >> d & 1u)) continue;
        // the state (p, d) was entered from pp = p + D[d], which left in direction d ^ 4
        const size_t pp = (size_t)(y + outline_dy(d)) * w + (x + outline_dx(d));
        const unsigned mp = nbr[pp];
        if (!mp)
            word_store(word + idx, pack(kRes | idx, 0));
        else
            word_store(word + idx, pack(state_index(base, pp, mp, outline_prev_dir(mp, d ^ 4)), 1));
        idx++;
    }
}

__global__ __launch_bounds__(kOlT) void k_outline_starts(const int32_t* __restrict__ labels, int w, int h,
                                                         const mdx_region* __restrict__ regions, int max_regions,
                                                         const int32_t* __restrict__ num_kept,
                                                         const uint8_t* __restrict__ nbr, const int32_t* __restrict__ base,
                                                         u64* __restrict__ words)
{
    const size_t N = (size_t)w * h, b = blockIdx.y;
    const int r = min(max(num_kept[b], 0), max_regions);
    const int j = blockIdx.x * kOlT + threadIdx.x;
    if (j >= r) return;
    const mdx_region R = regions[b * max_regions + j];
    if (!seed_ok(R, labels + b * N, w, h)) return;
    const size_t p = (size_t)R.seed_y * w + R.seed_x;
    const unsigned m = nbr[b * N + p];
    if (!m) return;
    word_store(words + b * 7 * N + state_index(base + b * N, p, m, outline_prev_dir(m, 4)), pack(kNil, (uint32_t)j));
}

// One round of pointer jumping, in place.  A state's word is (a, d): a is the state d steps back along the
// chain, and none of those steps passes a start.  That is a property of the pair alone, so it holds for
// every word ever stored; a word is written by its own state's lane only and read in one 8-byte access, so a
// jump that reads a's word (aa, ad) -- whether a's lane has already run this round or not -- stores (aa,
// d + ad), which has the property again.  Distances only grow.  After round k every state has d >= min(2^k,
// its position): a's word is at least a's word of the round before, so d + ad >= min(2 * 2^k, position).
// Hence outline_rounds rounds bring every state of a chain to its start.  A state that finds the start
// behind it, or a state that has, takes kRes and rests.  In every round in which a chain still has an
// unmarked state, the first such state along the chain is marked (what it points at lies before it, so
// that is the start or a marked state): a round that marks nothing in an image was not needed, and the
// rounds after it return at once (flags).  Cycles without a start -- hole borders, dead ends' tails --
// keep jumping in place, their distances wrapping: nobody reads them.
__global__ __launch_bounds__(kOlT) void k_outline_round(int k, size_t per_image, const int32_t* __restrict__ nstates,
                                                        int32_t* __restrict__ flags, u64* __restrict__ words)
{
    const size_t b = blockIdx.y;
    if (k > 0 && flags[b * kOlFlags + k - 1] == 0) return;
    const uint32_t S = (uint32_t)nstates[b];
    u64* word = words + b * per_image;
    bool marked = false;
    for (uint32_t i = blockIdx.x * kOlT + threadIdx.x; i < S; i += gridDim.x * kOlT) {
        const u64 me = word_load(word + i);
        const uint32_t a = (uint32_t)(me >> 32), d = (uint32_t)me;
        if (a & kRes) continue;
        const u64 wa = word_load(word + a);
        const uint32_t aa = (uint32_t)(wa >> 32), ad = (uint32_t)wa;
        if (aa == kNil) {
            word_store(word + i, pack(kRes | a, d));
            marked = true;
        } else {
            word_store(word + i, pack(aa, d + ad));
            marked |= (aa & kRes) != 0;
        }
    }
    if (marked) flags[b * kOlFlags + k] = 1;
}

// the record whose start state's word is ws, and the position, of a state whose word is me; false: none
__device__ __forceinline__ bool state_place(const u64* __restrict__ word, u64 me, uint32_t& j, uint32_t& pos)
{
    const uint32_t a = (uint32_t)(me >> 32);
    if (a == kNil) {
        j = (uint32_t)me;
        pos = 0;
        return true;
    }
    const u64 wa = word_load(word + (a & ~kRes));
    if ((uint32_t)(wa >> 32) != kNil) return false;
    j = (uint32_t)wa;
    pos = (uint32_t)me;
    return true;
}

__global__ __launch_bounds__(kOlScanT) void k_outline_offsets(const int32_t* __restrict__ labels, int w, int h,
                                                              const mdx_region* __restrict__ regions, int max_regions,
                                                              const int32_t* __restrict__ num_kept,
                                                              const uint8_t* __restrict__ nbr_,
                                                              const int32_t* __restrict__ base_,
                                                              const u64* __restrict__ words,
                                                              int32_t* __restrict__ offsets, int2* __restrict__ xy,
                                                              int max_points, int32_t* __restrict__ num_points)
{
    __shared__ long long wsum[kOlScanT / 64];
    const int tid = threadIdx.x;
    const size_t N = (size_t)w * h, b = blockIdx.x;
    const int r = num_kept ? min(max(num_kept[b], 0), max_regions) : 0;
    const int32_t* lab = labels + b * N;
    const uint8_t* nbr = nbr_ + b * N;
    const int32_t* base = base_ + b * N;
    const u64* word = words + b * 7 * N;
    int32_t* off = offsets + b * ((size_t)max_regions + 1);
    int2* dst = xy + b * (size_t)max_points;
    long long carry = 0;
    for (int j0 = 0; j0 < r; j0 += kOlScanT) {
        const int j = j0 + tid;
        long long len = 0;
        int walk_b0 = -1;                              // >= 0: the ranking did not deliver this record's cycle
        mdx_region R{};
        if (j < r) {
            R = regions[b * max_regions + j];
            if (seed_ok(R, lab, w, h)) {
                const size_t p = (size_t)R.seed_y * w + R.seed_x;
                const unsigned m = nbr[p];
                if (m) {
                    const int b0 = outline_prev_dir(m, 4);
                    const uint32_t s0 = state_index(base, p, m, b0);
                    walk_b0 = b0;
                    // the outline's last state is the start's predecessor: its position + 1 points
                    const size_t pp = (size_t)(R.seed_y + outline_dy(b0)) * w + (R.seed_x + outline_dx(b0));
                    const unsigned mp = nbr[pp];
                    if (mp && word_load(word + s0) == pack(kNil, (uint32_t)j)) {
                        const u64 wt = word_load(word + state_index(base, pp, mp, outline_prev_dir(mp, b0 ^ 4)));
                        const uint32_t a = (uint32_t)(wt >> 32);
                        if (a != kNil && (a & ~kRes) == s0) {
                            len = (long long)(uint32_t)wt + 1;
                            walk_b0 = -1;
                        }
                    }
                } else {
                    const unsigned tm = member_mask(lab, w, h, R.seed_x, R.seed_y, R.id);
                    if (tm)
                        walk_b0 = outline_prev_dir(tm, 4);
                    else
                        len = 1;                       // no neighbour: the single point
                }
                if (walk_b0 >= 0) len = outline_walk(lab, w, h, R.id, R.seed_x, R.seed_y, walk_b0, nullptr, 0);
            }
        }
        long long total;
        const long long pos = carry + block_scan_exclusive_ll<kOlScanT>(len, wsum, total);
        if (j < r) {
            off[j] = (int32_t)min(pos, (long long)INT32_MAX);
            if (walk_b0 >= 0)
                outline_walk(lab, w, h, R.id, R.seed_x, R.seed_y, walk_b0, dst + pos, max(0ll, (long long)max_points - pos));
            else if (len == 1 && pos < max_points)
                dst[pos] = make_int2(R.seed_x, R.seed_y);
        }
        carry += total;
    }
    const int32_t all = (int32_t)min(carry, (long long)INT32_MAX);
    for (int j = r + tid; j <= max_regions; j += kOlScanT) off[j] = all;
    if (tid == 0 && num_points) num_points[b] = all;
}

__global__ __launch_bounds__(kOlT) void k_outline_scatter(int w, int h, const uint8_t* __restrict__ nbr,
                                                          const int32_t* __restrict__ base, const u64* __restrict__ words,
                                                          int max_regions, const int32_t* __restrict__ offsets,
                                                          int2* __restrict__ xy, int max_points)
{
    const size_t N = (size_t)w * h, b = blockIdx.y;
    const size_t p = (size_t)blockIdx.x * kOlT + threadIdx.x;
    if (p >= N) return;
    const unsigned m = nbr[b * N + p];
    if (!m) return;
    const u64* word = words + b * 7 * N;
    const int32_t* off = offsets + b * ((size_t)max_regions + 1);
    int2* dst = xy + b * (size_t)max_points;
    const int2 pt = make_int2((int)(p % w), (int)(p / w));
    uint32_t idx = (uint32_t)base[b * N + p];
    for (int n = __popc(m); n > 0; n--, idx++) {
        uint32_t j, pos;
        if (!state_place(word, word_load(word + idx), j, pos)) continue;
        const long long q = (long long)off[j] + pos;
        if (q < max_points) dst[q] = pt;
    }
}

}  // namespace

static size_t up256(size_t v) { return (v + 255) / 256 * 256; }
static int outline_blocks(int w, int h) { return (int)(((size_t)w * h + kOlT - 1) / kOlT); }

size_t region_outlines_scratch_bytes(int batch, int w, int h, int max_regions, RegionOutlineScratch* lay)
{
    (void)max_regions;
    const size_t B = (size_t)batch, N = (size_t)w * h;
    RegionOutlineScratch L;
    L.words = 0;
    L.base = B * N * 56;
    L.blk = L.base + up256(B * N * 4);
    L.nstates = L.blk + up256(B * (size_t)outline_blocks(w, h) * 4);
    L.flags = L.nstates + up256(B * 4);
    L.nbr = L.flags + B * kOlFlags * 4;
    if (lay) *lay = L;
    return L.nbr + B * N;
}

hipError_t launch_region_outlines(hipStream_t s, int batch, const int32_t* labels, int w, int h, const mdx_region* regions,
                                  int max_regions, const int32_t* num_kept, int32_t* offsets, int32_t* xy, int max_points,
                                  int32_t* num_points, void* scratch, hipEvent_t* ev)
{
    RegionOutlineScratch lay;
    region_outlines_scratch_bytes(batch, w, h, max_regions, &lay);
    char* sc = static_cast<char*>(scratch);
    u64* words = reinterpret_cast<u64*>(sc + lay.words);
    int32_t* base = reinterpret_cast<int32_t*>(sc + lay.base);
    int32_t* blk = reinterpret_cast<int32_t*>(sc + lay.blk);
    int32_t* nstates = reinterpret_cast<int32_t*>(sc + lay.nstates);
    int32_t* flags = reinterpret_cast<int32_t*>(sc + lay.flags);
    uint8_t* nbr = reinterpret_cast<uint8_t*>(sc + lay.nbr);
    int2* pts = reinterpret_cast<int2*>(xy);
    const int nblk = outline_blocks(w, h);
    const dim3 px((unsigned)nblk, (unsigned)batch), img((unsigned)batch);
    if (max_regions == 0 && ev)
        for (int i = 1; i <= 2; i++) (void)hipEventRecord(ev[i], s);
    if (max_regions > 0) {                            // else no record takes part: the offsets alone
        hipLaunchKernelGGL(k_outline_mask, px, dim3(kOlT), 0, s, labels, w, h, nblk, nbr, blk);
        hipLaunchKernelGGL(k_outline_blocks, img, dim3(kOlScanT), 0, s, nblk, blk, nstates, flags);
        hipLaunchKernelGGL(k_outline_base, px, dim3(kOlT), 0, s, w, h, nblk, nbr, blk, base);
        hipLaunchKernelGGL(k_outline_pred, px, dim3(kOlT), 0, s, w, h, nbr, base, words);
        hipLaunchKernelGGL(k_outline_starts, dim3((unsigned)((max_regions + kOlT - 1) / kOlT), (unsigned)batch), dim3(kOlT), 0,
                           s, labels, w, h, regions, max_regions, num_kept, nbr, base, words);
        if (hipError_t e = hipGetLastError()) return e;
        if (ev) (void)hipEventRecord(ev[1], s);
        const size_t per_image = (size_t)w * h * 7;
        const unsigned gx = (unsigned)std::min<size_t>((per_image + kOlT - 1) / kOlT, kOlRoundBlocks);
        const int rounds = outline_rounds(w, h);
        for (int k = 0; k < rounds; k++)
            hipLaunchKernelGGL(k_outline_round, dim3(gx, (unsigned)batch), dim3(kOlT), 0, s, k, per_image, nstates, flags,
                               words);
        if (hipError_t e = hipGetLastError()) return e;
        if (ev) (void)hipEventRecord(ev[2], s);
    }
    hipLaunchKernelGGL(k_outline_offsets, img, dim3(kOlScanT), 0, s, labels, w, h, regions, max_regions,
                       max_regions > 0 ? num_kept : nullptr, nbr, base, words, offsets, pts, max_points, num_points);
    if (ev) (void)hipEventRecord(ev[3], s);
    if (max_regions > 0 && max_points > 0)
        hipLaunchKernelGGL(k_outline_scatter, px, dim3(kOlT), 0, s, w, h, nbr, base, words, max_regions, offsets, pts,
                           max_points);
    if (ev) (void)hipEventRecord(ev[4], s);
    return hipGetLastError();
}

int region_outlines_launches(int w, int h, int max_regions, int max_points)
{
    return max_regions > 0 ? 6 + outline_rounds(w, h) + (max_points > 0) : 1;
}

}  // namespace mdx
