// mdx_vcluster.hip -- first-fit clustering of flow vectors by distance and angle:
// FlowClusterer::getClusters (reference common/src/flow_clusterer.cpp:178-227) with
// VectorCluster::getClosestDistance / getClosestOrientation (vector_cluster.cpp:25-50, :118-139).
// Pinned against this reading of the source; unpinned against a real build (no OpenCV 2.4 here).
//
// The reference visits the active vectors in input order.  Vector i joins the earliest-created
// cluster that has some earlier member j with N(i, j) (distance below the threshold) and some
// earlier member j' with G(i, j') (angular distance below the threshold) -- two separate minima over
// the cluster, so j' need not be j -- and starts a new cluster otherwise.  With root(j) = the first
// vector of j's cluster (clusters are created in root order) that is
//     root(i) = min( {root(j): j < i, N(i, j)}  intersected with  {root(j'): j' < i, G(i, j')} ),  else i.
// The state of a vector is therefore two sets of roots, not a running minimum.
//   N(i, j): s = dx*dx + dy*dy in double, each operation rounded, no FMA; sqrt(s) < thr is s <= s*
//            with s* the largest such double, found by the host (slim; < 0: nothing passes).
//   G(i, j): th = the vector's angle in [0, 2 pi], computed by the host's libm and uploaded;
//            w = |th_i - th_j|, folded to 2 pi - w above pi; w < athr, or trunc(w) < athr under
//            MDX_VCLUSTER_ABS_INT.  No device transcendentals.
//
// The vectors are cut into blocks of kClB.  Block b's roots become final in three launches on the
// context's stream, ordered by the launch boundaries alone (no workgroup ever waits for another):
//   k_vcluster_scan    one workgroup per vector u of block b (b > 0).  Two bitsets indexed by root
//                      in LDS, the words below the block start only; the threads stride over every
//                      j of the earlier blocks (roots final) and set root(j)'s bit in the near set
//                      when N and in the angle set when G (test before the atomic: with coherent
//                      flow almost every pair passes G on a handful of roots).  The AND of the sets
//                      word by word gives qscan[u], the earliest qualifying root among the earlier
//                      blocks' members alone; both rows go to global scratch.
//   k_vcluster_gather  one workgroup per vector u.  (b > 0) The only earlier-block roots the
//                      block's walk can ever hand out are the 256 values qscan[t]: a vector's root
//                      is its own qscan, an earlier in-block vector's root, or itself.  So the
//                      workgroup reads, for every t, whether u's scan rows hold the root qscan[t]:
//                      2 x 256 bits, which takes every root-dependent global read out of the walk.
//                      (all b) It also makes u's in-block N and G against every earlier t of the
//                      block, one pair test per thread, as two 256-bit masks: they do not depend on
//                      roots, and here they cost the serial walk nothing.
//   k_vcluster_walk    one workgroup, thread u owns vector u.  Roots are named by slot: slot
//                      t < 256 is the earlier-block root qscan[t] (the first t with that value),
//                      slot 256 + t the block's own vector t.  Each thread keeps its near and angle
//                      sets over the 512 slots in LDS (thread-private words, no races), seeded by
//                      the gather.  Then, as k_cluster_step does, the four waves take turns: wave q
//                      walks its 64 vectors in order -- the vector whose turn it is has its final
//                      root, broadcast with v_readlane; every later lane with N or G towards it
//                      adds that root to its set and, when both sets then hold it, lowers its own
//                      candidate.  The walk itself runs in registers (see there); the wave then
//                      leaves its roots in LDS, one entry per distinct root with the mask of the
//                      lanes that took it, and after a barrier the later waves add them to their
//                      LDS sets.
// A call is 3 * ceil(n / kClB) - 1 launches.  Nothing needs clearing between calls: every word a
// launch reads was written by an earlier launch of the same call.
#include "mdx_internal.h"

#include <algorithm>

namespace mdx {

constexpr uint32_t kVcNone = 0xffffffffu;   // no qualifying root

// N(i, j): the reference's double expression, un-fused whatever the build flags
__device__ __forceinline__ bool vc_near(double xi, double yi, double xj, double yj, double slim)
{
    const double dx = __dsub_rn(xi, xj), dy = __dsub_rn(yi, yj);
    return __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)) <= slim;
}

// G(i, j): |atan2(sin d, cos d)| of the angle difference by its definition
__device__ __forceinline__ bool vc_angle(double ti, double tj, double athr, int abs_int)
{
    constexpr double kPi = 3.14159265358979323846, k2Pi = 2 * kPi;
    double w = fabs(__dsub_rn(ti, tj));
    if (w > kPi) w = __dsub_rn(k2Pi, w);
    return (abs_int ? trunc(w) : w) < athr;
}

// grid: the block's vectors; dynamic LDS: 2 * 8 b words
__global__ __launch_bounds__(kClB) void k_vcluster_scan(const double* __restrict__ xs, const double* __restrict__ ys,
                                                         const double* __restrict__ ths,
                                                         const int32_t* __restrict__ root, int b, double slim,
                                                         double athr, int abs_int, uint32_t* __restrict__ rows,
                                                         int W, uint32_t* __restrict__ qscan)
{
    extern __shared__ uint32_t vc_sets[];
    __shared__ uint32_t best;
    const int tid = threadIdx.x, u = blockIdx.x;
    const int nw = b * (kClB / 32), nj = b * kClB;
    uint32_t* nearset = vc_sets;
    uint32_t* angset = vc_sets + nw;
    for (int k = tid; k < 2 * nw; k += kClB) vc_sets[k] = 0;
    if (tid == 0) best = kVcNone;
    __syncthreads();
    const int i = nj + u;
    const double xi = xs[i], yi = ys[i], ti = ths[i];
    for (int j = tid; j < nj; j += kClB) {
        const uint32_t r = (uint32_t)root[j], bit = 1u << (r & 31);
        if (vc_near(xi, yi, xs[j], ys[j], slim) && !(nearset[r >> 5] & bit)) atomicOr(&nearset[r >> 5], bit);
        if (vc_angle(ti, ths[j], athr, abs_int) && !(angset[r >> 5] & bit)) atomicOr(&angset[r >> 5], bit);
    }
    __syncthreads();
    uint32_t mine = kVcNone;
    uint32_t* rn = rows + (size_t)(2 * u) * W;
    uint32_t* ra = rn + W;
    for (int k = tid; k < nw; k += kClB) {     // ascending per thread: its first hit is its lowest
        const uint32_t a = nearset[k], g = angset[k];
        rn[k] = a;
        ra[k] = g;
        if ((a & g) && mine == kVcNone) mine = (uint32_t)k * 32 + (uint32_t)__ffs((int)(a & g)) - 1;
    }
    if (mine != kVcNone) atomicMin(&best, mine);
    __syncthreads();
    if (tid == 0) qscan[u] = best;
}

// grid: the block's cnt vectors.  cand[u][0..7] bit t: u's near row holds qscan[t]; [8..15]: its angle
// row; [16..23] bit t: N(u, t), t < u; [24..31]: G(u, t), t < u
__global__ __launch_bounds__(kClB) void k_vcluster_gather(const double* __restrict__ xs, const double* __restrict__ ys,
                                                           const double* __restrict__ ths, int b, double slim,
                                                           double athr, int abs_int,
                                                           const uint32_t* __restrict__ rows, int W,
                                                           const uint32_t* __restrict__ qscan, int cnt,
                                                           uint32_t* __restrict__ cand)
{
    const int t = threadIdx.x, u = blockIdx.x, start = b * kClB;
    const uint32_t c = (b > 0 && t < cnt) ? qscan[t] : kVcNone;
    bool bn = false, ba = false, pn = false, pg = false;
    if (c != kVcNone) {
        const uint32_t* rn = rows + (size_t)(2 * u) * W;
        bn = (rn[c >> 5] >> (c & 31)) & 1;
        ba = (rn[W + (c >> 5)] >> (c & 31)) & 1;
    }
    if (t < u) {     // u < cnt, so t is a vector of the block too
        pn = vc_near(xs[start + u], ys[start + u], xs[start + t], ys[start + t], slim);
        pg = vc_angle(ths[start + u], ths[start + t], athr, abs_int);
    }
    const unsigned long long m[4] = {__ballot(bn), __ballot(ba), __ballot(pn), __ballot(pg)};
    if ((t & 63) == 0)
        for (int k = 0; k < 4; k++) {
            cand[u * 32 + 8 * k + 2 * (t >> 6)] = (uint32_t)m[k];
            cand[u * 32 + 8 * k + 2 * (t >> 6) + 1] = (uint32_t)(m[k] >> 32);
        }
}

// One root (value rv, slot s) met by a thread whose in-block tests towards its owners are n and g:
// the slot joins the thread's sets, and lowers its candidate once both hold it.
__device__ __forceinline__ void vc_take(uint32_t (*sn)[kClB], uint32_t (*sa)[kClB], int u, uint32_t n, uint32_t g,
                                        uint32_t rv, uint32_t s, uint32_t& qv, uint32_t& qs)
{
    if (!(n | g)) return;
    const uint32_t wi = s >> 5, sh = s & 31;
    const uint32_t a = sn[wi][u] | (n << sh), c = sa[wi][u] | (g << sh);
    sn[wi][u] = a;
    sa[wi][u] = c;
    if (((a & c) >> sh) & 1u && rv < qv) {
        qv = rv;
        qs = s;
    }
}

// grid: 1
__global__ __launch_bounds__(kClB) void k_vcluster_walk(int nA, int b, const uint32_t* __restrict__ qscan,
                                                         const uint32_t* __restrict__ cand,
                                                         int32_t* __restrict__ root)
{
    __shared__ uint32_t sn[16][kClB], sa[16][kClB];      // near / angle sets over the 512 slots, word-major
    __shared__ uint32_t mn[kClB / 32][kClB], mg[kClB / 32][kClB];   // in-block N / G towards every earlier t
    __shared__ uint32_t sc[kClB];
    // what a wave leaves for the later ones: per distinct root its value, slot and the lanes that took it
    __shared__ uint32_t wrv[3][64], wsl[3][64], wcnt[3];
    __shared__ unsigned long long weq[3][64];
    const int u = threadIdx.x, lane = u & 63, wave = u >> 6;
    const int start = b * kClB, i = start + u;
    const bool live = i < nA;
    uint32_t qv = (b > 0 && live) ? qscan[u] : kVcNone;
    sc[u] = qv;
    for (int k = 0; k < 8; k++) {
        sn[k][u] = (b > 0 && live) ? cand[u * 32 + k] : 0u;
        sa[k][u] = (b > 0 && live) ? cand[u * 32 + 8 + k] : 0u;
        sn[8 + k][u] = 0;
        sa[8 + k][u] = 0;
        // a dead thread (i >= nA) takes nothing and stores nothing: it only hands its own slot to
        // later threads, which are dead too
        mn[k][u] = live ? cand[u * 32 + 16 + k] : 0u;
        mg[k][u] = live ? cand[u * 32 + 24 + k] : 0u;
    }
    __syncthreads();
    // the slot of an earlier-block root: the first t whose qscan is that value
    uint32_t qs = (uint32_t)u;
    if (qv != kVcNone)
        for (int t = u - 1; t >= 0; t--)
            if (sc[t] == qv) qs = (uint32_t)t;
#pragma unroll 1
    for (int q = 0; q < 4; q++) {
        const unsigned long long a64 = mn[2 * q][u] | (unsigned long long)mn[2 * q + 1][u] << 32;
        const unsigned long long g64 = mg[2 * q][u] | (unsigned long long)mg[2 * q + 1][u] << 32;
        if (wave == q) {
            // The wave's own walk touches no LDS.  Every root it hands out is named by a lane id: a
            // lane's root is the candidate it entered the walk with (id j: the first lane that
            // entered with that slot), an earlier lane's root, or its own vector (id t: lane t
            // entered without a candidate, so j and t never collide).  What a lane's sets held of
            // the entering slots is read here, before the walk; what the walk adds is the two
            // 64-bit sets over ids, nid and aid.
            const uint32_t qv0 = qv, qs0 = qs;
            uint32_t qid = (uint32_t)lane;
            unsigned long long nid = 0, aid = 0;
#pragma unroll 4
            for (int j = 63; j >= 0; j--) {
                const uint32_t qvj = (uint32_t)__builtin_amdgcn_readlane((int)qv0, j);
                const uint32_t qsj = (uint32_t)__builtin_amdgcn_readlane((int)qs0, j);
                if (qvj == kVcNone) continue;     // wave-uniform
                if (qv0 != kVcNone && qs0 == qsj) qid = (uint32_t)j;
                nid |= (unsigned long long)((sn[qsj >> 5][u] >> (qsj & 31)) & 1u) << j;
                aid |= (unsigned long long)((sa[qsj >> 5][u] >> (qsj & 31)) & 1u) << j;
            }
#pragma unroll 8
            for (int t = 0; t < 64; t++) {
                // lane t has met every earlier vector: its candidate is final
                const uint32_t qvt = (uint32_t)__builtin_amdgcn_readlane((int)qv, t);
                const uint32_t qit = (uint32_t)__builtin_amdgcn_readlane((int)qid, t);
                const bool own = qvt == kVcNone;
                const uint32_t rv = own ? (uint32_t)(start + 64 * q + t) : qvt;
                const uint32_t id = own ? (uint32_t)t : qit;
                const unsigned long long m = 1ull << id;
                const bool n = (a64 >> t) & 1, g = (g64 >> t) & 1;
                nid |= n ? m : 0ull;
                aid |= g ? m : 0ull;
                if ((n || g) && (nid & aid & m) != 0 && rv < qv) {
                    qv = rv;
                    qid = id;
                }
            }
            // a lane's candidate cannot change after its own turn: it is its root
            const bool own = qv == kVcNone;
            const uint32_t myroot = own ? (uint32_t)i : qv, myid = own ? (uint32_t)lane : qid;
            // the slot of that root, for the later waves' sets: the entering slot of lane myid, or,
            // where that lane entered without a candidate, its vector's own slot
            const uint32_t ev = (uint32_t)__shfl((int)qv0, (int)myid), es = (uint32_t)__shfl((int)qs0, (int)myid);
            const uint32_t myslot = ev != kVcNone ? es : (uint32_t)(kClB + 64 * q) + myid;
            if (live) root[i] = (int32_t)myroot;
            if (q < 3) {
                unsigned long long rem = __ballot(live);
                uint32_t d = 0;
                while (rem) {
                    const int t0 = __ffsll((long long)rem) - 1;
                    const uint32_t s0 = (uint32_t)__builtin_amdgcn_readlane((int)myslot, t0);
                    const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)myroot, t0);
                    const unsigned long long eq = __ballot(live && myslot == s0);
                    if (lane == 0) {
                        wrv[q][d] = r0;
                        wsl[q][d] = s0;
                        weq[q][d] = eq;
                    }
                    rem &= ~eq;
                    d++;
                }
                if (lane == 0) wcnt[q] = d;
            }
        }
        if (q == 3) break;
        __syncthreads();
        if (wave > q) {
            const uint32_t cntd = wcnt[q];
            for (uint32_t d = 0; d < cntd; d++) {
                const unsigned long long eq = weq[q][d];
                vc_take(sn, sa, u, (a64 & eq) != 0, (g64 & eq) != 0, wrv[q][d], wsl[q][d], qv, qs);
            }
        }
    }
}

size_t vcluster_rows_bytes(int nA)
{
    const size_t nb = ((size_t)std::max(nA, 1) + kClB - 1) / kClB;
    return (size_t)kClB * 2 * nb * (kClB / 32) * 4;
}

hipError_t launch_vcluster(hipStream_t s, const double* xyt, int nA, double slim, double athr, int abs_int,
                           uint32_t* rows, uint32_t* qscan, uint32_t* cand, int32_t* root)
{
    if (nA <= 0 || nA > MDX_VCLUSTER_MAX_POINTS) return hipErrorInvalidValue;
    const int nb = (nA + kClB - 1) / kClB, W = nb * (kClB / 32);
    const double *xs = xyt, *ys = xyt + nA, *ths = xyt + 2 * (size_t)nA;
    for (int b = 0; b < nb; b++) {
        const int cnt = std::min(kClB, nA - b * kClB);
        if (b > 0)
            hipLaunchKernelGGL(k_vcluster_scan, dim3(cnt), dim3(kClB), (size_t)2 * b * (kClB / 32) * 4, s, xs, ys, ths,
                               root, b, slim, athr, abs_int, rows, W, qscan);
        hipLaunchKernelGGL(k_vcluster_gather, dim3(cnt), dim3(kClB), 0, s, xs, ys, ths, b, slim, athr, abs_int, rows, W,
                           qscan, cnt, cand);
        hipLaunchKernelGGL(k_vcluster_walk, dim3(1), dim3(kClB), 0, s, nA, b, qscan, cand, root);
    }
    return hipGetLastError();
}

}  // namespace mdx
