// mdx_cluster.hip -- greedy Euclidean clustering of the live chain's outlier points:
// FlowClusterer::clusterEuclidean (reference common/src/flow_clusterer.cpp:231-269), distance
// PointCluster::getClosestDistance (point_cluster.cpp:63-66).  Pinned against this reading of the
// source; unpinned against a real build (no OpenCV 2.4 here).
//
// The reference visits the points in input order; point i joins the cluster whose nearest member is
// nearest (strict <: the earliest-created cluster on a tie) when that distance is below the
// threshold, and starts a new cluster otherwise.  With root(j) = the first point of j's cluster,
// that is: over all j < i take the lexicographic minimum of the key
//     (s(i, j), root(j)),   s = dx*dx + dy*dy in float, each operation rounded, no FMA
// (sqrt in double is strictly increasing on floats, so d and s order and tie alike; clusters are
// created in root order, so the smallest root is the earliest cluster); if the winner's s passes
// the threshold root(i) = its root, else root(i) = i.  The key is packed (bits of s) << 32 | root:
// s >= +0, so its bits order as unsigned and one 64-bit min carries distance and tie-break.  The
// threshold test sqrt((double)s) < thr is s <= s*, with s* the largest such float found by the
// host (launch_cluster's slim = bits(s*) + 1, 0 when no s passes): exact without a device root.
//
// root(i) depends on earlier points only.  The points are cut into blocks of kClB; launch b
// (k_cluster_step) makes block b's roots final:
//   workgroup 0      block b: its points take the keys of block b-1 (whose roots launch b-1 left
//                    final), which completes their minimum over all earlier blocks.  Then the
//                    block's four waves take turns, wave q owning points 64q .. 64q+63, one per
//                    lane: wave q walks its points in order -- the point whose turn it is has its
//                    final key, its root is decided and broadcast (v_readlane), the later lanes
//                    take its key -- with no LDS traffic and no barrier inside the walk; it then
//                    leaves its 64 points and roots in LDS, and after a barrier the later waves
//                    take their keys.
//   workgroup k > 0  block b+k's points take the keys of block b-1 into their running minimum in
//                    best[] (one thread per point, the sources in LDS).
// A call is ceil(N / kClB) launches on the context's stream, ordered by the launch boundaries
// alone: no workgroup ever waits for another.  N <= kClB is a single launch.  best[] needs no
// clearing: launch 1 is the first to touch it and starts every point from the empty key.
#include "mdx_internal.h"

namespace mdx {

constexpr unsigned long long kClNone = ~0ull;   // the empty key: above every real one, fails every threshold

// s(i, j) as the reference's float expression, un-fused whatever the build flags
__device__ __forceinline__ unsigned long long cluster_key(float xi, float yi, float xj, float yj, uint32_t root)
{
    const float dx = __fsub_rn(xi, xj), dy = __fsub_rn(yi, yj);
    const float s = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
    return ((unsigned long long)__float_as_uint(s) << 32) | root;
}

__device__ __forceinline__ float lane_f(float v, int lane)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// grid: launch 0 one workgroup; launch b > 0: nb - b workgroups (workgroup k = block b + k)
__global__ __launch_bounds__(kClB) void k_cluster_step(const float2* __restrict__ pts, int N, int b, uint32_t slim,
                                                        unsigned long long* __restrict__ best,
                                                        int32_t* __restrict__ root)
{
    __shared__ float sx[kClB], sy[kClB];
    __shared__ uint32_t sr[kClB];
    const int tid = threadIdx.x;
    const int blk = b + (int)blockIdx.x;
    const int i = blk * kClB + tid;                 // this thread's point
    const bool live = i < N;
    const float2 pi = live ? pts[i] : make_float2(0.f, 0.f);
    unsigned long long bk = kClNone;
    if (b > 0) {
        // block b-1 is never the last block, so it is full and its roots are final
        const int j = (b - 1) * kClB + tid;
        const float2 pj = pts[j];
        sx[tid] = pj.x;
        sy[tid] = pj.y;
        sr[tid] = (uint32_t)root[j];
        if (b > 1 && live) bk = best[i];
        __syncthreads();
#pragma unroll 8
        for (int t = 0; t < kClB; t++) {
            const unsigned long long k = cluster_key(pi.x, pi.y, sx[t], sy[t], sr[t]);
            bk = k < bk ? k : bk;
        }
        if (blockIdx.x != 0) {
            if (live) best[i] = bk;
            return;
        }
    }
    // Block b itself.  A dead lane (i >= N) carries a made-up point: it only ever hands keys to
    // later lanes and waves, which are dead too, and stores nothing.
    __shared__ float wx[3][64], wy[3][64];
    __shared__ uint32_t wr[3][64];
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t myroot = 0;
    for (int q = 0; q < 4; q++) {
        if (wave == q) {
            uint32_t klo = (uint32_t)bk, khi = (uint32_t)(bk >> 32);
#pragma unroll 16
            for (int t = 0; t < 64; t++) {
                // lane t has met every earlier point: its key is final
                const uint32_t tlo = (uint32_t)__builtin_amdgcn_readlane((int)klo, t);
                const uint32_t thi = (uint32_t)__builtin_amdgcn_readlane((int)khi, t);
                const float xt = lane_f(pi.x, t), yt = lane_f(pi.y, t);
                const uint32_t rt = thi < slim ? tlo : (uint32_t)(i - lane + t);
                if (lane == t) myroot = rt;
                const unsigned long long k = cluster_key(pi.x, pi.y, xt, yt, rt);
                const bool take = lane > t && k < (((unsigned long long)khi << 32) | klo);
                klo = take ? (uint32_t)k : klo;
                khi = take ? (uint32_t)(k >> 32) : khi;
            }
            if (live) root[i] = (int32_t)myroot;
            if (q < 3) {
                wx[q][lane] = pi.x;
                wy[q][lane] = pi.y;
                wr[q][lane] = myroot;
            }
        }
        if (q == 3) break;
        __syncthreads();
        if (wave > q) {
#pragma unroll 8
            for (int t = 0; t < 64; t++) {
                const unsigned long long k = cluster_key(pi.x, pi.y, wx[q][t], wy[q][t], wr[q][t]);
                bk = k < bk ? k : bk;
            }
        }
    }
}

hipError_t launch_cluster(hipStream_t s, const float* pts, int N, uint32_t slim, unsigned long long* best,
                          int32_t* root)
{
    if (N <= 0 || N > MDX_CLUSTER_MAX_POINTS) return hipErrorInvalidValue;
    const int nb = (N + kClB - 1) / kClB;
    for (int b = 0; b < nb; b++)
        hipLaunchKernelGGL(k_cluster_step, dim3(b == 0 ? 1 : nb - b), dim3(kClB), 0, s,
                           reinterpret_cast<const float2*>(pts), N, b, slim, best, root);
    return hipGetLastError();
}

}  // namespace mdx
