// mdx_subspace.hip -- trajectory subspace RANSAC:
// OutlierDetector::fitSubspace (reference common/src/outlier_detector.cpp:236-331).
//
//   data      n x N floats, column i = trajectory i's (x, y) points, mean-subtracted with the
//             reference's quirks (meanSubtract :200-221: the means of rows 0 / 1 only, float sums
//             in column order, y flipped)                                   -> k_subspace_prep
//   50 x      d = 4*num_motions columns drawn by rand() % N (host-side glibc rand restatement);
//             Pnd = I - U_d U_d' from the sample's SVD = Q2 Q2' with Q2 the last n - d columns of
//             the sample's Householder Q; residual_i = |x_i' Pnd x_i| = ||Q2' x_i||^2; inliers:
//             residual < (n - d) sigma^2                                     -> k_subspace_hyp
//   winner    the first hypothesis with the most inliers (strict >, :300); outliers: its residual
//             > sigma^2 chi2_99[n - d] (:312-323)                            -> k_subspace_final
//
// Precision MDX_SUBSPACE_F64 (default) as above; MDX_SUBSPACE_F32 follows the reference's float
// arithmetic shape instead (explicit float Pnd, residual |x' (Pnd x)|).  The two modes are the
// policies SubF64 / SubF32 (element type, basis size, build, residual); k_subspace_hyp<P> and
// k_subspace_final<P> are written once, and so are the Householder factorisation and the columns
// of Q (householder_wave<T>, q_column<T>) both modes' bases come from.  The arithmetic follows the
// oracle's restatement (oracle/mdx_oracle.c) operation for operation, un-fused, so both round
// identically.
#include "mdx_internal.h"

#include <algorithm>

namespace mdx {

constexpr int kMaxSub = 32;   // n = 2 * trajectory length (reference: 10 / 14 / 18 for 2..4 motions)

// acc = acc + v as one v_add_f32 (round to nearest even, like the compiler's).  Written out so
// the x and y chains stay two scalar chains: the compiler pairs them into one v_pk_add_f32 chain,
// whose dependent issue is several times slower (k_subspace_prep 306 us -> see DESIGN §7c).
__device__ __forceinline__ void fadd(float& acc, float v)
{
    asm volatile("v_add_f32 %0, %0, %1" : "+v"(acc) : "v"(v));
}

// meanSubtract.  One workgroup: the row-0 / row-1 sums are sequential float sums (Eigen's
// row().sum() on a column-major matrix visits the columns in order), staged through LDS in
// chunks so lane 0's dependent adds read LDS, not HBM.
__global__ __launch_bounds__(256) void k_subspace_prep(const float* __restrict__ traj, int N, int T,
                                                        float* __restrict__ mean)
{
    constexpr int kChunk = 4096;
    __shared__ __attribute__((aligned(16))) float sx[kChunk], sy[kChunk];
    __shared__ float s_ys;
    const int tid = threadIdx.x;
    float xs = 0.f, ys = 0.f;
    for (int base = 0; base < N; base += kChunk) {
        const int m = min(kChunk, N - base);
        for (int i = tid; i < m; i += 256) {
            sx[i] = traj[(long long)(base + i) * T * 2];
            sy[i] = traj[(long long)(base + i) * T * 2 + 1];
        }
        __syncthreads();
        if (tid == 0 || tid == 64) {
            // the reference's order exactly: one float chain per axis, the x chain on lane 0 of
            // wave 0 and the y chain on lane 0 of wave 1 (two SIMDs: a lone wave's dependent adds
            // issue slowly, so two chains in one wave ran at half this rate).  16 values are read
            // with ds_read_b128 one block ahead of the adds (software pipelined).
            const float* sv = tid ? sy : sx;
            float acc = tid ? ys : xs;
            int i = 0;
            if (base == 0) { acc = sv[0]; i = 1; }
            for (; i < m && (i & 3); i++) fadd(acc, sv[i]);
            auto add16 = [&](const float4 (&v)[4]) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    fadd(acc, v[k].x);
                    fadd(acc, v[k].y);
                    fadd(acc, v[k].z);
                    fadd(acc, v[k].w);
                }
            };
            auto ld16 = [&](float4 (&v)[4], int at) {
#pragma unroll
                for (int k = 0; k < 4; k++) v[k] = reinterpret_cast<const float4*>(sv + at)[k];
            };
            if (i + 32 <= m) {
                // two blocks of 16 in flight ahead of the adds (one block ahead left each block's
                // LDS latency exposed: ~20 cycles per dependent add)
                float4 a4[4], b4[4], c4[4];
                ld16(a4, i);
                ld16(b4, i + 16);
                for (; i + 48 <= m; i += 48) {
                    ld16(c4, i + 32);
                    add16(a4);
                    if (i + 64 > m) { add16(b4); add16(c4); i += 48; goto drained; }
                    ld16(a4, i + 48);
                    add16(b4);
                    if (i + 80 > m) { add16(c4); add16(a4); i += 64; goto drained; }
                    ld16(b4, i + 64);
                    add16(c4);
                }
                // a4, b4 loaded (blocks at i, i + 16), fewer than 16 more after them
                add16(a4);
                add16(b4);
                i += 32;
            drained:;
            }
            for (; i < m; i++) fadd(acc, sv[i]);
            if (tid) ys = acc;
            else xs = acc;
        }
        __syncthreads();
    }
    if (tid == 64) s_ys = ys;
    __syncthreads();
    if (tid == 0) {
        double xm = (double)xs, ym = (double)s_ys;
        xm /= N;
        ym /= N;
        mean[0] = (float)xm;
        mean[1] = (float)ym;
    }
}

// The centred data, one trajectory per thread over the whole grid (this pass ran inside
// k_subspace_prep's single workgroup with a 64-bit modulo per element: ~190 us of its 306 us).
__global__ __launch_bounds__(256) void k_subspace_center(const float* __restrict__ traj, int N, int n,
                                                          const float* __restrict__ mean, float* __restrict__ data)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float xc = mean[0], yc = mean[1];
    const float* t = traj + (long long)i * n;
    float* d = data + (long long)i * n;
    for (int r = 0; r < n; r += 2) {
        d[r] = t[r] - xc;
        d[r + 1] = yc - t[r + 1];
    }
}

// A wave's LDS accesses complete in order; the fences keep the compiler from moving them across the
// hand-offs between lane 0 and the other lanes.
__device__ __forceinline__ void lane_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double sqrt_of(double v) { return __builtin_sqrt(v); }
__device__ __forceinline__ float sqrt_of(float v) { return __builtin_sqrtf(v); }

// Householder QR of the n x d sample in T, the oracle's subspace_basis / subspace_pnd_f32 statement
// for statement; A, V column-major with leading dimension n, reflector k in column k of V (rows
// k..n-1), beta[k] = v'v.  On the 64 lanes of one wave: lane 0 forms each reflector (norm, v, beta),
// then every lane applies it to its own columns c = k + lane, k + lane + 64, ... -- each column's
// dot product and update in the serial order, so the results are identical; only the independent
// columns run side by side (the factorisation by one lane was the hypothesis kernel's serial
// critical path).
template <typename T>
__device__ void householder_wave(T* A, int n, int d, T* V, T* beta, int lane)
{
    for (int k = 0; k < d; k++) {
        if (lane == 0) {
            T nrm2 = T(0);
            for (int r = k; r < n; r++) nrm2 = nrm2 + A[k * n + r] * A[k * n + r];
            const T nrm = sqrt_of(nrm2);
            const T x0 = A[k * n + k];
            const T alpha = x0 >= T(0) ? -nrm : nrm;
            for (int r = k; r < n; r++) V[k * n + r] = A[k * n + r];
            V[k * n + k] = x0 - alpha;
            T b = T(0);
            for (int r = k; r < n; r++) b = b + V[k * n + r] * V[k * n + r];
            beta[k] = b;
        }
        lane_lds_sync();
        const T b = beta[k];
        if (b != T(0)) {
            for (int c = k + lane; c < d; c += 64) {
                T dot = T(0);
                for (int r = k; r < n; r++) dot = dot + V[k * n + r] * A[c * n + r];
                const T f = T(2) * dot / b;
                for (int r = k; r < n; r++) A[c * n + r] = A[c * n + r] - f * V[k * n + r];
            }
        }
        lane_lds_sync();
    }
}

// Column j of Q = H_0 ... H_{d-1}: q = e_j, then the reflectors d-1 ... 0.  One lane per column.
template <typename T>
__device__ void q_column(const T* V, const T* beta, int n, int d, int j, T* q)
{
    for (int r = 0; r < n; r++) q[r] = r == j ? T(1) : T(0);
    for (int k = d - 1; k >= 0; k--) {
        if (beta[k] == T(0)) continue;
        T dot = T(0);
        for (int r = k; r < n; r++) dot = dot + V[k * n + r] * q[r];
        const T f = T(2) * dot / beta[k];
        for (int r = k; r < n; r++) q[r] = q[r] - f * V[k * n + r];
    }
}

// The two precision modes: the element type, the size of a hypothesis' basis, how one wave builds
// it from the sample A (n x d, factored in place; V, beta: the reflectors) and a trajectory's
// residual against it.  Both follow the oracle (oracle/mdx_oracle.c) operation for operation.

// MDX_SUBSPACE_F64: basis = Q2, the last n - d columns of Q (column-major, n x (n-d));
// residual = ||Q2' x||^2 in double (the oracle's subspace_basis / subspace_residual).
struct SubF64 {
    using T = double;
    static __host__ __device__ int basis_elems(int n, int d) { return n * (n - d); }
    static __device__ __forceinline__ void build(T* A, int n, int d, T* V, T* beta, T* q2, int lane)
    {
        householder_wave(A, n, d, V, beta, lane);
        for (int j = d + lane; j < n; j += 64) q_column(V, beta, n, d, j, q2 + (j - d) * n);
    }
    static __device__ __forceinline__ double residual(const T* q2, int n, int d, const float* x)
    {
        double res = 0.0;
        for (int j = 0; j < n - d; j++) {
            double p = 0.0;
            for (int r = 0; r < n; r++) p = p + q2[j * n + r] * (double)x[r];
            res = res + p * p;
        }
        return res;
    }
};

// MDX_SUBSPACE_F32: the reference's float arithmetic shape -- basis = Pnd = I - sum_j u_j u_j' formed
// explicitly (outlier_detector.cpp:272-282; n x n row-major), u_j the first d columns of Q; residual
// = |x' (Pnd x)| as the two float products of :286 (the oracle's subspace_pnd_f32 /
// subspace_residual_f32).
struct SubF32 {
    using T = float;
    static __host__ __device__ int basis_elems(int n, int d) { return n * n; }
    static __device__ __forceinline__ void build(T* A, int n, int d, T* V, T* beta, T* P, int lane)
    {
        householder_wave(A, n, d, V, beta, lane);
        // the factored sample is not read again: its n x d storage takes the d columns of Q
        T* Q = A;
        for (int j = lane; j < d; j += 64) q_column(V, beta, n, d, j, Q + j * n);
        lane_lds_sync();
        // one entry per lane, each summed over j in ascending order from 0 as the oracle's
        // Pnd = Pnd + u_j u_j' does entry by entry
        for (int e = lane; e < n * n; e += 64) {
            const int a = e / n, b = e - a * n;
            T p = 0.0f;
            for (int j = 0; j < d; j++) p = p + Q[j * n + a] * Q[j * n + b];
            P[e] = (a == b ? 1.0f : 0.0f) - p;
        }
    }
    static __device__ __forceinline__ double residual(const T* P, int n, int d, const float* x)
    {
        float res = 0.0f;
        for (int a = 0; a < n; a++) {
            float y = 0.0f;
            for (int b = 0; b < n; b++) y = y + P[a * n + b] * x[b];
            res = res + x[a] * y;
        }
        return (double)__builtin_fabsf(res);
    }
};

size_t subspace_basis_bytes(int n, int d, int precision)
{
    return precision == MDX_SUBSPACE_F32 ? SubF32::basis_elems(n, d) * sizeof(SubF32::T)
                                         : SubF64::basis_elems(n, d) * sizeof(SubF64::T);
}

// grid: (hypothesis, slice of the trajectories), one workgroup each.  cols: [nhyp][d] sample
// indices; basis: [nhyp][P::basis_elems] (written by slice 0); counts: [nhyp] inliers, zeroed.
// Wave 0 builds the basis of the tiny n x d sample (n <= 32) in LDS, the workgroup then streams its
// slice's columns and adds its inlier count.
template <class P>
__global__ __launch_bounds__(256) void k_subspace_hyp(const float* __restrict__ data, int N, int n, int d,
                                                       const int* __restrict__ cols, double inlier_thr,
                                                       typename P::T* __restrict__ basis, int* __restrict__ counts)
{
    using T = typename P::T;
    __shared__ T sA[kMaxSub * kMaxSub], sV[kMaxSub * kMaxSub], sbeta[kMaxSub];
    __shared__ T sB[kMaxSub * kMaxSub];
    __shared__ int s_cnt[4];
    const int h = blockIdx.x, tid = threadIdx.x, nb = P::basis_elems(n, d);
    const int i0 = (int)((long long)N * blockIdx.y / gridDim.y), i1 = (int)((long long)N * (blockIdx.y + 1) / gridDim.y);
    for (int e = tid; e < n * d; e += 256) {
        const int k = e / n, r = e - k * n;
        sA[e] = (T)data[(long long)cols[h * d + k] * n + r];
    }
    __syncthreads();
    if (tid < 64) P::build(sA, n, d, sV, sbeta, sB, tid);
    __syncthreads();
    if (blockIdx.y == 0)
        for (int e = tid; e < nb; e += 256) basis[(long long)h * nb + e] = sB[e];
    int cnt = 0;
    for (int i = i0 + tid; i < i1; i += 256)
        if (P::residual(sB, n, d, data + (long long)i * n) < inlier_thr) cnt++;
    for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) atomicAdd(counts + h, s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]);
}

// Winner = the first hypothesis with the largest positive count; its residual per trajectory and
// the outlier flags.  best[0] = winner index or -1 (no hypothesis had an inlier).
template <class P>
__global__ __launch_bounds__(256) void k_subspace_final(const float* __restrict__ data, int N, int n, int d,
                                                         int nhyp, const int* __restrict__ counts,
                                                         const typename P::T* __restrict__ basis, double out_thr,
                                                         double* __restrict__ residuals,
                                                         uint8_t* __restrict__ is_outlier, int* __restrict__ best)
{
    int bh = -1, bc = 0;
    for (int h = 0; h < nhyp; h++)
        if (counts[h] > bc) { bc = counts[h]; bh = h; }
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) best[0] = bh;
    if (i >= N) return;
    double r = 0.0;
    if (bh >= 0) r = P::residual(basis + (long long)bh * P::basis_elems(n, d), n, d, data + (long long)i * n);
    if (residuals) residuals[i] = r;
    is_outlier[i] = (uint8_t)(bh >= 0 && r > out_thr);
}

hipError_t launch_subspace(hipStream_t s, const float* traj, int N, int T, int d, const int* cols, int nhyp,
                           double sigma, float* data, void* basis, int* counts, double* residuals,
                           uint8_t* is_outlier, int* best, int precision)
{
    const int n = 2 * T;
    // n - d == 10: the reference's chi_square_table.at(0).at(10) throws (outlier_detector.cpp:315)
    if (N <= 0 || d <= 0 || d > n || n > kMaxSub || nhyp <= 0 || n - d == 10) return hipErrorInvalidValue;
    const double inlier_thr = (double)(n - d) * sigma * sigma;
    // chi-square 99% table (outlier_detector.cpp:19-30), indexed by n - d; 0.2 outside 1..10 (:311)
    static const double p99[10] = {0.0, 0.020, 0.115, 0.297, 0.554, 0.872, 1.239, 1.646, 2.088, 2.558};
    const double out_thr = (n - d > 0 && n - d < 10) ? sigma * sigma * p99[n - d] : 0.2;
    // the two means go to the scratch word after the data ([N * n] floats, then 2)
    float* mean = data + (size_t)N * n;
    hipLaunchKernelGGL(k_subspace_prep, dim3(1), dim3(256), 0, s, traj, N, T, mean);
    hipLaunchKernelGGL(k_subspace_center, dim3((N + 255) / 256), dim3(256), 0, s, traj, N, n, mean, data);
    // every hypothesis over S slices of the trajectories (one workgroup each, the basis recomputed per
    // slice, inlier counts added atomically -- an order-free integer sum): one workgroup per hypothesis
    // left 50 of 256 CUs streaming ~20K trajectories each at one wave per SIMD, latency-bound
    const int S = std::max(1, std::min(16, N / 1024));
    if (hipError_t e = hipMemsetAsync(counts, 0, sizeof(int) * (size_t)nhyp, s)) return e;
    auto fit = [&](auto mode) {
        using P = decltype(mode);
        auto* b = static_cast<typename P::T*>(basis);
        hipLaunchKernelGGL(k_subspace_hyp<P>, dim3(nhyp, S), dim3(256), 0, s, data, N, n, d, cols, inlier_thr, b, counts);
        hipLaunchKernelGGL(k_subspace_final<P>, dim3((N + 255) / 256), dim3(256), 0, s, data, N, n, d, nhyp, counts, b,
                           out_thr, residuals, is_outlier, best);
    };
    if (precision == MDX_SUBSPACE_F32) fit(SubF32{});
    else fit(SubF64{});
    return hipGetLastError();
}

}  // namespace mdx
