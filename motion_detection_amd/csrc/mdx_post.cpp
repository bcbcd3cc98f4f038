// mdx_post.cpp -- what follows the flow: the reference's random stream, the trajectory subspace
// fit (OutlierDetector::fitSubspace), Euclidean clustering (FlowClusterer::clusterEuclidean), flow
// vectors clustered by distance and angle (getClusters), the kept clusters' convex hulls
// (showClusterContours), the flow vectors' median / MAD outliers (findOutliers), the pair path's mask labelled
// into regions (BackgroundSubtractor::getMotionContours' recipe), those regions' convex hulls and which of
// them lies inside which (its RETR_EXTERNAL).
#include "mdx_ctx.h"

#include <cfloat>
#include <cmath>
#include <cstring>

using namespace mdx;

// glibc rand() (random_r TYPE_3), the generator of fitSubspace's samples
// (outlier_detector.cpp:17 srand(time(NULL)), :226 rand() % data.cols()).
extern "C" void mdx_srand(mdx_rand_state* st, uint32_t seed)
{
    int32_t r[34];
    r[0] = (int32_t)(seed ? seed : 1u);
    for (int i = 1; i < 31; i++) {
        const int64_t hi = r[i - 1] / 127773, lo = r[i - 1] % 127773;
        int64_t word = 16807 * lo - 2836 * hi;
        if (word < 0) word += 2147483647;
        r[i] = (int32_t)word;
    }
    for (int i = 31; i < 34; i++) r[i] = r[i - 31];
    for (int i = 0; i < 34; i++) st->x[i] = (uint32_t)r[i];
    st->pos = 34;
    for (int k = 0; k < 310; k++) (void)mdx_rand(st);
}

extern "C" int mdx_rand(mdx_rand_state* st)
{
    const int i = st->pos;                       // ring of 34: x[i] = x[i-31] + x[i-3]
    const uint32_t v = st->x[(i - 31) % 34] + st->x[(i - 3) % 34];
    st->x[i % 34] = v;
    st->pos = (i + 1) % 34 + 34;
    return (int)(v >> 1);
}

// fitSubspace (outlier_detector.cpp:236-331): samples drawn on the host from the caller's
// generator state (the reference's OutlierDetector keeps one stream across calls), the rest on
// the device (mdx_subspace.hip).
extern "C" int mdx_fit_subspace(mdx_ctx* c, const float* traj, int ntraj, int traj_len, int num_motions, double sigma,
                                mdx_rand_state* rng, int* columns, uint8_t* is_outlier, double* residuals,
                                float* outlier_points, int* n_outliers)
{
    if (!c) return MDX_EINVAL;
    const int n = 2 * traj_len, d = 4 * num_motions;
    if (!traj || !rng || ntraj <= 0 || traj_len < 1 || num_motions < 1)
        return set_err(c, MDX_EINVAL, "mdx_fit_subspace: bad argument (the reference needs >= 1 trajectory: rand() %% 0)");
    if (d > n) return set_err(c, MDX_EINVAL, "mdx_fit_subspace: 4*num_motions > 2*traj_len (reference reads U past its columns)");
    if (n > 32) return set_err(c, MDX_EINVAL, "mdx_fit_subspace: trajectories longer than 16 points");
    if (n - d == 10) return set_err(c, MDX_EINVAL, "mdx_fit_subspace: n - d == 10 (reference chi_square_table.at(10) throws)");
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    constexpr int kHyp = 50;                      // num_iterations (:250)
    std::vector<int> cols((size_t)kHyp * d);
    for (auto& v : cols) v = mdx_rand(rng) % ntraj;   // fillSubset, hypothesis by hypothesis (:223-230)
    const size_t N = (size_t)ntraj;
    const size_t qb = subspace_basis_bytes(n, d, c->prm.subspace_precision);
    const int rc = ensure_all(c, {{&c->straj, N * n * 4}, {&c->sdata, (N * n + 2) * 4},   // + the two means
                                  {&c->sq, (size_t)kHyp * qb}, {&c->scnt, kHyp * 4}, {&c->scols, cols.size() * 4},
                                  {&c->sres, N * 8}, {&c->sout, N}, {&c->sbest, 4}});
    if (rc != MDX_OK) return rc;
    hipStream_t s = c->stream;
    HIP_OR_RETURN(c, hipMemcpyAsync(c->straj.p, traj, N * n * 4, hipMemcpyHostToDevice, s));
    HIP_OR_RETURN(c, hipMemcpyAsync(c->scols.p, cols.data(), cols.size() * 4, hipMemcpyHostToDevice, s));
    HIP_OR_RETURN(c, launch_subspace(s, c->straj.as<float>(), ntraj, traj_len, d, c->scols.as<int>(), kHyp, sigma,
                                     c->sdata.as<float>(), c->sq.p, c->scnt.as<int>(), c->sres.as<double>(),
                                     c->sout.as<uint8_t>(), c->sbest.as<int>(), c->prm.subspace_precision));
    std::vector<uint8_t> out(N);
    int best = -1;
    HIP_OR_RETURN(c, hipMemcpyAsync(out.data(), c->sout.p, N, hipMemcpyDeviceToHost, s));
    if (residuals) HIP_OR_RETURN(c, hipMemcpyAsync(residuals, c->sres.p, N * 8, hipMemcpyDeviceToHost, s));
    HIP_OR_RETURN(c, hipMemcpyAsync(&best, c->sbest.p, 4, hipMemcpyDeviceToHost, s));
    HIP_OR_RETURN(c, hipStreamSynchronize(s));
    int nout = 0;
    for (size_t i = 0; i < N; i++) {
        if (!out[i]) continue;
        if (outlier_points) {     // the trajectory's second-to-last point (:322)
            const int j = traj_len >= 2 ? traj_len - 2 : 0;
            outlier_points[2 * nout] = traj[(i * traj_len + j) * 2];
            outlier_points[2 * nout + 1] = traj[(i * traj_len + j) * 2 + 1];
        }
        nout++;
    }
    if (is_outlier) std::memcpy(is_outlier, out.data(), N);
    if (columns) {
        if (best >= 0)
            std::memcpy(columns, cols.data() + (size_t)best * d, (size_t)d * 4);
        else
            for (int k = 0; k < d; k++) columns[k] = -1;
    }
    if (n_outliers) *n_outliers = nout;
    return MDX_OK;
}

// What follows the one copy that brings root[] back, O(N) on the host: clusters in creation order =
// roots in ascending order (a root precedes its members); ranks, sizes, each kept cluster's
// boundingRect.  cl: the context's [7 N] host block whose first N entries are the roots.
static int clusters_from_roots(mdx_ctx* c, const char* who, const float* points, size_t N, int32_t* cl, int min_size,
                               int32_t* labels, int* num_all, int32_t* kept, int32_t* rects, int max_kept,
                               int* num_kept)
{
    int32_t* root = cl;                           // [N] each: root, rank of a root, size, xmin, ymin, xmax, ymax
    int32_t *rank = root + N, *size = rank + N, *x0 = size + N, *y0 = x0 + N, *x1 = y0 + N, *y1 = x1 + N;
    int nall = 0;
    for (size_t i = 0; i < N; i++) {
        const int32_t r = root[i];
        if (r < 0 || (size_t)r > i || root[r] != r)
            return set_err(c, MDX_EHIP, "%s: inconsistent root %d of point %zu", who, r, i);
        const int32_t xi = cv_round(points[2 * i]), yi = cv_round(points[2 * i + 1]);   // copyTo(vector<cv::Point>)
        if ((size_t)r == i) {
            rank[i] = nall++;
            size[i] = 1;
            x0[i] = x1[i] = xi;
            y0[i] = y1[i] = yi;
        } else {
            size[r]++;
            x0[r] = std::min(x0[r], xi);
            x1[r] = std::max(x1[r], xi);
            y0[r] = std::min(y0[r], yi);
            y1[r] = std::max(y1[r], yi);
        }
        if (labels) labels[i] = rank[r];
    }
    int nk = 0;
    for (size_t i = 0; i < N; i++) {
        if ((size_t)root[i] != i || size[i] <= min_size) continue;
        if (nk < max_kept) {
            if (kept) kept[nk] = rank[i];
            if (rects) {                          // boundingRect of integer points
                rects[4 * nk] = x0[i];
                rects[4 * nk + 1] = y0[i];
                rects[4 * nk + 2] = (int32_t)((uint32_t)x1[i] - (uint32_t)x0[i] + 1u);
                rects[4 * nk + 3] = (int32_t)((uint32_t)y1[i] - (uint32_t)y0[i] + 1u);
            }
        }
        nk++;
    }
    if (num_all) *num_all = nall;
    if (num_kept) *num_kept = nk;
    return MDX_OK;
}

// clusterEuclidean (flow_clusterer.cpp:231-269) + boundingRect per kept cluster
// (optical_flow_visualizer.cpp:230-236).  The O(N^2) key minimisation runs on the device
// (mdx_cluster.hip) and leaves root[i], the first point of i's cluster; everything after it is O(N)
// and runs here, after the one copy that brings root[] back.
extern "C" int mdx_cluster_euclidean(mdx_ctx* c, const float* points, int npoints, double thr, int min_size,
                                     int32_t* labels, int* num_all, int32_t* kept, int32_t* rects, int max_kept,
                                     int* num_kept)
{
    if (!c) return MDX_EINVAL;
    if (npoints < 0 || max_kept < 0 || (npoints > 0 && !points))
        return set_err(c, MDX_EINVAL, "mdx_cluster_euclidean: bad argument");
    if (npoints > MDX_CLUSTER_MAX_POINTS)
        return set_err(c, MDX_EINVAL, "mdx_cluster_euclidean: more than %d points", MDX_CLUSTER_MAX_POINTS);
    if (std::isnan(thr)) return set_err(c, MDX_EINVAL, "mdx_cluster_euclidean: distance_threshold is NaN");
    for (size_t i = 0; i < (size_t)2 * npoints; i++)
        if (!std::isfinite(points[i]))
            return set_err(c, MDX_EINVAL, "mdx_cluster_euclidean: point %zu has a non-finite coordinate", i / 2);
    if (num_all) *num_all = 0;
    if (num_kept) *num_kept = 0;
    if (npoints == 0) return MDX_OK;
    // the threshold test sqrt((double)s) < thr as s <= s*: s* = the largest float that passes (sqrt
    // is monotonic, so every smaller s passes too); slim = bits(s*) + 1, 0 when not even s = 0 passes
    uint32_t slim = 0;
    if (thr > 0.0) {
        float f = (float)std::min(thr * thr, (double)FLT_MAX);
        while (f < FLT_MAX && std::sqrt((double)std::nextafterf(f, INFINITY)) < thr) f = std::nextafterf(f, INFINITY);
        while (f > 0.f && !(std::sqrt((double)f) < thr)) f = std::nextafterf(f, 0.f);
        if (std::sqrt((double)f) < thr) {
            std::memcpy(&slim, &f, 4);
            slim += 1;
        }
    }
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    const size_t N = (size_t)npoints;
    const int rc = ensure_all(c, {{&c->clpts, N * 8}, {&c->clbest, N * 8}, {&c->clroot, N * 4}});
    if (rc != MDX_OK) return rc;
    if (c->cl_host.size() < 7 * N) c->cl_host.resize(7 * N);
    int32_t* root = c->cl_host.data();
    hipStream_t s = c->stream;
    HIP_OR_RETURN(c, hipMemcpyAsync(c->clpts.p, points, N * 8, hipMemcpyHostToDevice, s));
    HIP_OR_RETURN(c, launch_cluster(s, c->clpts.as<float>(), npoints, slim, c->clbest.as<unsigned long long>(),
                                    c->clroot.as<int32_t>()));
    HIP_OR_RETURN(c, hipMemcpyAsync(root, c->clroot.p, N * 4, hipMemcpyDeviceToHost, s));
    HIP_OR_RETURN(c, hipStreamSynchronize(s));
    return clusters_from_roots(c, "mdx_cluster_euclidean", points, N, root, min_size, labels, num_all, kept, rects,
                               max_kept, num_kept);
}

// getClusters (flow_clusterer.cpp:178-227) + boundingRect per kept cluster (node.cpp:376-395).  The
// host does the O(n) work in front -- which vectors are active, each one's angle by libm
// (vector_cluster.cpp:131-139), the distance limit s* -- and behind (clusters_from_roots); every pair
// test and the whole first-fit resolution run on the device (mdx_vcluster.hip).
extern "C" int mdx_cluster_vectors(mdx_ctx* c, const double* vectors, int n, double thr, double athr, int min_size,
                                   int flags, int32_t* labels, int* num_active, int* num_all, int32_t* kept,
                                   int32_t* rects, int max_kept, int* num_kept)
{
    if (!c) return MDX_EINVAL;
    if (n < 0 || max_kept < 0 || (n > 0 && !vectors)) return set_err(c, MDX_EINVAL, "mdx_cluster_vectors: bad argument");
    if (n > MDX_VCLUSTER_MAX_POINTS)
        return set_err(c, MDX_EINVAL, "mdx_cluster_vectors: more than %d vectors", MDX_VCLUSTER_MAX_POINTS);
    if (std::isnan(thr) || std::isnan(athr)) return set_err(c, MDX_EINVAL, "mdx_cluster_vectors: a threshold is NaN");
    if (flags & ~MDX_VCLUSTER_ABS_INT) return set_err(c, MDX_EINVAL, "mdx_cluster_vectors: unknown flag bits 0x%x", flags);
    for (size_t i = 0; i < (size_t)4 * n; i++)
        if (!std::isfinite(vectors[i]))
            return set_err(c, MDX_EINVAL, "mdx_cluster_vectors: vector %zu has a non-finite component", i / 4);
    if (num_active) *num_active = 0;
    if (num_all) *num_all = 0;
    if (num_kept) *num_kept = 0;
    // active: fabs(dx) > 0 || fabs(dy) > 0 (:185); the others are skipped
    size_t N = 0;
    for (int i = 0; i < n; i++) N += vectors[4 * i + 2] != 0.0 || vectors[4 * i + 3] != 0.0;
    if (labels)
        for (int i = 0; i < n; i++) labels[i] = -1;
    if (N == 0) return MDX_OK;
    if (c->vc_host.size() < 3 * N) c->vc_host.resize(3 * N);
    if (c->vc_pts.size() < 2 * N) c->vc_pts.resize(2 * N);
    if (c->vc_idx.size() < 2 * N) c->vc_idx.resize(2 * N);
    if (c->cl_host.size() < 7 * N) c->cl_host.resize(7 * N);
    double *hx = c->vc_host.data(), *hy = hx + N, *ht = hy + N;
    float* pts = c->vc_pts.data();
    int32_t *idx = c->vc_idx.data(), *lab = idx + N;
    size_t k = 0;
    for (int i = 0; i < n; i++) {
        const double* v = vectors + 4 * (size_t)i;
        if (!(v[2] != 0.0 || v[3] != 0.0)) continue;
        hx[k] = v[0];
        hy[k] = v[1];
        double ang = std::atan2(v[3], v[2]);      // getAngle (:131-139)
        if (ang < 0.0) ang += 2 * M_PI;
        ht[k] = ang;
        pts[2 * k] = (float)v[0];                 // cv::Point2f(vec[0], vec[1]) (node.cpp:382)
        pts[2 * k + 1] = (float)v[1];
        idx[k++] = i;
    }
    // sqrt(s) < thr as s <= s*: s* = the largest double that passes (sqrt is monotonic); -1: none does
    double slim = -1.0;
    if (thr > 0.0) {
        double f = std::min(thr * thr, DBL_MAX);
        while (f < DBL_MAX && std::sqrt(std::nextafter(f, INFINITY)) < thr) f = std::nextafter(f, INFINITY);
        while (f > 0.0 && !(std::sqrt(f) < thr)) f = std::nextafter(f, 0.0);
        if (std::sqrt(f) < thr) slim = f;
    }
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    const int rc = ensure_all(c, {{&c->vcpts, N * 24}, {&c->vcroot, N * 4}, {&c->vcrows, vcluster_rows_bytes((int)N)},
                                  {&c->vcq, (size_t)kClB * 33 * 4}});
    if (rc != MDX_OK) return rc;
    int32_t* root = c->cl_host.data();
    hipStream_t s = c->stream;
    HIP_OR_RETURN(c, hipMemcpyAsync(c->vcpts.p, hx, N * 24, hipMemcpyHostToDevice, s));
    HIP_OR_RETURN(c, launch_vcluster(s, c->vcpts.as<double>(), (int)N, slim, athr, flags & MDX_VCLUSTER_ABS_INT,
                                     c->vcrows.as<uint32_t>(), c->vcq.as<uint32_t>(), c->vcq.as<uint32_t>() + kClB,
                                     c->vcroot.as<int32_t>()));
    HIP_OR_RETURN(c, hipMemcpyAsync(root, c->vcroot.p, N * 4, hipMemcpyDeviceToHost, s));
    HIP_OR_RETURN(c, hipStreamSynchronize(s));
    const int frc = clusters_from_roots(c, "mdx_cluster_vectors", pts, N, root, min_size, labels ? lab : nullptr,
                                        num_all, kept, rects, max_kept, num_kept);
    if (frc != MDX_OK) return frc;
    if (labels)
        for (size_t a = 0; a < N; a++) labels[idx[a]] = lab[a];
    if (num_active) *num_active = (int)N;
    return MDX_OK;
}

// showClusterContours' cv::convexHull of each requested cluster (optical_flow_visualizer.cpp:204-221,
// DESIGN.md §7j).  The host checks the input and, in the O(n) walk that clusters_from_roots' callers
// already make, groups the members by cluster and takes each cluster's column range; the column
// extremes, the chains and the ordered vertices are the device's (mdx_hull.hip), one launch.  The hulls
// come back in one copy, each in its own slice of a staging block, and are packed behind `offsets` here.
extern "C" int mdx_cluster_hulls(mdx_ctx* c, const float* points, const int32_t* labels, int n, const int32_t* ids,
                                 int k, int32_t* offsets, int32_t* xy, int max_vertices, int* num_vertices)
{
    if (!c) return MDX_EINVAL;
    if (n < 0 || k < 0 || max_vertices < 0) return set_err(c, MDX_EINVAL, "mdx_cluster_hulls: negative n, k or max_vertices");
    if (n > MDX_CLUSTER_MAX_POINTS)
        return set_err(c, MDX_EINVAL, "mdx_cluster_hulls: more than %d points", MDX_CLUSTER_MAX_POINTS);
    if (!offsets || (n > 0 && (!points || !labels)) || (k > 0 && !ids) || (max_vertices > 0 && !xy))
        return set_err(c, MDX_EINVAL, "mdx_cluster_hulls: a needed pointer is NULL");
    for (int j = 0; j < k; j++)
        if (ids[j] < 0 || (j > 0 && ids[j] <= ids[j - 1]))
            return set_err(c, MDX_EINVAL, "mdx_cluster_hulls: ids[%d] = %d: ids must be non-negative and strictly ascending", j, ids[j]);
    if (num_vertices) *num_vertices = 0;
    if (k == 0 || n == 0) {
        std::fill(offsets, offsets + k + 1, 0);
        return MDX_OK;
    }
    if (k > n) return set_err(c, MDX_EINVAL, "mdx_cluster_hulls: %d ids for %d members: an id has no member", k, n);
    for (size_t i = 0; i < (size_t)2 * n; i++)
        if (!std::isfinite(points[i]))
            return set_err(c, MDX_EINVAL, "mdx_cluster_hulls: point %zu has a non-finite coordinate", i / 2);
    const size_t N = (size_t)n, K = (size_t)k;
    try {
        if (c->hl_idx.size() < N + K) c->hl_idx.resize(N + K);
        if (c->hl_in.size() < 8 * K + 2 * N) c->hl_in.resize(8 * K + 2 * N);
        if (c->hl_out.size() < K) c->hl_out.resize(K);
    } catch (const std::bad_alloc&) {
        return set_err(c, MDX_ENOMEM, "mdx_cluster_hulls: no host memory for %d points", n);
    }
    int32_t *cidx = c->hl_idx.data(), *fill = cidx + N;
    HullCluster* rec = reinterpret_cast<HullCluster*>(c->hl_in.data());
    float* grouped = reinterpret_cast<float*>(c->hl_in.data() + 8 * K);
    std::vector<int32_t>& xmax = c->hl_out;           // [K] until the launch
    for (size_t j = 0; j < K; j++) rec[j] = HullCluster{0, 0, INT32_MAX, 0, 0, 0, {0, 0}}, xmax[j] = INT32_MIN;
    constexpr float kLim = 536870912.f;               // 2^29: cross products of differences stay in int64
    for (size_t i = 0; i < N; i++) {
        const int32_t* at = std::lower_bound(ids, ids + k, labels[i]);
        if (labels[i] < 0 || at == ids + k || *at != labels[i]) {
            cidx[i] = -1;
            continue;
        }
        const float x = points[2 * i], y = points[2 * i + 1];
        if (!(std::fabs(x) <= kLim) || !(std::fabs(y) <= kLim))   // floats there are integers: rounding changes nothing
            return set_err(c, MDX_EINVAL, "mdx_cluster_hulls: point %zu lies beyond +-2^29", i);
        const size_t j = (size_t)(at - ids);
        cidx[i] = (int32_t)j;
        const int32_t xi = cv_round(x);
        rec[j].count++;
        rec[j].xmin = std::min(rec[j].xmin, xi);
        xmax[j] = std::max(xmax[j], xi);
    }
    size_t members = 0, slots = 0;
    int max_ncols = 0;
    for (size_t j = 0; j < K; j++) {
        if (rec[j].count == 0) return set_err(c, MDX_EINVAL, "mdx_cluster_hulls: cluster %d has no member", ids[j]);
        const long long span = (long long)xmax[j] - rec[j].xmin + 1;
        if (span > MDX_HULL_MAX_SPAN)
            return set_err(c, MDX_EINVAL, "mdx_cluster_hulls: cluster %d spans %lld columns, more than %d", ids[j], span,
                           MDX_HULL_MAX_SPAN);
        rec[j].ncols = (int32_t)span;
        rec[j].start = (int32_t)members;
        rec[j].out_off = (int32_t)slots;
        rec[j].bound = (int32_t)std::min<long long>(rec[j].count, 2 * span);
        fill[j] = rec[j].start;
        members += (size_t)rec[j].count;
        slots += (size_t)rec[j].bound;
        max_ncols = std::max(max_ncols, rec[j].ncols);
    }
    for (size_t i = 0; i < N; i++)
        if (cidx[i] >= 0) std::memcpy(grouped + 2 * (size_t)fill[cidx[i]]++, points + 2 * i, 8);
    std::vector<int32_t>& out = c->hl_out;            // counts [K], then the staging block [slots][2]
    try {
        if (out.size() < K + 2 * slots) out.resize(K + 2 * slots);
    } catch (const std::bad_alloc&) {
        return set_err(c, MDX_ENOMEM, "mdx_cluster_hulls: no host memory for %zu vertices", slots);
    }
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    const size_t in_bytes = (8 * K + 2 * members) * 4, out_bytes = (K + 2 * slots) * 4;
    if (const int rc = ensure_all(c, {{&c->hlin, in_bytes}, {&c->hlout, out_bytes}}); rc != MDX_OK) return rc;
    hipStream_t s = c->stream;
    int32_t *d_in = c->hlin.as<int32_t>(), *d_out = c->hlout.as<int32_t>();
    // (mdx_enable_timing: stage 0 the upload, 3 k_hull, 4 the readback, 6 the three together)
    mark(c, 0);
    HIP_OR_RETURN(c, hipMemcpyAsync(d_in, c->hl_in.data(), in_bytes, hipMemcpyHostToDevice, s));
    for (int i = 1; i <= 3; i++) mark(c, i);
    HIP_OR_RETURN(c, launch_hull(s, k, reinterpret_cast<const HullCluster*>(d_in), reinterpret_cast<const float*>(d_in + 8 * K),
                                 max_ncols, d_out, d_out + K));
    mark(c, 4);
    HIP_OR_RETURN(c, hipMemcpyAsync(out.data(), d_out, out_bytes, hipMemcpyDeviceToHost, s));
    for (int i = 5; i <= 6; i++) mark(c, i);
    HIP_OR_RETURN(c, hipStreamSynchronize(s));
    long long total = 0;
    for (size_t j = 0; j < K; j++) {
        const int32_t nv = out[j];
        if (nv < 1 || nv > rec[j].bound) return set_err(c, MDX_EHIP, "mdx_cluster_hulls: cluster %d: %d vertices", ids[j], nv);
        offsets[j] = (int32_t)total;
        const long long room = std::min<long long>(nv, (long long)max_vertices - total);
        if (room > 0) std::memcpy(xy + 2 * total, out.data() + K + 2 * (size_t)rec[j].out_off, (size_t)room * 8);
        total += nv;
    }
    offsets[K] = (int32_t)total;
    if (num_vertices) *num_vertices = (int)total;
    return MDX_OK;
}

// findOutliers + getOutlierVectors (outlier_detector.cpp:37-186).  The host checks
// the input and computes each vector's angle by libm (:80), O(n); the magnitudes, the four order
// statistics per field and every flag are the device's (mdx_outliers.hip), one launch for the batch.
extern "C" int mdx_find_outliers(mdx_ctx* c, const double* vectors, int batch, int n, int flags, uint8_t* out_flags,
                                 double* outlier_vectors, mdx_outlier_stats* stats)
{
    if (!c) return MDX_EINVAL;
    if (batch < 0 || n < 0) return set_err(c, MDX_EINVAL, "mdx_find_outliers: negative batch or n");
    if (n > MDX_OUTLIERS_MAX_POINTS)
        return set_err(c, MDX_EINVAL, "mdx_find_outliers: more than %d vectors per field", MDX_OUTLIERS_MAX_POINTS);
    if (flags & ~MDX_OUTLIERS_INCLUDE_ZEROS) return set_err(c, MDX_EINVAL, "mdx_find_outliers: unknown flag bits 0x%x", flags);
    const size_t N = (size_t)n, total = (size_t)batch * N;
    if (total > 0 && !vectors) return set_err(c, MDX_EINVAL, "mdx_find_outliers: vectors is NULL");
    for (size_t i = 0; i < 4 * total; i++)
        if (!std::isfinite(vectors[i]))
            return set_err(c, MDX_EINVAL, "mdx_find_outliers: vector %zu has a non-finite component", i / 4);
    for (size_t i = 0; i < total; i++)      // dx*dx must not overflow: inf - inf = NaN in the reference's sort
        if (!(std::fabs(vectors[4 * i + 2]) < 1e150) || !(std::fabs(vectors[4 * i + 3]) < 1e150))
            return set_err(c, MDX_EINVAL, "mdx_find_outliers: vector %zu has a flow component >= 1e150", i);
    if (stats && batch > 0) std::memset(stats, 0, sizeof(mdx_outlier_stats) * (size_t)batch);
    if (total == 0) return MDX_OK;
    try {
        if (c->ol_host.size() < 3 * total) c->ol_host.resize(3 * total);
        if (!out_flags && outlier_vectors && c->ol_flags.size() < total) c->ol_flags.resize(total);
    } catch (const std::bad_alloc&) {
        return set_err(c, MDX_ENOMEM, "mdx_find_outliers: no host memory for %zu vectors", total);
    }
    double *hxy = c->ol_host.data(), *ha = hxy + 2 * total;
    for (int b = 0; b < batch; b++) {
        const double* v = vectors + 4 * (size_t)b * N;
        double *hx = hxy + 2 * (size_t)b * N, *hy = hx + N;
        for (size_t i = 0; i < N; i++) {
            hx[i] = v[4 * i + 2];
            hy[i] = v[4 * i + 3];
            ha[(size_t)b * N + i] = std::atan2(v[4 * i + 3], v[4 * i + 2]);   // createAngleMatrix (:80)
        }
    }
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    const size_t o_flags = (sizeof(mdx_outlier_stats) * (size_t)batch + 255) / 256 * 256;
    const int rc = ensure_all(c, {{&c->olin, total * 24}, {&c->olmag, total * 8}, {&c->olout, o_flags + total}});
    if (rc != MDX_OK) return rc;
    hipStream_t s = c->stream;
    double* d_in = c->olin.as<double>();
    char* d_out = c->olout.as<char>();
    HIP_OR_RETURN(c, hipMemcpyAsync(d_in, hxy, total * 24, hipMemcpyHostToDevice, s));
    HIP_OR_RETURN(c, launch_outliers(s, batch, n, d_in, d_in + 2 * total, c->olmag.as<double>(),
                                     flags & MDX_OUTLIERS_INCLUDE_ZEROS, reinterpret_cast<uint8_t*>(d_out + o_flags),
                                     reinterpret_cast<mdx_outlier_stats*>(d_out), c->ol_reg));
    uint8_t* fl = out_flags ? out_flags : (outlier_vectors ? c->ol_flags.data() : nullptr);
    if (fl) HIP_OR_RETURN(c, hipMemcpyAsync(fl, d_out + o_flags, total, hipMemcpyDeviceToHost, s));
    if (stats)
        HIP_OR_RETURN(c, hipMemcpyAsync(stats, d_out, sizeof(mdx_outlier_stats) * (size_t)batch, hipMemcpyDeviceToHost, s));
    HIP_OR_RETURN(c, hipStreamSynchronize(s));
    if (outlier_vectors)                    // getOutlierVectors (:55-71)
        for (size_t i = 0; i < total; i++) {
            if (fl[i])
                std::memcpy(outlier_vectors + 4 * i, vectors + 4 * i, 32);
            else
                std::memset(outlier_vectors + 4 * i, 0, 32);
        }
    return MDX_OK;
}

// getMotionContours' recipe on the pair path's mask: opening, 8-connected
// components, one record per kept component.  All of it runs on the device (mdx_regions.hip); the
// call only queues launches on the context's stream.
static int check_regions(mdx_ctx* c, const char* who, int batch, const void* mask, int w, int h, int stride,
                         size_t frame_stride, int flags, const void* regions, int max_regions, const void* mask_out)
{
    if (!mask || batch < 1 || w < 1 || h < 1) return set_err(c, MDX_EINVAL, "%s: bad mask, batch or size", who);
    if (stride < w) return set_err(c, MDX_EINVAL, "%s: stride %d < w %d", who, stride, w);
    if (frame_stride < (size_t)h * (size_t)stride) return set_err(c, MDX_EINVAL, "%s: frame_stride < h*stride", who);
    if ((long long)w * h > (1ll << 30)) return set_err(c, MDX_EINVAL, "%s: more than 2^30 pixels", who);
    if (max_regions < 0 || (max_regions > 0 && !regions))
        return set_err(c, MDX_EINVAL, "%s: max_regions %d without room for the records", who, max_regions);
    if (flags & ~MDX_REGIONS_OPEN3) return set_err(c, MDX_EINVAL, "%s: unknown flag bits 0x%x", who, flags);
    if (mask_out == mask) return set_err(c, MDX_EINVAL, "%s: mask_out is the input mask", who);
    return MDX_OK;
}

extern "C" int mdx_mask_regions_dev(mdx_ctx* c, int batch, const uint8_t* d_mask, int w, int h, int stride,
                                    size_t frame_stride, int flags, int min_area, mdx_region* d_regions,
                                    int max_regions, int32_t* d_num_all, int32_t* d_num_kept, int32_t* d_labels,
                                    uint8_t* d_mask_out)
{
    if (!c) return MDX_EINVAL;
    if (const int rc = check_regions(c, "mdx_mask_regions_dev", batch, d_mask, w, h, stride, frame_stride, flags,
                                     d_regions, max_regions, d_mask_out);
        rc != MDX_OK)
        return rc;
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    const int chunk = std::min(batch, kRegionsMaxBatch);
    if (const int rc = ensure(c, c->rgscr, regions_scratch_bytes(chunk, w, h)); rc != MDX_OK) return rc;
    hipStream_t s = c->stream;
    if (c->input_ev) {      // mdx_input_ready: one-shot
        hipEvent_t e = c->input_ev;
        c->input_ev = nullptr;
        HIP_OR_RETURN(c, hipStreamWaitEvent(s, e, 0));
    }
    const size_t N = (size_t)w * h;
    for (int b0 = 0; b0 < batch; b0 += chunk) {
        const int nb = std::min(chunk, batch - b0);
        HIP_OR_RETURN(c, launch_mask_regions(s, nb, d_mask + b0 * frame_stride, w, h, stride, frame_stride,
                                             flags & MDX_REGIONS_OPEN3, min_area,
                                             d_regions ? d_regions + (size_t)b0 * max_regions : nullptr, max_regions,
                                             d_num_all ? d_num_all + b0 : nullptr, d_num_kept ? d_num_kept + b0 : nullptr,
                                             d_labels ? d_labels + b0 * N : nullptr,
                                             d_mask_out ? d_mask_out + b0 * N : nullptr, c->rgscr.p));
    }
    return MDX_OK;
}

extern "C" int mdx_mask_regions(mdx_ctx* c, const uint8_t* mask, int w, int h, int stride, int flags, int min_area,
                                mdx_region* regions, int max_regions, int* num_all, int* num_kept, int32_t* labels,
                                uint8_t* mask_out)
{
    if (!c) return MDX_EINVAL;
    const size_t fs = (size_t)std::max(h, 0) * (size_t)std::max(stride, 0);
    if (const int rc = check_regions(c, "mdx_mask_regions", 1, mask, w, h, stride, fs, flags, regions, max_regions,
                                     mask_out);
        rc != MDX_OK)
        return rc;
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    // one output block: counts (num_all, num_kept), records, labels, mask
    const size_t N = (size_t)w * h, o_rec = 256, o_lab = o_rec + ((size_t)max_regions * sizeof(mdx_region) + 255) / 256 * 256,
                 o_msk = o_lab + (labels ? N * 4 : 0);
    // the caller's last row holds w bytes, not stride
    const size_t in_bytes = (size_t)(h - 1) * stride + w;
    if (const int rc = ensure_all(c, {{&c->rgin, fs}, {&c->rgout, o_msk + (mask_out ? N : 0)}}); rc != MDX_OK)
        return rc;
    hipStream_t s = c->stream;
    char* out = c->rgout.as<char>();
    HIP_OR_RETURN(c, hipMemcpyAsync(c->rgin.p, mask, in_bytes, hipMemcpyHostToDevice, s));
    int32_t* d_cnt = reinterpret_cast<int32_t*>(out);
    const int rc = mdx_mask_regions_dev(c, 1, c->rgin.as<uint8_t>(), w, h, stride, fs, flags, min_area,
                                        max_regions ? reinterpret_cast<mdx_region*>(out + o_rec) : nullptr, max_regions,
                                        d_cnt, d_cnt + 1, labels ? reinterpret_cast<int32_t*>(out + o_lab) : nullptr,
                                        mask_out ? reinterpret_cast<uint8_t*>(out + o_msk) : nullptr);
    if (rc != MDX_OK) return rc;
    int32_t cnt[2] = {0, 0};
    HIP_OR_RETURN(c, hipMemcpyAsync(cnt, d_cnt, 8, hipMemcpyDeviceToHost, s));
    if (labels) HIP_OR_RETURN(c, hipMemcpyAsync(labels, out + o_lab, N * 4, hipMemcpyDeviceToHost, s));
    if (mask_out) HIP_OR_RETURN(c, hipMemcpyAsync(mask_out, out + o_msk, N, hipMemcpyDeviceToHost, s));
    HIP_OR_RETURN(c, hipStreamSynchronize(s));
    const int nrec = std::min(cnt[1], max_regions);
    if (nrec > 0)
        HIP_OR_RETURN(c, hipMemcpy(regions, out + o_rec, (size_t)nrec * sizeof(mdx_region), hipMemcpyDeviceToHost));
    if (num_all) *num_all = cnt[0];
    if (num_kept) *num_kept = cnt[1];
    return MDX_OK;
}

// The convex hull of each region record's pixels: what the node takes from a blob next to
// its boundingRect (optical_flow_visualizer.cpp:204-240).  All of it runs on the device (mdx_hull.hip);
// the call only queues three launches on the context's stream.
static int check_region_hulls(mdx_ctx* c, const char* who, int w, const void* offsets, const void* xy, int max_vertices)
{
    if (w > MDX_HULL_MAX_SPAN) return set_err(c, MDX_EINVAL, "%s: w %d is more than %d columns", who, w, MDX_HULL_MAX_SPAN);
    if (max_vertices < 0) return set_err(c, MDX_EINVAL, "%s: negative max_vertices", who);
    if (!offsets || (max_vertices > 0 && !xy)) return set_err(c, MDX_EINVAL, "%s: a needed pointer is NULL", who);
    return MDX_OK;
}

extern "C" int mdx_region_hulls_dev(mdx_ctx* c, int batch, const int32_t* d_labels, int w, int h,
                                    const mdx_region* d_regions, int max_regions, const int32_t* d_num_kept,
                                    int32_t* d_offsets, int32_t* d_xy, int max_vertices, int32_t* d_num_vertices)
{
    if (!c) return MDX_EINVAL;
    const char* who = "mdx_region_hulls_dev";
    if (batch < 1 || w < 1 || h < 1) return set_err(c, MDX_EINVAL, "%s: bad batch or size", who);
    if ((long long)w * h > (1ll << 30)) return set_err(c, MDX_EINVAL, "%s: more than 2^30 pixels", who);
    if (max_regions < 0) return set_err(c, MDX_EINVAL, "%s: negative max_regions", who);
    if (const int rc = check_region_hulls(c, who, w, d_offsets, d_xy, max_vertices); rc != MDX_OK) return rc;
    if (!d_labels || (max_regions > 0 && (!d_regions || !d_num_kept)))
        return set_err(c, MDX_EINVAL, "%s: a needed pointer is NULL", who);
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    const int chunk = std::min(batch, kRegionsMaxBatch);
    if (const int rc = ensure(c, c->rhscr, region_hulls_scratch_bytes(chunk, w, h, max_regions)); rc != MDX_OK) return rc;
    hipStream_t s = c->stream;
    if (c->input_ev) {      // mdx_input_ready: one-shot
        hipEvent_t e = c->input_ev;
        c->input_ev = nullptr;
        HIP_OR_RETURN(c, hipStreamWaitEvent(s, e, 0));
    }
    const size_t N = (size_t)w * h;
    // (mdx_enable_timing: stage 2 k_region_hull_slices, 3 k_region_hull, 4 k_region_hull_pack, 6 the three together)
    for (int i = 0; i <= 2; i++) mark(c, i);
    hipEvent_t* ev = c->timing && c->cur >= 0 ? c->ev.data() + c->cur * 7 : nullptr;
    for (int b0 = 0; b0 < batch; b0 += chunk) {
        const int nb = std::min(chunk, batch - b0);
        HIP_OR_RETURN(c, launch_region_hulls(s, nb, d_labels + b0 * N, w, h,
                                             d_regions ? d_regions + (size_t)b0 * max_regions : nullptr, max_regions,
                                             d_num_kept ? d_num_kept + b0 : nullptr,
                                             d_offsets + (size_t)b0 * ((size_t)max_regions + 1),
                                             d_xy ? d_xy + (size_t)b0 * max_vertices * 2 : nullptr, max_vertices,
                                             d_num_vertices ? d_num_vertices + b0 : nullptr, c->rhscr.p,
                                             ev ? ev[3] : nullptr, ev ? ev[4] : nullptr));
    }
    if (max_regions == 0)
        for (int i = 3; i <= 4; i++) mark(c, i);     // no record, no k_region_hull: its stage is empty
    for (int i = 5; i <= 6; i++) mark(c, i);
    return MDX_OK;
}

extern "C" int mdx_mask_region_hulls(mdx_ctx* c, const uint8_t* mask, int w, int h, int stride, int flags, int min_area,
                                     mdx_region* regions, int max_regions, int* num_all, int* num_kept,
                                     int32_t* offsets, int32_t* xy, int max_vertices, int* num_vertices)
{
    if (!c) return MDX_EINVAL;
    const char* who = "mdx_mask_region_hulls";
    const size_t fs = (size_t)std::max(h, 0) * (size_t)std::max(stride, 0);
    if (const int rc = check_regions(c, who, 1, mask, w, h, stride, fs, flags, regions, max_regions, nullptr); rc != MDX_OK)
        return rc;
    if (const int rc = check_region_hulls(c, who, w, offsets, xy, max_vertices); rc != MDX_OK) return rc;
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    // one output block: counts (num_all, num_kept, num_vertices), records, offsets, labels, xy; the labels
    // stay on the device
    const size_t N = (size_t)w * h, M = (size_t)max_regions, o_rec = 256,
                 o_off = o_rec + (M * sizeof(mdx_region) + 255) / 256 * 256, o_lab = o_off + ((M + 1) * 4 + 255) / 256 * 256,
                 o_xy = o_lab + (N * 4 + 255) / 256 * 256;
    const size_t in_bytes = (size_t)(h - 1) * stride + w;     // the caller's last row holds w bytes, not stride
    if (const int rc = ensure_all(c, {{&c->rgin, fs}, {&c->rhout, o_xy + (size_t)max_vertices * 8}}); rc != MDX_OK)
        return rc;
    hipStream_t s = c->stream;
    char* out = c->rhout.as<char>();
    HIP_OR_RETURN(c, hipMemcpyAsync(c->rgin.p, mask, in_bytes, hipMemcpyHostToDevice, s));
    int32_t* d_cnt = reinterpret_cast<int32_t*>(out);
    mdx_region* d_rec = max_regions ? reinterpret_cast<mdx_region*>(out + o_rec) : nullptr;
    int32_t* d_lab = reinterpret_cast<int32_t*>(out + o_lab);
    if (const int rc = mdx_mask_regions_dev(c, 1, c->rgin.as<uint8_t>(), w, h, stride, fs, flags, min_area, d_rec,
                                            max_regions, d_cnt, d_cnt + 1, d_lab, nullptr);
        rc != MDX_OK)
        return rc;
    if (const int rc = mdx_region_hulls_dev(c, 1, d_lab, w, h, d_rec, max_regions, d_cnt + 1,
                                            reinterpret_cast<int32_t*>(out + o_off),
                                            max_vertices ? reinterpret_cast<int32_t*>(out + o_xy) : nullptr, max_vertices,
                                            d_cnt + 2);
        rc != MDX_OK)
        return rc;
    int32_t cnt[3] = {0, 0, 0};
    HIP_OR_RETURN(c, hipMemcpyAsync(cnt, d_cnt, 12, hipMemcpyDeviceToHost, s));
    HIP_OR_RETURN(c, hipMemcpyAsync(offsets, out + o_off, (M + 1) * 4, hipMemcpyDeviceToHost, s));
    HIP_OR_RETURN(c, hipStreamSynchronize(s));
    const int nrec = std::min(cnt[1], max_regions);
    if (nrec > 0)
        HIP_OR_RETURN(c, hipMemcpy(regions, out + o_rec, (size_t)nrec * sizeof(mdx_region), hipMemcpyDeviceToHost));
    const int nxy = std::min(cnt[2], max_vertices);           // only the vertices that exist come back
    if (nxy > 0) HIP_OR_RETURN(c, hipMemcpy(xy, out + o_xy, (size_t)nxy * 8, hipMemcpyDeviceToHost));
    if (num_all) *num_all = cnt[0];
    if (num_kept) *num_kept = cnt[1];
    if (num_vertices) *num_vertices = cnt[2];
    return MDX_OK;
}

// Which blob lies inside which: the parent of each region record and the records that
// findContours' RETR_EXTERNAL keeps.  All of it runs on the device (mdx_regions.hip, the k_tree_* kernels);
// the call only queues five launches on the context's stream.
extern "C" int mdx_region_parents_dev(mdx_ctx* c, int batch, const int32_t* d_labels, int w, int h,
                                      const mdx_region* d_regions, int max_regions, const int32_t* d_num_kept,
                                      int32_t* d_parent, mdx_region* d_external, int32_t* d_num_external)
{
    if (!c) return MDX_EINVAL;
    const char* who = "mdx_region_parents_dev";
    if (batch < 1 || w < 1 || h < 1) return set_err(c, MDX_EINVAL, "%s: bad batch or size", who);
    if ((long long)w * h > (1ll << 30)) return set_err(c, MDX_EINVAL, "%s: more than 2^30 pixels", who);
    if (max_regions < 0) return set_err(c, MDX_EINVAL, "%s: negative max_regions", who);
    if (!d_labels || (max_regions > 0 && (!d_regions || !d_num_kept)))
        return set_err(c, MDX_EINVAL, "%s: a needed pointer is NULL", who);
    if (d_external && d_regions && max_regions > 0) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(d_regions), b = reinterpret_cast<uintptr_t>(d_external);
        const size_t bytes = (size_t)batch * max_regions * sizeof(mdx_region);
        if (a < b + bytes && b < a + bytes) return set_err(c, MDX_EINVAL, "%s: d_external overlaps d_regions", who);
    }
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    const int chunk = std::min(batch, kRegionsMaxBatch);
    if (const int rc = ensure(c, c->rtscr, region_parents_scratch_bytes(chunk, w, h)); rc != MDX_OK) return rc;
    hipStream_t s = c->stream;
    if (c->input_ev) {      // mdx_input_ready: one-shot
        hipEvent_t e = c->input_ev;
        c->input_ev = nullptr;
        HIP_OR_RETURN(c, hipStreamWaitEvent(s, e, 0));
    }
    const size_t N = (size_t)w * h, M = (size_t)max_regions;
    // (mdx_enable_timing: stages 0 .. 4 the tile, merge, roots, flatten and resolve kernels, 6 the five together)
    mark(c, 0);
    hipEvent_t* ev = c->timing && c->cur >= 0 ? c->ev.data() + c->cur * 7 : nullptr;
    for (int b0 = 0; b0 < batch; b0 += chunk) {
        const int nb = std::min(chunk, batch - b0);
        HIP_OR_RETURN(c, launch_region_parents(s, nb, d_labels + b0 * N, w, h, d_regions ? d_regions + b0 * M : nullptr,
                                               max_regions, d_num_kept ? d_num_kept + b0 : nullptr,
                                               d_parent ? d_parent + b0 * M : nullptr,
                                               d_external ? d_external + b0 * M : nullptr,
                                               d_num_external ? d_num_external + b0 : nullptr, c->rtscr.p, ev));
    }
    mark(c, 6);
    return MDX_OK;
}

extern "C" int mdx_mask_regions_tree(mdx_ctx* c, const uint8_t* mask, int w, int h, int stride, int flags, int min_area,
                                     mdx_region* regions, int max_regions, int* num_all, int* num_kept, int32_t* parent,
                                     int32_t* external_index, int* num_external, int32_t* offsets, int32_t* xy,
                                     int max_vertices, int* num_vertices)
{
    if (!c) return MDX_EINVAL;
    const char* who = "mdx_mask_regions_tree";
    const size_t fs = (size_t)std::max(h, 0) * (size_t)std::max(stride, 0);
    if (const int rc = check_regions(c, who, 1, mask, w, h, stride, fs, flags, regions, max_regions, nullptr); rc != MDX_OK)
        return rc;
    if (offsets) {
        if (const int rc = check_region_hulls(c, who, w, offsets, xy, max_vertices); rc != MDX_OK) return rc;
    } else {
        max_vertices = 0;
    }
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    // one output block: counts (num_all, num_kept, num_external, num_vertices), records, external records,
    // parents, offsets, labels, xy; the labels stay on the device
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t N = (size_t)w * h, M = (size_t)max_regions, o_rec = 256, o_ext = o_rec + up(M * sizeof(mdx_region)),
                 o_par = o_ext + up(M * sizeof(mdx_region)), o_off = o_par + up(M * 4), o_lab = o_off + up((M + 1) * 4),
                 o_xy = o_lab + up(N * 4);
    const size_t in_bytes = (size_t)(h - 1) * stride + w;     // the caller's last row holds w bytes, not stride
    if (const int rc = ensure_all(c, {{&c->rgin, fs}, {&c->rtout, o_xy + (size_t)max_vertices * 8}}); rc != MDX_OK)
        return rc;
    hipStream_t s = c->stream;
    char* out = c->rtout.as<char>();
    HIP_OR_RETURN(c, hipMemcpyAsync(c->rgin.p, mask, in_bytes, hipMemcpyHostToDevice, s));
    int32_t* d_cnt = reinterpret_cast<int32_t*>(out);
    mdx_region* d_rec = max_regions ? reinterpret_cast<mdx_region*>(out + o_rec) : nullptr;
    mdx_region* d_ext = max_regions ? reinterpret_cast<mdx_region*>(out + o_ext) : nullptr;
    int32_t* d_lab = reinterpret_cast<int32_t*>(out + o_lab);
    if (const int rc = mdx_mask_regions_dev(c, 1, c->rgin.as<uint8_t>(), w, h, stride, fs, flags, min_area, d_rec,
                                            max_regions, d_cnt, d_cnt + 1, d_lab, nullptr);
        rc != MDX_OK)
        return rc;
    if (const int rc = mdx_region_parents_dev(c, 1, d_lab, w, h, d_rec, max_regions, d_cnt + 1,
                                              reinterpret_cast<int32_t*>(out + o_par), d_ext, d_cnt + 2);
        rc != MDX_OK)
        return rc;
    if (offsets)
        if (const int rc = mdx_region_hulls_dev(c, 1, d_lab, w, h, d_ext, max_regions, d_cnt + 2,
                                                reinterpret_cast<int32_t*>(out + o_off),
                                                max_vertices ? reinterpret_cast<int32_t*>(out + o_xy) : nullptr,
                                                max_vertices, d_cnt + 3);
            rc != MDX_OK)
            return rc;
    int32_t cnt[4] = {0, 0, 0, 0};
    HIP_OR_RETURN(c, hipMemcpyAsync(cnt, d_cnt, offsets ? 16 : 12, hipMemcpyDeviceToHost, s));
    if (offsets) HIP_OR_RETURN(c, hipMemcpyAsync(offsets, out + o_off, (M + 1) * 4, hipMemcpyDeviceToHost, s));
    HIP_OR_RETURN(c, hipStreamSynchronize(s));
    const int nrec = std::min(cnt[1], max_regions);
    if (nrec > 0) {
        HIP_OR_RETURN(c, hipMemcpy(regions, out + o_rec, (size_t)nrec * sizeof(mdx_region), hipMemcpyDeviceToHost));
        std::vector<int32_t> par;     // external_index follows from the parents
        if (!parent) par.resize((size_t)nrec);
        int32_t* p = parent ? parent : par.data();
        HIP_OR_RETURN(c, hipMemcpy(p, out + o_par, (size_t)nrec * 4, hipMemcpyDeviceToHost));
        if (external_index)
            for (int j = 0, k = 0; j < nrec; j++)
                if (p[j] == MDX_REGION_NO_PARENT) external_index[k++] = j;
    }
    const int nxy = std::min(cnt[3], max_vertices);           // only the vertices that exist come back
    if (nxy > 0) HIP_OR_RETURN(c, hipMemcpy(xy, out + o_xy, (size_t)nxy * 8, hipMemcpyDeviceToHost));
    if (num_all) *num_all = cnt[0];
    if (num_kept) *num_kept = cnt[1];
    if (num_external) *num_external = cnt[2];
    if (offsets && num_vertices) *num_vertices = cnt[3];
    return MDX_OK;
}

// The outer border polyline of each region record: what findContours itself returns for a
// blob.  All of it runs on the device (mdx_outline.hip); the call only queues launches on the context's
// stream, their number fixed by (w, h).
static int check_region_outlines(mdx_ctx* c, const char* who, int w, int h, const void* offsets, const void* xy,
                                 int max_points)
{
    if ((long long)w * h > (1ll << 28)) return set_err(c, MDX_EINVAL, "%s: more than 2^28 pixels", who);
    if (max_points < 0) return set_err(c, MDX_EINVAL, "%s: negative max_points", who);
    if (!offsets || (max_points > 0 && !xy)) return set_err(c, MDX_EINVAL, "%s: a needed pointer is NULL", who);
    return MDX_OK;
}

extern "C" int mdx_region_outlines_dev(mdx_ctx* c, int batch, const int32_t* d_labels, int w, int h,
                                       const mdx_region* d_regions, int max_regions, const int32_t* d_num_kept,
                                       int32_t* d_offsets, int32_t* d_xy, int max_points, int32_t* d_num_points)
{
    if (!c) return MDX_EINVAL;
    const char* who = "mdx_region_outlines_dev";
    if (batch < 1 || w < 1 || h < 1) return set_err(c, MDX_EINVAL, "%s: bad batch or size", who);
    if (max_regions < 0) return set_err(c, MDX_EINVAL, "%s: negative max_regions", who);
    if (const int rc = check_region_outlines(c, who, w, h, d_offsets, d_xy, max_points); rc != MDX_OK) return rc;
    if (!d_labels || (max_regions > 0 && (!d_regions || !d_num_kept)))
        return set_err(c, MDX_EINVAL, "%s: a needed pointer is NULL", who);
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    const int chunk = std::min(batch, kRegionsMaxBatch);
    if (max_regions > 0)                             // without records the one launch touches no scratch
        if (const int rc = ensure(c, c->roscr, region_outlines_scratch_bytes(chunk, w, h, max_regions)); rc != MDX_OK)
            return rc;
    hipStream_t s = c->stream;
    if (c->input_ev) {      // mdx_input_ready: one-shot
        hipEvent_t e = c->input_ev;
        c->input_ev = nullptr;
        HIP_OR_RETURN(c, hipStreamWaitEvent(s, e, 0));
    }
    const size_t N = (size_t)w * h, M = (size_t)max_regions;
    // (mdx_enable_timing: stage 0 the set-up kernels, 1 the rounds, 2 the offsets, 3 the scatter, 6 all of them)
    mark(c, 0);
    hipEvent_t* ev = c->timing && c->cur >= 0 ? c->ev.data() + c->cur * 7 : nullptr;
    for (int b0 = 0; b0 < batch; b0 += chunk) {
        const int nb = std::min(chunk, batch - b0);
        HIP_OR_RETURN(c, launch_region_outlines(s, nb, d_labels + b0 * N, w, h, d_regions ? d_regions + b0 * M : nullptr,
                                                max_regions, d_num_kept ? d_num_kept + b0 : nullptr,
                                                d_offsets + b0 * (M + 1),
                                                d_xy ? d_xy + (size_t)b0 * max_points * 2 : nullptr, max_points,
                                                d_num_points ? d_num_points + b0 : nullptr, c->roscr.p, ev));
    }
    for (int i = 5; i <= 6; i++) mark(c, i);
    return MDX_OK;
}

extern "C" int mdx_mask_region_outlines(mdx_ctx* c, const uint8_t* mask, int w, int h, int stride, int flags, int min_area,
                                        mdx_region* regions, int max_regions, int* num_all, int* num_kept,
                                        int32_t* parent, int32_t* external_index, int* num_external, int32_t* offsets,
                                        int32_t* xy, int max_points, int* num_points)
{
    if (!c) return MDX_EINVAL;
    const char* who = "mdx_mask_region_outlines";
    const size_t fs = (size_t)std::max(h, 0) * (size_t)std::max(stride, 0);
    if (const int rc = check_regions(c, who, 1, mask, w, h, stride, fs, flags, regions, max_regions, nullptr); rc != MDX_OK)
        return rc;
    if (const int rc = check_region_outlines(c, who, w, h, offsets, xy, max_points); rc != MDX_OK) return rc;
    const bool tree = parent || external_index || num_external;    // outline the external records only
    HIP_OR_RETURN(c, hipSetDevice(c->device));
    // one output block: counts (num_all, num_kept, num_external, num_points), records, external records,
    // parents, offsets, labels, xy; the labels stay on the device
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t N = (size_t)w * h, M = (size_t)max_regions, o_rec = 256, o_ext = o_rec + up(M * sizeof(mdx_region)),
                 o_par = o_ext + up(M * sizeof(mdx_region)), o_off = o_par + up(M * 4), o_lab = o_off + up((M + 1) * 4),
                 o_xy = o_lab + up(N * 4);
    const size_t in_bytes = (size_t)(h - 1) * stride + w;     // the caller's last row holds w bytes, not stride
    if (const int rc = ensure_all(c, {{&c->rgin, fs}, {&c->roout, o_xy + (size_t)max_points * 8}}); rc != MDX_OK)
        return rc;
    hipStream_t s = c->stream;
    char* out = c->roout.as<char>();
    HIP_OR_RETURN(c, hipMemcpyAsync(c->rgin.p, mask, in_bytes, hipMemcpyHostToDevice, s));
    int32_t* d_cnt = reinterpret_cast<int32_t*>(out);
    mdx_region* d_rec = max_regions ? reinterpret_cast<mdx_region*>(out + o_rec) : nullptr;
    mdx_region* d_ext = max_regions ? reinterpret_cast<mdx_region*>(out + o_ext) : nullptr;
    int32_t* d_lab = reinterpret_cast<int32_t*>(out + o_lab);
    if (const int rc = mdx_mask_regions_dev(c, 1, c->rgin.as<uint8_t>(), w, h, stride, fs, flags, min_area, d_rec,
                                            max_regions, d_cnt, d_cnt + 1, d_lab, nullptr);
        rc != MDX_OK)
        return rc;
    if (tree)
        if (const int rc = mdx_region_parents_dev(c, 1, d_lab, w, h, d_rec, max_regions, d_cnt + 1,
                                                  reinterpret_cast<int32_t*>(out + o_par), d_ext, d_cnt + 2);
            rc != MDX_OK)
            return rc;
    if (const int rc = mdx_region_outlines_dev(c, 1, d_lab, w, h, tree ? d_ext : d_rec, max_regions,
                                               tree ? d_cnt + 2 : d_cnt + 1, reinterpret_cast<int32_t*>(out + o_off),
                                               max_points ? reinterpret_cast<int32_t*>(out + o_xy) : nullptr, max_points,
                                               d_cnt + 3);
        rc != MDX_OK)
        return rc;
    int32_t cnt[4] = {0, 0, 0, 0};
    HIP_OR_RETURN(c, hipMemcpyAsync(cnt, d_cnt, 16, hipMemcpyDeviceToHost, s));
    HIP_OR_RETURN(c, hipMemcpyAsync(offsets, out + o_off, (M + 1) * 4, hipMemcpyDeviceToHost, s));
    HIP_OR_RETURN(c, hipStreamSynchronize(s));
    const int nrec = std::min(cnt[1], max_regions);
    if (nrec > 0) {
        HIP_OR_RETURN(c, hipMemcpy(regions, out + o_rec, (size_t)nrec * sizeof(mdx_region), hipMemcpyDeviceToHost));
        if (tree) {
            std::vector<int32_t> par;     // external_index follows from the parents
            if (!parent) par.resize((size_t)nrec);
            int32_t* p = parent ? parent : par.data();
            HIP_OR_RETURN(c, hipMemcpy(p, out + o_par, (size_t)nrec * 4, hipMemcpyDeviceToHost));
            if (external_index)
                for (int j = 0, k = 0; j < nrec; j++)
                    if (p[j] == MDX_REGION_NO_PARENT) external_index[k++] = j;
        }
    }
    const int nxy = std::min(cnt[3], max_points);             // only the points that exist come back
    if (nxy > 0) HIP_OR_RETURN(c, hipMemcpy(xy, out + o_xy, (size_t)nxy * 8, hipMemcpyDeviceToHost));
    if (num_all) *num_all = cnt[0];
    if (num_kept) *num_kept = cnt[1];
    if (tree && num_external) *num_external = cnt[2];
    if (num_points) *num_points = cnt[3];
    return MDX_OK;
}
