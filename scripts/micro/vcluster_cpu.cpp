// vcluster_cpu -- yardstick for scripts/vcluster_timing.py: the loop shape of
// FlowClusterer::getClusters (reference common/src/flow_clusterer.cpp:178-227) as one host thread runs
// it: per vector, the clusters in creation order; per cluster the smallest distance over its members
// and, only if that passes, the smallest angular distance over its members, each from three atan2, a
// sin and a cos (vector_cluster.cpp:25-50, :118-139); the first cluster that passes both takes the
// vector.  A program of this project's own, written from the description in DESIGN.md §7g; it is not
// the code under test.
//
//   g++ -O2 -ffp-contract=off -o vcluster_cpu vcluster_cpu.cpp
//   vcluster_cpu <vectors.f64> <n> <distance_threshold> <angular_threshold> <abs_int> <repeats>
// vectors.f64: n x (x, y, dx, dy) float64, in visiting order.
// Prints "n <n> active <active> clusters <all> kept <kept> ms <median>".
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

struct Vec4 { double v[4]; };

static double angle_of(const Vec4& a)
{
    double ang = std::atan2(a.v[3], a.v[2]);
    if (ang < 0.0) ang += 2 * M_PI;
    return ang;
}

static double angular_distance(const Vec4& a, const Vec4& b)
{
    const double a1 = angle_of(a), a2 = angle_of(b);
    return std::atan2(std::sin(a1 - a2), std::cos(a1 - a2));
}

static int cluster(const std::vector<Vec4>& vecs, double thr, double athr, bool abs_int, int* active, int* kept)
{
    std::vector<std::vector<Vec4>> clusters;
    *active = 0;
    for (const Vec4& p : vecs) {
        if (!(std::fabs(p.v[2]) > 0.0 || std::fabs(p.v[3]) > 0.0)) continue;
        ++*active;
        bool added = false;
        for (auto& c : clusters) {
            double dmin = std::numeric_limits<double>::max();
            for (const Vec4& q : c) {
                const double dx = p.v[0] - q.v[0], dy = p.v[1] - q.v[1];
                dmin = std::min(dmin, std::sqrt(dx * dx + dy * dy));
            }
            if (!(dmin < thr)) continue;
            double amin = std::numeric_limits<double>::max();
            for (const Vec4& q : c) {
                double a = angular_distance(p, q);
                a = abs_int ? (double)std::abs((int)a) : std::fabs(a);
                amin = std::min(amin, a);
            }
            if (amin < athr) {
                c.push_back(p);
                added = true;
                break;
            }
        }
        if (!added) clusters.emplace_back(1, p);
    }
    *kept = 0;
    for (const auto& c : clusters)
        if (c.size() > 5) ++*kept;
    return (int)clusters.size();
}

int main(int argc, char** argv)
{
    if (argc < 7) {
        std::fprintf(stderr, "usage: %s <vectors.f64> <n> <distance_threshold> <angular_threshold> <abs_int> <repeats>\n",
                     argv[0]);
        return 2;
    }
    const int n = std::atoi(argv[2]), reps = std::max(1, std::atoi(argv[6]));
    const double thr = std::atof(argv[3]), athr = std::atof(argv[4]);
    const bool abs_int = std::atoi(argv[5]) != 0;
    std::vector<Vec4> vecs(n);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(vecs.data(), sizeof(Vec4), n, f) != (size_t)n) {
        std::fprintf(stderr, "cannot read %d vectors from %s\n", n, argv[1]);
        return 1;
    }
    std::fclose(f);
    std::vector<double> ms;
    int all = 0, active = 0, kept = 0;
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        all = cluster(vecs, thr, athr, abs_int, &active, &kept);
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    std::printf("n %d active %d clusters %d kept %d ms %.4f\n", n, active, all, kept, ms[ms.size() / 2]);
    return 0;
}
