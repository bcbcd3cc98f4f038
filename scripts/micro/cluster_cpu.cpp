// cluster_cpu -- yardstick for scripts/cluster_timing.py: the literal greedy loop of
// FlowClusterer::clusterEuclidean (reference common/src/flow_clusterer.cpp:231-269 with
// PointCluster::getClosestDistance, point_cluster.cpp:63-66) as one host thread runs it.  A program
// of this project's own, written from the description in DESIGN.md §7e; it is not the code under test.
//
//   g++ -O2 -ffp-contract=off -o cluster_cpu cluster_cpu.cpp
//   cluster_cpu <points.f32> <npoints> <threshold> <repeats>
// points.f32: npoints x (x, y) float32.  Prints "n <npoints> clusters <all> kept <kept> ms <median>".
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

struct Pt { float x, y; };

static int cluster(const std::vector<Pt>& pts, double thr, int* kept)
{
    std::vector<std::vector<Pt>> clusters;
    for (size_t i = 0; i < pts.size(); i++) {
        const Pt p = pts[i];
        double closest = std::numeric_limits<double>::max();
        int index = -1;
        for (size_t k = 0; k < clusters.size(); k++) {
            double dk = std::numeric_limits<double>::max();
            for (const Pt& q : clusters[k]) {
                const float dx = p.x - q.x, dy = p.y - q.y;
                const double d = std::sqrt((double)(dx * dx + dy * dy));
                if (d < dk) dk = d;
            }
            if (dk < closest) {
                closest = dk;
                index = (int)k;
            }
        }
        if (index != -1 && closest < thr) {
            clusters[index].push_back(p);
        } else {
            clusters.emplace_back(1, p);
        }
    }
    *kept = 0;
    for (const auto& c : clusters)
        if (c.size() > 5) ++*kept;
    return (int)clusters.size();
}

int main(int argc, char** argv)
{
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s <points.f32> <npoints> <threshold> <repeats>\n", argv[0]);
        return 2;
    }
    const int n = std::atoi(argv[2]), reps = std::max(1, std::atoi(argv[4]));
    const double thr = std::atof(argv[3]);
    std::vector<Pt> pts(n);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(pts.data(), sizeof(Pt), n, f) != (size_t)n) {
        std::fprintf(stderr, "cannot read %d points from %s\n", n, argv[1]);
        return 1;
    }
    std::fclose(f);
    std::vector<double> ms;
    int all = 0, kept = 0;
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        all = cluster(pts, thr, &kept);
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    std::printf("n %d clusters %d kept %d ms %.4f\n", n, all, kept, ms[ms.size() / 2]);
    return 0;
}
