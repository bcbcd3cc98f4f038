// outliers_cpu -- yardstick for scripts/outliers_timing.py: the loop shape of
// OutlierDetector::findOutliers (reference common/src/outlier_detector.cpp:37-186) as one host thread
// runs it: per field an atan2 and a sqrt per vector, then per channel the selected values gathered into
// a vector, a std::sort for the median, the absolute deviations, a second std::sort for the MAD, and
// the z-score test per selected vector.  A program of this project's own, written from the description
// in DESIGN.md §7h; it is not the code under test.
//
//   g++ -O2 -ffp-contract=off -o outliers_cpu outliers_cpu.cpp
//   outliers_cpu <vectors.f64> <batch> <n> <include_zeros> <repeats>
// vectors.f64: batch x n x (x, y, dx, dy) float64.
// Prints "batch <b> n <n> selected <sum> angle <sum> magnitude <sum> outliers <sum> ms <median>
// atan2_ms <median of the atan2 pass alone>".
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

static double median_of(std::vector<double> v)      // by value, as getMedian takes it
{
    std::sort(v.begin(), v.end());
    return v.size() % 2 == 0 ? (v[v.size() / 2 - 1] + v[v.size() / 2]) / 2.0 : v[(v.size() - 1) / 2];
}

static void mask(const double* vec, const std::vector<double>& values, int n, bool zeros, std::vector<unsigned char>& flags,
                 unsigned char bit, long* selected, long* flagged)
{
    std::vector<double> vals;
    for (int i = 0; i < n; i++)
        if (zeros || std::fabs(vec[4 * i + 2]) > 0.0 || std::fabs(vec[4 * i + 3]) > 0.0) vals.push_back(values[i]);
    *selected = (long)vals.size();
    if (vals.empty()) return;
    const double median = median_of(vals);
    std::vector<double> diff;
    for (double v : vals) diff.push_back(std::fabs(v - median));
    const double mad = median_of(diff);
    size_t index = 0;
    for (int i = 0; i < n; i++) {
        if (!(zeros || std::fabs(vec[4 * i + 2]) > 0.0 || std::fabs(vec[4 * i + 3]) > 0.0)) continue;
        const double z = 0.6745 * diff[index++] / mad;
        if (std::fabs(z) > 3.5) {
            flags[i] |= bit;
            ++*flagged;
        }
    }
}

int main(int argc, char** argv)
{
    if (argc < 6) {
        std::fprintf(stderr, "usage: %s <vectors.f64> <batch> <n> <include_zeros> <repeats>\n", argv[0]);
        return 2;
    }
    const int batch = std::atoi(argv[2]), n = std::atoi(argv[3]), reps = std::max(1, std::atoi(argv[5]));
    const bool zeros = std::atoi(argv[4]) != 0;
    std::vector<double> vec((size_t)batch * n * 4);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(vec.data(), 32, (size_t)batch * n, f) != (size_t)batch * n) {
        std::fprintf(stderr, "cannot read %d x %d vectors from %s\n", batch, n, argv[1]);
        return 1;
    }
    std::fclose(f);
    std::vector<double> ms, ams;
    long sel = 0, fa = 0, fm = 0, out = 0;
    for (int r = 0; r < reps; r++) {
        sel = fa = fm = out = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int b = 0; b < batch; b++) {
            const double* v = vec.data() + (size_t)b * n * 4;
            std::vector<double> ang(n), mag(n);
            std::vector<unsigned char> flags(n, 0);
            for (int i = 0; i < n; i++) ang[i] = std::atan2(v[4 * i + 3], v[4 * i + 2]);
            for (int i = 0; i < n; i++) mag[i] = std::sqrt(v[4 * i + 3] * v[4 * i + 3] + v[4 * i + 2] * v[4 * i + 2]);
            long s = 0;
            mask(v, ang, n, zeros, flags, 1, &s, &fa);
            mask(v, mag, n, zeros, flags, 2, &s, &fm);
            sel += s;
            for (int i = 0; i < n; i++) out += flags[i] != 0;
        }
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        const auto t1 = std::chrono::steady_clock::now();
        double sink = 0;
        for (size_t i = 0; i < (size_t)batch * n; i++) sink += std::atan2(vec[4 * i + 3], vec[4 * i + 2]);
        ams.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
        if (sink == 12345.678) std::printf(" ");      // keeps the pass
    }
    std::sort(ms.begin(), ms.end());
    std::sort(ams.begin(), ams.end());
    std::printf("batch %d n %d selected %ld angle %ld magnitude %ld outliers %ld ms %.4f atan2_ms %.4f\n", batch, n, sel, fa,
                fm, out, ms[ms.size() / 2], ams[ams.size() / 2]);
    return 0;
}
