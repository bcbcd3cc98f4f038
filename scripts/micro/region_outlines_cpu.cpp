// region_outlines_cpu.cpp -- the host yardstick of scripts/region_outlines_timing.py: what a caller of
// mdx_mask_regions_dev does without mdx_region_outlines_dev.  From the label images (copied to the host) it
// takes each component's first pixel and area, and traces the outer border of the first max_regions
// components of at least min_area pixels with include/mdx.h's sequential rule, on one thread.
//   region_outlines_cpu <labels.i32> <w> <h> <batch> <min_area> <max_regions> <reps>
// prints: points <sum over the batch> states <sum over the batch of the device's states: per pixel with a
// non-member 4-neighbour, its same-label neighbours> ms <median of reps, whole batch, the states not timed>
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

static const int DX[8] = {1, 1, 0, -1, -1, -1, 0, 1}, DY[8] = {0, -1, -1, -1, 0, 1, 1, 1};

int main(int argc, char** argv)
{
    if (argc < 8) return 2;
    const int w = atoi(argv[2]), h = atoi(argv[3]), B = atoi(argv[4]), min_area = atoi(argv[5]), cap = atoi(argv[6]),
              reps = atoi(argv[7]);
    const size_t N = (size_t)w * h;
    std::vector<int32_t> lab(N * B);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(lab.data(), 4, lab.size(), f) != lab.size()) return 3;
    fclose(f);
    std::vector<int32_t> seed, area, xy;
    std::vector<double> ms;
    long long points = 0, states = 0;
    for (int rep = 0; rep < reps; rep++) {
        points = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int b = 0; b < B; b++) {
            const int32_t* L = lab.data() + b * N;
            auto member = [&](int x, int y, int32_t id) {
                return (unsigned)x < (unsigned)w && (unsigned)y < (unsigned)h && L[(size_t)y * w + x] == id;
            };
            seed.clear(), area.clear(), xy.clear();
            for (size_t i = 0; i < N; i++) {
                if (L[i] < 0) continue;
                if ((size_t)L[i] >= seed.size()) seed.resize(L[i] + 1, -1), area.resize(L[i] + 1, 0);
                if (seed[L[i]] < 0) seed[L[i]] = (int32_t)i;
                area[L[i]]++;
            }
            int kept = 0;
            for (size_t id = 0; id < seed.size() && kept < cap; id++) {
                if (seed[id] < 0 || area[id] < std::max(min_area, 1)) continue;
                kept++;
                const int sx = seed[id] % w, sy = seed[id] / w;
                int b0 = -1;
                for (int i = 0; i < 8 && b0 < 0; i++)
                    if (member(sx + DX[(3 - i) & 7], sy + DY[(3 - i) & 7], (int32_t)id)) b0 = (3 - i) & 7;
                if (b0 < 0) {
                    xy.push_back(sx), xy.push_back(sy);
                    continue;
                }
                int x = sx, y = sy, d = b0;
                do {
                    xy.push_back(x), xy.push_back(y);
                    int t = d;
                    for (int i = 1; i <= 8; i++) {
                        t = (d + i) & 7;
                        if (member(x + DX[t], y + DY[t], (int32_t)id)) break;
                    }
                    x += DX[t], y += DY[t], d = t ^ 4;
                } while (x != sx || y != sy || d != b0);
            }
            points += (long long)xy.size() / 2;
        }
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    for (int b = 0; b < B; b++) {
        const int32_t* L = lab.data() + b * N;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const int32_t id = L[(size_t)y * w + x];
                if (id < 0) continue;
                int n = 0, n4 = 0;
                for (int d = 0; d < 8; d++) {
                    const int nx = x + DX[d], ny = y + DY[d];
                    const bool in = (unsigned)nx < (unsigned)w && (unsigned)ny < (unsigned)h && L[(size_t)ny * w + nx] == id;
                    n += in, n4 += in && !(d & 1);
                }
                if (n4 < 4) states += n;
            }
    }
    std::sort(ms.begin(), ms.end());
    std::printf("points %lld states %lld ms %.3f\n", points, states, ms[ms.size() / 2]);
    return 0;
}
