// region_parents_cpu.cpp -- the host yardstick of scripts/region_parents_timing.py: what a caller of
// mdx_mask_regions_dev does without mdx_region_parents_dev.  From the label images (copied to the host) it
// flood-fills the background with 4-connectivity on one thread, takes each component's first pixel and area
// from the labels, and applies include/mdx.h's parent rule to the first max_regions components of at least
// min_area pixels.
//   region_parents_cpu <labels.i32> <w> <h> <batch> <min_area> <max_regions> <reps>
// prints: external <sum over the batch> nested <sum> ms <median of reps, whole batch>
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

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
    std::vector<int32_t> bg(N), stack, seed, area;
    std::vector<uint8_t> frame;      // per background component: touches the frame's edge
    std::vector<int32_t> first;      // per background component: its first pixel
    std::vector<double> ms;
    long long external = 0, nested = 0;
    for (int rep = 0; rep < reps; rep++) {
        external = nested = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int b = 0; b < B; b++) {
            const int32_t* L = lab.data() + b * N;
            std::fill(bg.begin(), bg.end(), -1);
            frame.clear(), first.clear(), seed.clear(), area.clear();
            for (size_t i = 0; i < N; i++) {
                if (L[i] >= 0) {
                    if ((size_t)L[i] >= seed.size()) seed.resize(L[i] + 1, -1), area.resize(L[i] + 1, 0);
                    if (seed[L[i]] < 0) seed[L[i]] = (int32_t)i;
                    area[L[i]]++;
                    continue;
                }
                if (bg[i] >= 0) continue;
                const int32_t id = (int32_t)first.size();
                first.push_back((int32_t)i);
                uint8_t edge = 0;
                bg[i] = id;
                stack.assign(1, (int32_t)i);
                while (!stack.empty()) {
                    const int32_t p = stack.back();
                    stack.pop_back();
                    const int x = p % w, y = p / w;
                    edge |= x == 0 || y == 0 || x == w - 1 || y == h - 1;
                    const int32_t nb[4] = {y > 0 ? p - w : -1, x > 0 ? p - 1 : -1, x < w - 1 ? p + 1 : -1, y < h - 1 ? p + w : -1};
                    for (const int32_t q : nb)
                        if (q >= 0 && L[q] < 0 && bg[q] < 0) bg[q] = id, stack.push_back(q);
                }
                frame.push_back(edge);
            }
            int kept = 0;
            for (size_t c = 0; c < seed.size() && kept < cap; c++) {
                if (area[c] < min_area) continue;
                kept++;
                const int32_t s = seed[c];
                const bool ext = s < w || frame[bg[s - w]];
                external += ext;
                nested += !ext && L[first[bg[s - w]] - w] >= 0;
            }
        }
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    printf("external %lld nested %lld ms %.3f\n", external, nested, ms[ms.size() / 2]);
    return 0;
}
