// regions_cpu -- yardstick for scripts/regions_timing.py: what a caller without mdx_mask_regions_dev
// does with the pair path's masks once they are in host memory, on one host thread: the 3x3 opening
// of DESIGN.md §7f and a plain two-pass union-find labelling (8-connected) with bounding box and area
// per component.  A program of this project's own, written from §7f; it is not the code under test.
//
//   g++ -O2 -o regions_cpu regions_cpu.cpp
//   regions_cpu <masks.u8> <w> <h> <batch> <open3> <min_area> <repeats>
// masks.u8: batch x h x w bytes.  Prints "batch <b> all <sum num_all> kept <sum num_kept> ms <median>",
// the time of all `batch` masks.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct Box { int x0, y0, x1, y1, area; };

static int find(std::vector<int>& p, int a)
{
    while (p[a] != a) a = p[a] = p[p[a]];
    return a;
}

static void open3(const uint8_t* m, int w, int h, std::vector<uint8_t>& e, std::vector<uint8_t>& d)
{
    // out-of-image neighbours neither erode nor dilate
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            uint8_t v = 1;
            for (int dy = -1; dy <= 1 && v; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    const int yy = y + dy, xx = x + dx;
                    if (yy >= 0 && yy < h && xx >= 0 && xx < w && !m[(size_t)yy * w + xx]) v = 0;
                }
            e[(size_t)y * w + x] = v;
        }
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            uint8_t v = 0;
            for (int dy = -1; dy <= 1 && !v; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    const int yy = y + dy, xx = x + dx;
                    if (yy >= 0 && yy < h && xx >= 0 && xx < w && e[(size_t)yy * w + xx]) v = 1;
                }
            d[(size_t)y * w + x] = v;
        }
}

// two passes: provisional labels with unions against the four already-visited neighbours, then the
// boxes of the roots; *kept = components with area >= min_area
static int label(const uint8_t* d, int w, int h, int min_area, std::vector<int>& lab, std::vector<int>& parent,
                 std::vector<Box>& box, int* kept)
{
    parent.clear();
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const size_t i = (size_t)y * w + x;
            if (!d[i]) {
                lab[i] = -1;
                continue;
            }
            int l = -1;
            const int nb[4][2] = {{-1, -1}, {0, -1}, {1, -1}, {-1, 0}};
            for (const auto& o : nb) {
                const int xx = x + o[0], yy = y + o[1];
                if (xx < 0 || xx >= w || yy < 0) continue;
                const int q = lab[(size_t)yy * w + xx];
                if (q < 0) continue;
                const int r = find(parent, q);
                if (l < 0) l = r;
                else if (r != l) {
                    const int lo = std::min(l, r), hi = std::max(l, r);
                    parent[hi] = lo;
                    l = lo;
                }
            }
            if (l < 0) {
                l = (int)parent.size();
                parent.push_back(l);
            }
            lab[i] = l;
        }
    box.assign(parent.size(), Box{1 << 30, 1 << 30, -1, -1, 0});
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const int q = lab[(size_t)y * w + x];
            if (q < 0) continue;
            Box& b = box[find(parent, q)];
            b.x0 = std::min(b.x0, x), b.y0 = std::min(b.y0, y), b.x1 = std::max(b.x1, x), b.y1 = std::max(b.y1, y);
            b.area++;
        }
    int all = 0;
    *kept = 0;
    for (size_t k = 0; k < box.size(); k++)
        if (parent[k] == (int)k) {
            all++;
            if (box[k].area >= min_area) ++*kept;
        }
    return all;
}

int main(int argc, char** argv)
{
    if (argc < 8) {
        std::fprintf(stderr, "usage: %s <masks.u8> <w> <h> <batch> <open3> <min_area> <repeats>\n", argv[0]);
        return 2;
    }
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), batch = std::atoi(argv[4]), op = std::atoi(argv[5]),
              min_area = std::atoi(argv[6]), reps = std::max(1, std::atoi(argv[7]));
    const size_t N = (size_t)w * h;
    std::vector<uint8_t> masks(N * batch), e(N), d(N);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(masks.data(), 1, masks.size(), f) != masks.size()) {
        std::fprintf(stderr, "cannot read %d masks from %s\n", batch, argv[1]);
        return 1;
    }
    std::fclose(f);
    std::vector<int> lab(N), parent;
    std::vector<Box> box;
    std::vector<double> ms;
    long long all = 0, kept = 0;
    for (int r = 0; r < reps; r++) {
        all = kept = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int b = 0; b < batch; b++) {
            const uint8_t* m = masks.data() + N * b;
            if (op) open3(m, w, h, e, d);
            int k = 0;
            all += label(op ? d.data() : m, w, h, min_area, lab, parent, box, &k);
            kept += k;
        }
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    std::printf("batch %d all %lld kept %lld ms %.4f\n", batch, all, kept, ms[ms.size() / 2]);
    return 0;
}
