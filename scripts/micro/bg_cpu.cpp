// bg_cpu.cpp -- the CPU side of scripts/bg_timing.py: tests/bg_check.cpp's per-pixel loop (the scalar restatement
// of the contract, NOT OpenCV) on one host thread and on `threads`, rows split evenly, on the frames the device
// was timed on.
//   g++ -O2 -ffp-contract=off -pthread -I tests scripts/micro/bg_cpu.cpp
//   bg_cpu FRAMES w h channels nframes warm threads
// FRAMES: nframes packed frames.  The model first takes the frames `warm` times round (untimed, on `threads`
// threads: the result does not depend on the split), then each
// configuration takes them once more, timed; prints "threads ms_per_frame checksum" per configuration (the
// checksum is the sum of the mask bytes: the configurations must agree).
#include <chrono>
#include <cstdlib>
#include <thread>

#define BG_CHECK_NO_MAIN
#include "bg_check.cpp"

int main(int argc, char** argv)
{
    if (argc != 8) return fprintf(stderr, "usage: bg_cpu FRAMES w h channels nframes warm threads\n"), 2;
    const int w = atoi(argv[2]), h = atoi(argv[3]), cn = atoi(argv[4]), nf = atoi(argv[5]), warm = atoi(argv[6]);
    const int threads = atoi(argv[7]);
    const size_t fb = (size_t)w * h * cn;
    std::vector<uint8_t> frames(fb * nf), mask((size_t)w * h);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(frames.data(), 1, frames.size(), f) != frames.size()) return fprintf(stderr, "short frames\n"), 2;
    fclose(f);
    const bgc::Params P{500, 5, 16.f, 9.f, 0.9f, 15.f, 4.f, 75.f, 0.05f, 1, 127, 0.5f};
    bgc::Model warmed;
    warmed.init(w, h, cn, P);
    warmed.count = false;     // the counters are not atomic
    // one frame on nt threads, the rows split evenly
    auto frame_on = [&](bgc::Model& M, int t, int nt) {
        M.nframes++;
        const float alphaT = bgc::Model::alpha_of(P, M.nframes, -1.0);
        std::vector<std::thread> pool;
        for (int i = 1; i < nt; i++)
            pool.emplace_back([&, i] { M.apply_rows(&frames[fb * t], alphaT, mask.data(), h * i / nt, h * (i + 1) / nt); });
        M.apply_rows(&frames[fb * t], alphaT, mask.data(), 0, h / nt);
        for (auto& th : pool) th.join();
    };
    for (int r = 0; r < warm; r++)
        for (int t = 0; t < nf; t++) frame_on(warmed, t, threads);
    for (int nt : {1, threads}) {
        bgc::Model M = warmed;
        unsigned long long sum = 0;
        const auto t0 = std::chrono::steady_clock::now();
        for (int t = 0; t < nf; t++) {
            frame_on(M, t, nt);
            for (uint8_t v : mask) sum += v;
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("%d %.3f %llu\n", nt, ms / nf, sum);
    }
    return 0;
}
