// outline_check.cpp -- the border-following rule of the region outlines (motion_detection_amd/csrc/mdx_plan.h
// outline_next_dir, outline_prev_dir, outline_dx, outline_dy, outline_rounds) run on a CPU: the functions the
// kernels are built on, for every input (tests/test_region_outlines.py compares with its own tracer's loop).
//   g++ -std=c++17 -I motion_detection_amd/csrc -I include tests/outline_check.cpp
// Prints D[0..7] as x y pairs, then next prev for mask 0..255 x b 0..7; with an argument, outline_rounds of
// 1x1, 512x512, 1920x1080 and 3840x2160.
#include <cstdio>

#include "mdx_plan.h"

int main(int argc, char**)
{
    if (argc > 1) {
        std::printf("%d %d %d %d\n", mdx::outline_rounds(1, 1), mdx::outline_rounds(512, 512), mdx::outline_rounds(1920, 1080),
                    mdx::outline_rounds(3840, 2160));
        return 0;
    }
    for (int d = 0; d < 8; d++) std::printf("%d %d\n", mdx::outline_dx(d), mdx::outline_dy(d));
    for (unsigned m = 0; m < 256; m++)
        for (int b = 0; b < 8; b++) std::printf("%d %d\n", mdx::outline_next_dir(m, b), mdx::outline_prev_dir(m, b));
    return 0;
}
