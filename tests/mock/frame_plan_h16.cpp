// frame_plan_h16.cpp -- prints what csrc/sg_2d_h16_host.hpp decides, one line per request read from standard input.  Plain g++, no GPU, no HIP:
// tests/test_h16_2d_host.py feeds the requests and holds every line to the rules restated in Python.
//   plan n additive xdom method rows cols in_off out_off in_stride in_pitch out_stride out_pitch out_elem roll_tile tiles   -> frame_plan_h16's route
//        (n only labels the line: the half window reaches the rule through `additive`, the launcher's own predicate; in_off / out_off = the
//        bases' byte offsets from a 256-byte boundary)
//   stage rows cols images                                                                                                  -> frame_stage_h16
//   overlap a_off a_elem a_pitch a_stride b_off b_elem b_pitch b_stride rows cols images                                    -> frames_overlap
//        (a_off / b_off = byte offsets of the two bases inside one buffer)
#include <cstdio>
#include <cstring>

#include "sg_2d_h16_host.hpp"

int main()
{
    char word[16];
    const uintptr_t base = (uintptr_t)1 << 32;
    while (scanf("%15s", word) == 1) {
        if (!strcmp(word, "plan")) {
            int n, additive, xdom, roll, tiles;
            unsigned long long in_off, out_off;
            sg::FrameShapeH16 s;
            if (scanf("%d %d %d %d %d %d %llu %llu %lld %lld %lld %lld %d %d %d", &n, &additive, &xdom, &s.method, &s.rows, &s.cols, &in_off, &out_off, &s.in_stride,
                      &s.in_pitch, &s.out_stride, &s.out_pitch, &s.out_elem, &roll, &tiles) != 15) return 1;
            s.in_base = base + in_off; s.out_base = 2 * base + out_off;
            s.additive_tile = additive != 0; s.x_dominant = xdom != 0; s.roll_tile_switch = roll != 0; s.tiles_switch = tiles != 0;
            printf("plan n=%d: %s\n", n, sg::frame_plan_h16(s) == sg::FRAME_H16_TILES ? "TILES" : "STAGED");
        } else if (!strcmp(word, "stage")) {
            int rows, cols;
            unsigned long long images;
            if (scanf("%d %d %llu", &rows, &cols, &images) != 3) return 1;
            const sg::FrameStageH16 g = sg::frame_stage_h16(rows, cols, images);
            printf("stage: stride=%d frame=%zu frames=%zu\n", g.stride, g.frame, g.frames);
        } else if (!strcmp(word, "overlap")) {
            unsigned long long a_off, b_off, a_elem, b_elem, images;
            long long a_pitch, a_stride, b_pitch, b_stride;
            int rows, cols;
            if (scanf("%llu %llu %lld %lld %llu %llu %lld %lld %d %d %llu", &a_off, &a_elem, &a_pitch, &a_stride, &b_off, &b_elem, &b_pitch, &b_stride, &rows, &cols,
                      &images) != 11) return 1;
            printf("overlap: %d\n", sg::frames_overlap(base + a_off, a_elem, a_pitch, a_stride, base + b_off, b_elem, b_pitch, b_stride, rows, cols, images) ? 1 : 0);
        } else return 1;
    }
    return 0;
}
