// grad_plan_i16.cpp -- prints what csrc/sg_2d_grad16_host.hpp decides, one line per request read from standard input.  Plain g++, no GPU, no HIP:
// tests/test_i16_2d_grad_host.py feeds the requests and holds every line to the rule restated in Python.
//   plan nx ny gx_ok gy_ok want_gx want_gy rows cols in_off gx_off gy_off in_stride in_pitch out_stride out_pitch out_elem roll_tile direct   -> grad_plan_i16's route
//        (gx_ok / gy_ok: the factors' answers, which reach the rule as facts; in_off / gx_off / gy_off = the bases' byte offsets from a 256-byte boundary)
//   stage rows cols images                                                                                                                   -> grad_stage_i16
#include <cstdio>
#include <cstring>

#include "sg_2d_grad16_host.hpp"

int main()
{
    char word[16];
    const uintptr_t base = (uintptr_t)1 << 32;
    while (scanf("%15s", word) == 1) {
        if (!strcmp(word, "plan")) {
            int gx_ok, gy_ok, want_gx, want_gy, roll, direct;
            unsigned long long in_off, gx_off, gy_off;
            sg::GradShapeI16 s;
            if (scanf("%d %d %d %d %d %d %d %d %llu %llu %llu %lld %lld %lld %lld %d %d %d", &s.nx, &s.ny, &gx_ok, &gy_ok, &want_gx, &want_gy, &s.rows, &s.cols, &in_off,
                      &gx_off, &gy_off, &s.in_stride, &s.in_pitch, &s.out_stride, &s.out_pitch, &s.out_elem, &roll, &direct) != 18) return 1;
            s.in_base = base + in_off; s.gx_base = 2 * base + gx_off; s.gy_base = 3 * base + gy_off;
            s.gx_direct = gx_ok != 0; s.gy_direct = gy_ok != 0; s.want_gx = want_gx != 0; s.want_gy = want_gy != 0;
            s.roll_tile_switch = roll != 0; s.direct_switch = direct != 0;
            printf("plan n=%dx%d: %s\n", s.nx, s.ny, sg::grad_plan_i16(s) == sg::GRAD_I16_DIRECT ? "DIRECT" : "STAGED");
        } else if (!strcmp(word, "stage")) {
            int rows, cols;
            unsigned long long images;
            if (scanf("%d %d %llu", &rows, &cols, &images) != 3) return 1;
            const sg::FrameStageH16 g = sg::grad_stage_i16(rows, cols, images);
            printf("stage: stride=%d frame=%zu frames=%zu\n", g.stride, g.frame, g.frames);
        } else return 1;
    }
    return 0;
}
