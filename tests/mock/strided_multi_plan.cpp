// strided_multi_plan.cpp -- prints what strided_multi_plan (csrc/sg_k1d_strided_multi_host.hpp) decides for a list of multi-field strided calls, one
// line per call.  Plain g++, no GPU, no HIP: tests/test_strided_multi_host.py feeds the calls on standard input -- njobs in_stride in_pitch
// out_stride out_pitch channels count boundary_aware reference_summation, then half_window boundary in_address out_address for each job -- and
// holds every line to the rule restated in Python.
#include <cstdio>

#include "sg_k1d_strided_multi_host.hpp"

int main()
{
    int njobs, aware, ref;
    unsigned long long in_stride, in_pitch, out_stride, out_pitch, channels, count;
    while (scanf("%d %llu %llu %llu %llu %llu %llu %d %d", &njobs, &in_stride, &in_pitch, &out_stride, &out_pitch, &channels, &count, &aware, &ref) == 9) {
        if (njobs < 1 || njobs > sg::STRIDED_MULTI_MAX_JOBS) return 1;
        sg::StridedMultiField jobs[sg::STRIDED_MULTI_MAX_JOBS] = {};
        for (int k = 0; k < njobs; ++k) {
            unsigned long long in, out;
            if (scanf("%d %d %llu %llu", &jobs[k].half_window, &jobs[k].boundary, &in, &out) != 4) return 1;
            jobs[k].in = (uintptr_t)in;
            jobs[k].out = (uintptr_t)out;
        }
        const sg::StridedMultiPlan p = sg::strided_multi_plan(jobs, njobs, in_stride, in_pitch, out_stride, out_pitch, channels, count, aware != 0, ref != 0);
        printf("launches=%d groups=", p.launches);
        for (int g = 0; g < p.groups; ++g) printf("%s%d", g ? "," : "", p.per[g]);
        printf("\n");
    }
    printf("bounds jobs=%d per_launch=%d max_length=%zu\n", sg::STRIDED_MULTI_MAX_JOBS, sg::STRIDED_MULTI_MAX_PER_LAUNCH, sg::STRIDED_MULTI_MAX_LENGTH);
    return 0;
}
