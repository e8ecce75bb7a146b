// stream_block_multi_i16.cpp -- prints what block_plan_multi_i16 (csrc/sg_stream_host.hpp) decides for a list of fused multi-output block pushes on
// int16 storage, one line per shape.  Plain g++, no GPU, no HIP: tests/test_stream_multi_i16_host.py feeds the shapes on standard input -- count streams
// ticks misaligned dma_switch moment_switch, then n fma centre moment_terms for each bank -- and holds every line to the rule restated in Python.
// The last line prints the shipped bound table.
#include <cstdio>

#include "sg_stream_host.hpp"

int main()
{
    int count, dma, mom;
    unsigned long long streams, ticks;
    unsigned mis;
    while (scanf("%d %llu %llu %u %d %d", &count, &streams, &ticks, &mis, &dma, &mom) == 6) {
        sg::MultiBank banks[sg::STREAM_MULTI_MAX_BANKS] = {};
        int terms[sg::STREAM_MULTI_MAX_BANKS] = {};
        printf("count=%d streams=%llu ticks=%llu mis=%u dma=%d mom=%d banks=", count, streams, ticks, mis, dma, mom);
        for (int k = 0; k < count; ++k) {
            int n, fma, centre;
            if (scanf("%d %d %d %d", &n, &fma, &centre, &terms[k % sg::STREAM_MULTI_MAX_BANKS]) != 4) return 1;
            if (k < sg::STREAM_MULTI_MAX_BANKS) banks[k] = sg::MultiBank{n, fma != 0, centre != 0};
            printf("%s%d/%d/%d/%d", k ? "," : "", n, fma, centre, terms[k % sg::STREAM_MULTI_MAX_BANKS]);
        }
        const sg::MultiPlan p = sg::block_plan_multi_i16(banks, count, streams, ticks, mis, dma != 0, mom != 0, [&](int k) { return terms[k]; });
        if (p.launches == 0) {
            printf(": SINGLE calls=%d\n", count);
        } else {
            printf(": FUSED launches=%d per=%d,%d head=%zu body=%zu wpb=%d rows=%d strips=%u bands=%u group=%u total=%llu grid=%u\n", p.launches, p.per[0], p.per[1],
                   p.head, p.body, p.wpb, 4 * p.dp, p.geo.strips, p.geo.bands, p.geo.group, p.geo.total, p.grid);
        }
    }
    printf("bounds fused %d %d exact %d %d\n", sg::stream_multi_i16_max_n(true, 2), sg::stream_multi_i16_max_n(true, 3), sg::stream_multi_i16_max_n(false, 2),
           sg::stream_multi_i16_max_n(false, 3));
    return 0;
}
