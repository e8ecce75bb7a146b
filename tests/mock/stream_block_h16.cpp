// stream_block_h16.cpp -- prints what block_plan_h16 (csrc/sg_stream_host.hpp) decides for a list of 16-bit block pushes, one line per shape.  Plain g++,
// no GPU, no HIP: tests/test_stream_h16_host.py feeds the shapes on standard input -- n fma streams ticks misaligned centre moment_terms dma_switch
// moment_switch -- and holds every line to the rule restated in Python.
#include <cstdio>

#include "sg_stream_host.hpp"

int main()
{
    static const char *const names[] = {"MOMENT_TILES", "DMA_TILES", "REGISTER_TILES", "WALK"};
    int n, fma, centre, terms, dma, mom;
    unsigned long long streams, ticks;
    unsigned mis;
    while (scanf("%d %d %llu %llu %u %d %d %d %d", &n, &fma, &streams, &ticks, &mis, &centre, &terms, &dma, &mom) == 9) {
        const sg::H16Plan p = sg::block_plan_h16(n, fma != 0, streams, ticks, mis, centre != 0, dma != 0, mom != 0, [&] { return terms; });
        printf("n=%d fma=%d streams=%llu ticks=%llu mis=%u centre=%d terms=%d dma=%d mom=%d:", n, fma, streams, ticks, mis, centre, terms, dma, mom);
        if (p.route == sg::H16_TILES) {
            printf(" TILES %s head=%zu body=%zu wpb=%d", names[p.form], p.head, p.body, p.wpb);
            if (p.body) printf(" strips=%u bands=%u group=%u total=%llu grid=%u", p.geo.strips, p.geo.bands, p.geo.group, p.geo.total, p.grid);
        } else {
            printf(" STAGED chunks=");
            int shown = 0;
            unsigned long long count = 0;
            for (unsigned long long done = 0; done < ticks; done += p.chunk, ++count) {
                const unsigned long long part = ticks - done < p.chunk ? ticks - done : p.chunk;
                if (shown < 3 || done + p.chunk >= ticks) { printf("%s%llu", shown ? "," : "", part); ++shown; }
            }
            printf(" count=%llu", count);
        }
        printf("\n");
    }
    return 0;
}
