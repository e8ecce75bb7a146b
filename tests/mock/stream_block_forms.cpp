// stream_block_forms.cpp -- prints what the host rules of the stream block push (csrc/sg_stream_host.hpp) decide for a list of call shapes, one line per
// shape: the forms the call is offered in order (the first is the one it takes; the rest is where it goes when a launcher reports "not covered"), then
// each tile form's geometry and grid and the walk's band count.  Plain g++, no GPU, no HIP: tests/test_stream_block_forms.py feeds the shapes on
// standard input -- n fma streams ticks misaligned centre moment_terms dma_switch moment_switch nwaves -- and compares with tests/golden/stream_block_forms.txt.
#include <cstdio>

#include "sg_stream_host.hpp"

struct Pair { float x, y; };

int main()
{
    // pack_taps: tap k is half k & 1 of pair k >> 1
    const float w[5] = {1.0f, 2.0f, 3.0f, 4.0f, 5.0f};
    Pair pairs[3] = {};
    sg::pack_taps(w, 5, pairs);
    printf("pack_taps %g %g | %g %g | %g %g\n", pairs[0].x, pairs[0].y, pairs[1].x, pairs[1].y, pairs[2].x, pairs[2].y);

    static const char *const names[] = {"MOMENT_TILES", "DMA_TILES", "REGISTER_TILES", "WALK"};
    int n, fma, centre, terms, dma, mom;
    unsigned long long streams, ticks, nwaves;
    unsigned mis;
    while (scanf("%d %d %llu %llu %u %d %d %d %d %llu", &n, &fma, &streams, &ticks, &mis, &centre, &terms, &dma, &mom, &nwaves) == 10) {
        printf("n=%d fma=%d streams=%llu ticks=%llu mis=%u centre=%d terms=%d dma=%d mom=%d:", n, fma, streams, ticks, mis, centre, terms, dma, mom);
        for (int first = sg::MOMENT_TILES; first <= sg::WALK; ++first) {
            const sg::BlockForm form = sg::block_form(n, fma != 0, streams, ticks, mis, centre != 0, dma != 0, mom != 0, [&] { return terms; }, first);
            first = form;
            printf(" %s", names[form]);
            sg::TileGeom geo;
            unsigned grid = 0;
            // the tile shapes of the launchers (sg_stream_dma.hip: launch_bank_dma_mom, launch_bank_dma_shape; sg_stream_roll.hip: dispatch_bank_tile)
            if (form == sg::MOMENT_TILES) {
                const unsigned want = (unsigned)(streams / 128 / 4);
                grid = sg::tile_geom(streams, 128, ticks, 32, want < 16u ? 16u : (want > 64u ? 64u : want), 8, &geo);
            } else if (form == sg::DMA_TILES) {
                grid = sg::tile_geom(streams, 128, ticks, 32, 128, n > 5 && n <= 11 && fma ? 8 : 4, &geo);
            } else if (form == sg::REGISTER_TILES) {
                grid = sg::tile_geom(streams, 256, ticks, sg::STREAM_TILE_ROWS, 64, sg::STREAM_TILE_WPB, &geo);
            } else {
                printf("(bands=%zu of %llu waves)", sg::walk_bands(ticks, (streams + 127) / 128, nwaves, n), nwaves);
                continue;
            }
            printf("(strips=%u bands=%u group=%u total=%llu grid=%u)", geo.strips, geo.bands, geo.group, geo.total, grid);
        }
        printf("\n");
    }
    return 0;
}
