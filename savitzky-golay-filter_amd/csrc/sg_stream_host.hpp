// sg_stream_host.hpp -- host-only rules of the stream block push (no device types: included by g++ translation units too): which form a call takes
// (block_form), the geometry of its tiles or bands, how taps are packed.  tests/mock/stream_block_forms.cpp prints them for a table of call shapes.
#pragma once

#include <cstddef>

namespace sg {

// Block-moment form of the fused bank's LDS-DMA tiles (sg_stream_dma.hip, MomTaps): half windows it is built for, and the host fit's result
constexpr int STREAM_MOMENT_MIN_N = 12;                      // below, a window holds at most two whole 8-tick blocks: nothing to win
constexpr int STREAM_MOMENT_MAX_N = 20;                      // interleaved A/B on config 3's shape (profiles/r05_stream_moment_ab.txt): n = 12 / 14 / 16 10 % ahead of the
                                                             // tap-by-tap tiles, 20 level, 24 / 28 / 32 behind by 5 / 9 / 2 % (their 2n halo rows want the waves the moment tiles give up)
constexpr int STREAM_MOMENT_OFFSETS = 2 * STREAM_MOMENT_MAX_N - 6;   // block offsets 0 .. 2n - 7
struct StreamMomentFit {
    int   terms;                                             // 1..3 moments per block (polynomial degree + 1)
    float c[3][STREAM_MOMENT_OFFSETS];                       // c[s][off]: weight of moment s of the block that starts `off` taps into the window
};
// 0 = the table is not a polynomial of degree <= 2 to 3e-7 of its largest tap (or n outside the range): keep the tap-by-tap tiles
int stream_moment_fit(int n, const float *center_weights, StreamMomentFit *fit);
constexpr int STREAM_TILE_ROWS = 16, STREAM_TILE_WPB = 2;    // register tiles: 16 tick rows, 2 waves per block
constexpr int STREAM_DMA_MIN_TICKS = 64;                     // LDS-DMA tiles: whole 128-stream strips, two tiles of 32 ticks
// taps w[0 .. count) into pairs: tap k is half k & 1 of pair k >> 1 (the kernels read one tap out of an aligned SGPR pair with op_sel)
template <class Pair>
inline void pack_taps(const float *w, int count, Pair *pairs)
{
    for (int k = 0; k < count; ++k) {
        if (k & 1) pairs[k >> 1].y = w[k]; else pairs[k >> 1].x = w[k];
    }
}

// May this call take tiles: rows of whole `multiple`-stream units (the buffer range check works on whole accesses), rows < 2 GiB (the descriptors),
// the bases of samples / out / ring 16-byte aligned (misaligned = the low four bits of the three addresses, or-ed), at least min_ticks ticks
inline bool tiles_take(size_t streams, size_t multiple, unsigned misaligned, size_t ticks, size_t min_ticks)
{
    return streams % multiple == 0 && (unsigned long long)streams * 4 < 0x7fffff00ull && misaligned == 0 && ticks >= min_ticks;
}

// Tiles of strip_width streams x TR ticks, dealt in groups of `group` neighbouring strips: inside a group band after band, strips fastest (tile_of,
// sg_stream_roll.hpp); `total` counts the last group as a whole one.  Returns the grid (WPB tiles per block, a multiple of 8 blocks: one share per
// XCD), 0 = not covered: the kernels index tiles with 32 bits.
struct TileGeom { unsigned strips, bands, group; unsigned long long total; };
inline unsigned tile_geom(size_t streams, unsigned strip_width, size_t ticks, int TR, unsigned group, int WPB, TileGeom *geo)
{
    geo->strips = (unsigned)((streams + strip_width - 1) / strip_width);
    geo->bands = (unsigned)((ticks + (size_t)TR - 1) / (size_t)TR);
    geo->group = group > geo->strips ? geo->strips : group;
    const unsigned groups = (geo->strips + geo->group - 1) / geo->group;
    geo->total = (unsigned long long)groups * geo->group * geo->bands;
    if (geo->total >= 0x7fffff00ull) return 0;
    return ((unsigned)((geo->total + (unsigned)WPB - 1) / (unsigned)WPB) + 7u) & ~7u;
}

// The walk's bands of ticks: the resident waves take the strips x bands items round robin, so the call lasts (rounds of items) x (rows per band +
// 2n warm-up rows).  Rounds 1-3 took ceil(waves / strips) bands, which is right when the strips divide the waves (65 536 streams: 512
// strips, 4 bands, one round) and badly wrong next to it: 66 560 streams = 520 strips x 4 bands = 2080 items on 2048 waves -- a second
// round for 32 items, 0.595 ms where 65 536 streams take 0.44.  Now the band count with the cheapest (rounds x rows) is taken
// (a band re-reads 2n warm-up rows: keep it >= 8 windows).
inline size_t walk_bands(size_t ticks, size_t strips, size_t nwaves, int n)
{
    const size_t ws = 2 * (size_t)n + 1;
    const size_t max_bands = ticks / (8 * ws) > 0 ? ticks / (8 * ws) : 1;
    size_t bands = 1;
    // Candidates: every count up to the one that gives each resident wave an item (ceil(waves / strips), what rounds 1-3 took), bounded
    // by max_bands.  (round 4 stopped the search at 64, so a bank of FEW strips and a long block -- 1024 streams = 8 strips
    // x 100 000 ticks -- ran on 512 of its 2048 waves; the search is coarse above 64 to stay a few hundred steps.)
    double best = 1e300;
    const size_t fill = (nwaves + strips - 1) / strips;
    size_t top = fill > 64 ? fill : 64;
    if (top > max_bands) top = max_bands;
    for (size_t b = 1; b <= top; b += (b < 64 ? 1 : (b / 64 < 1 ? 1 : b / 64))) {
        const size_t rows = (ticks + b - 1) / b + 2 * (size_t)n;
        const size_t rounds = (strips * b + nwaves - 1) / nwaves;
        const double cost = (double)rounds * (double)rows;
        if (cost < best * 0.999) { best = cost; bands = b; }
    }
    if (top > 64) {                                          // the exact fill count is always a candidate
        const size_t b = top;
        const double cost = (double)((strips * b + nwaves - 1) / nwaves) * (double)((ticks + b - 1) / b + 2 * (size_t)n);
        if (cost < best * 0.999) { best = cost; bands = b; }
    }
    return bands;
}

// ---- which form a block push takes: the one place that says so ----
// In this order; sg_bank_roll_launch asks again with first = the next form when a launcher reports "not covered" (a refused launch, a tile count
// beyond 32 bits).  moment_terms() is the host fit (stream_moment_fit's terms, 0 = the taps are no polynomial of degree <= 2), called only where
// everything else admits the block-moment tiles.  dma_switch / moment_switch: SAVGOL_HIP_STREAM_DMA / SAVGOL_HIP_STREAM_MOMENT (0 = A/B runs against
// the forms further down).
enum BlockForm { MOMENT_TILES, DMA_TILES, REGISTER_TILES, WALK };
template <class Fit>
inline BlockForm block_form(int n, bool fma, size_t streams, size_t ticks, unsigned misaligned, bool centre, bool dma_switch, bool moment_switch,
                            Fit &&moment_terms, int first = MOMENT_TILES)
{
    const bool dma_shape = dma_switch && tiles_take(streams, 128, misaligned, ticks, STREAM_DMA_MIN_TICKS);
    // the fused bank where its taps are a polynomial of degree <= 2 (config 3: linear): blocks of 8 ticks through their moments
    if (first <= MOMENT_TILES && dma_shape && fma && moment_switch && n >= STREAM_MOMENT_MIN_N && n <= STREAM_MOMENT_MAX_N) {
        const int terms = moment_terms();
        // quadratic taps that sum to zero (a second derivative): the outputs are small against the samples, and what the fitted polynomial leaves of the
        // reference's fp32 taps (<= 3e-7 of the largest) shows in them -- 1.4e-6 of the oracle where the tap-by-tap tiles are at 0.7e-6 and the reference's
        // own loop at 0.6e-6 (tools/offset_probe_1d.py, R6.16).  Those banks keep the tap-by-tap tiles (7 % slower); config 3's taps are linear.
        if (terms > 0 && !(centre && terms >= 3)) return MOMENT_TILES;
    }
    // Which half windows take the LDS-DMA tiles (profiles/r05_stream_dma.txt, config 3's shape, sustained): every n <= 16; above 16 the FMA bank gains
    // 6 % (n = 17) ... 15 % (n = 32) over the accumulator-ring walk and the bit-exact bank 10-19 % from n = 24, while at n = 17 its sustained time is
    // 10 % worse (0.603 against 0.548 ms: twice the vector instructions, and the chip lowers its clock under them) -- it keeps the walk below 20.
    if (first <= DMA_TILES && dma_shape && (n <= 16 || fma || n >= 20)) return DMA_TILES;
    // Where the register tiles pay (profiles/r04_stream_tile.txt; config 3's shape, 65 536 streams x 4096 ... 16 384 ticks, five variants of
    // streams per lane x rows per tile x waves per block, strips per group 8 ... 256): the reference-order bank at n <= 12 (n = 4: 0.393 vs
    // 0.420 ms, n = 8: 0.408 vs 0.425); at n = 16 its 2n = 32 halo rows per 16-row tile (3 x the row reads out of L2) cancel the gain
    // (0.44-0.47 vs 0.45-0.46), and the fused multiply-add bank's walk is level or ahead at every half window (n = 16: 0.400-0.425 vs
    // 0.403-0.446).  Both forms sit at 0.60-0.69 of the roofline on this 2 GB call, a 0.4 ms launch, whatever the call's length.
    if (first <= REGISTER_TILES && !fma && n <= 12 && tiles_take(streams, 4, misaligned, ticks, 2 * STREAM_TILE_ROWS)) return REGISTER_TILES;
    return WALK;                                             // every half window, every shape (sg_stream_roll.hip)
}

}  // namespace sg
