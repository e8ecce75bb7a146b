// sg_stream_host.hpp -- host-only rules of the stream block push (no device types: included by g++ translation units too): which form a call takes
// (block_form), the geometry of its tiles or bands, how taps are packed, the wait counts of the LDS-DMA tiles (DmaQueue) and the routes of the 16-bit
// call (block_plan_h16), of the fused multi-output call (block_plan_multi) and of the fused multi-output call on 16-bit storage (block_plan_multi_h16,
// block_plan_multi_i16).  tests/mock/stream_block_forms.cpp, stream_block_h16.cpp, stream_block_multi.cpp, stream_block_multi_h16.cpp,
// stream_block_multi_i16.cpp, dma_queue.cpp, dma_queue_multi.cpp and dma_queue_multi_h16.cpp print them for tables of call shapes.
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

// ---- LDS-DMA tiles (sg_stream_dma.hpp): compile-time bookkeeping, plain constexpr so that tests/mock/dma_queue.cpp can hold it to a simulated queue ----
// vmcnt bookkeeping.  A DMA instruction moves RPD rows (2 rows of 512 bytes: fp32 rows; 4 rows of 256 bytes: 16-bit rows); a step consumes the RPD rows of
// one DMA.  The wave's vector-memory queue, in issue order: the DP DMAs of the prologue, then per step j: the stores of the outputs that rows RPD j ..
// RPD j + RPD - 1 finish, then DMA j + DP (if it exists).  ROWS = TR + 2N is rounded up to whole DMAs (pad rows finish no output).  A finished output
// row issues SPR stores: 1, or one per output of the fused multi-output tiles (sg_stream_dma_multi.hip).
template <int N, int TR, int DP, int RPD = 2, int SPR = 1> struct DmaQueue {
    static constexpr int NI = (TR + 2 * N + RPD - 1) / RPD;
    static constexpr int done(int r) { return SPR * (r - 2 * N < 0 ? 0 : (r - 2 * N > TR ? TR : r - 2 * N)); }     // stores issued by the outputs that rows < r finish
    static constexpr int dmas(int a, int b) { int c = 0; for (int j = a; j < b; ++j) c += (j >= 0 && j + DP < NI) ? 1 : 0; return c; }  // DMAs issued by steps [a, b)
    // operations younger than DMA p when step g starts (p = g + 1 is the one step g waits for)
    static constexpr int younger(int p, int g)
    {
        if (p < DP) return (DP - 1 - p) + done(RPD * g) + dmas(0, g);                   // a prologue DMA: the rest of the prologue, then every step so far
        const int born = p - DP;                                                        // issued at the END of step `born`
        return (done(RPD * g) - done(RPD * born + RPD)) + dmas(born + 1, g);
    }
};

// ---- block moments down the tick axis (round 5, profiles/EXPERIMENTS.md R5.9) ----
// The fused bank's taps are a polynomial in the tap index for the filters streams are made of (config 3: m = 2, d = 1 -- LINEAR taps).  A tile's rows
// are cut into blocks of 8 ticks (tile-relative rows 8j .. 8j + 7); output m = 8a + p takes the rows of its window that fill whole blocks through the
// blocks' M moments (M coefficients per block, the same for both streams of the lane) and only the rows before its first / after its last whole block
// tap by tap: at n = 16, 7 direct taps + 3.25 blocks x M per output on average, plus M operations per input row for the moments -- 17.5 (M = 2)
// instead of 33 packed multiply-adds per output pair.  Same idea as sg_k1d_momenth.hpp, along the other axis.
template <int N> struct MomGeom {
    static constexpr int BK = 8;
    static constexpr int NOFF = 2 * N - (BK - 1) + 1;                                    // block offsets 8j - m = 0 .. 2N - 7
    static constexpr int jf(int m) { return m / BK + (m % BK ? 1 : 0); }                 // first / last block that lies wholly inside the window m .. m + 2N
    static constexpr int jl(int m) { return (m + 2 * N - (BK - 1)) / BK; }
    static constexpr bool whole(int m, int r) { return r >= m && r <= m + 2 * N && r / BK >= jf(m) && r / BK <= jl(m); }
    static constexpr bool direct(int m, int r) { return r >= m && r <= m + 2 * N && !whole(m, r); }
    static_assert(N >= BK / 2, "a window holds at least one whole block");
};

// ---- the block push on 16-bit rows (savgol_streambank_push_block_h16): which route a call takes, decided before anything is enqueued ----
// (waves per block, strips per group) of the LDS-DMA tile launchers, by form, half window and bank: launch_bank_dma_shape / launch_bank_dma_mom
// (sg_stream_dma.hip) and their 16-bit mirrors (sg_stream_dma_h16.hip)
struct DmaTileShape { int wpb; unsigned group; };
inline DmaTileShape dma_tile_shape(BlockForm form, int n, bool fma, size_t streams)
{
    if (form == MOMENT_TILES) {
        const unsigned want = (unsigned)(streams / 128 / 4);
        return DmaTileShape{8, want < 16u ? 16u : (want > 64u ? 64u : want)};
    }
    return DmaTileShape{n > 5 && n <= 11 && fma ? 8 : 4, 128u};
}

// TILES: streams % 128 == 0, ticks >= 64, both 16-bit bases 16-byte aligned (misaligned = their low four bits, or-ed), rows under the descriptor
// limit, and the fp32 call on aligned buffers (the twin) takes LDS-DMA tiles, block moments or tap by tap, whose tile count 32 bits index.  The call is
// then a head of STREAM_DMA_MIN_TICKS = 64 ticks = two whole 32-tick bands (widened into fp32 scratch and pushed through the fp32 block push: the twin's
// own tiles of bands 0 and 1; 2n <= 64, so only the head reads the fp32 ring) and a body of ticks - 64 (the 16-bit tiles: the twin's bands >= 2, `geo`
// in the twin's tile order with the band index counted from the body's first band).
// STAGED: every other call: widened into aligned fp32 scratch, the fp32 block push, rounded out -- in one piece up to 2^24 stream-ticks (128 MiB of
// scratch), else in chunks of max(64, (2^24 / streams) & ~63) ticks.
enum H16Route { H16_STAGED, H16_TILES };
constexpr size_t H16_STAGED_MAX = (size_t)1 << 24;
struct H16Plan {
    H16Route  route;
    BlockForm form;                  // TILES: the twin's form (MOMENT_TILES or DMA_TILES)
    size_t    head, body;            // TILES: 64 and ticks - 64
    size_t    chunk;                 // STAGED: ticks per fp32 block push (the last chunk takes what is left)
    TileGeom  geo;                   // TILES with body > 0: the body's tiles ...
    unsigned  grid;                  // ... and its grid
    int       wpb;
};
inline size_t h16_staged_chunk(size_t streams, size_t ticks)
{
    if (ticks <= H16_STAGED_MAX / streams) return ticks;                                // streams * ticks <= 2^24
    const size_t c = (H16_STAGED_MAX / streams) & ~(size_t)63;
    return c > 64 ? c : 64;
}
template <class Fit>
inline H16Plan block_plan_h16(int n, bool fma, size_t streams, size_t ticks, unsigned misaligned, bool centre, bool dma_switch, bool moment_switch,
                              Fit &&moment_terms)
{
    H16Plan plan = {};
    plan.route = H16_STAGED;
    plan.form = WALK;
    plan.chunk = h16_staged_chunk(streams, ticks);
    if (!tiles_take(streams, 128, misaligned, ticks, STREAM_DMA_MIN_TICKS)) return plan;
    const BlockForm form = block_form(n, fma, streams, ticks, 0u, centre, dma_switch, moment_switch, static_cast<Fit &&>(moment_terms));
    if (form != MOMENT_TILES && form != DMA_TILES) return plan;
    const DmaTileShape shape = dma_tile_shape(form, n, fma, streams);
    TileGeom whole;
    if (!tile_geom(streams, 128, ticks, 32, shape.group, shape.wpb, &whole)) return plan;   // the twin itself would leave the tiles
    plan.route = H16_TILES;
    plan.form = form;
    plan.head = STREAM_DMA_MIN_TICKS;
    plan.body = ticks - STREAM_DMA_MIN_TICKS;
    plan.chunk = 0;
    plan.wpb = shape.wpb;
    if (plan.body) plan.grid = tile_geom(streams, 128, plan.body, 32, shape.group, shape.wpb, &plan.geo);
    return plan;
}

// ---- the fused multi-output block push (savgol_streambank_push_block_multi): count banks, one read of the block.  Decided before anything is enqueued ----
// FUSED needs all of: count >= 2; every bank the same half window n and the same SAVGOL_STREAMBANK_FMA flag; n <= stream_multi_max_n(bank kind, outputs
// per launch); tiles_take(streams, 128, misaligned, ticks, 64) with `misaligned` or-ed over the samples, every output and every ring; ticks > 64; block_form
// answers DMA_TILES for every bank (tap by tap, not the block moments; both switches as sg_bank_roll_launch reads them); the twin's and the body's tile
// counts are indexed by 32 bits.  2 or 3 outputs are one launch, 4 are two launches of two (as savgol_apply_multi_batch_f32).  A fused call is, per bank,
// a head of 64 ticks through the bank's own fp32 tiles (sg_bank_roll_launch: the twin's bands 0 and 1, the only ones that read the ring since 2n <= 64),
// then the body's tiles of all outputs in `launches` launches (bands >= 2 of the twin's tile order), then per bank the tail store.
// SINGLE (launches == 0): everything else -- `count` single block pushes in the caller's order.
// Shipped bounds: 8 for both bank kinds and for 2 and 3 outputs per launch -- at every fused shape the call's median is 1.18-1.66 x ahead of the single
// calls on config 3's shape (profiles/stream_multi_time.txt); nothing above 8 has been measured.
constexpr int STREAM_MULTI_MAX_BANKS = 4;
constexpr int stream_multi_max_n(bool fma, int outputs) { return (outputs == 2 || outputs == 3) ? (fma ? 8 : 8) : 0; }   // (fused bank : bit-exact bank)
// (waves per block, ring pairs) of a multi-output launch: launch_bank_dma_shape's values for the half windows the call fuses -- the ring is per wave and
// shared by the outputs, the accumulators stay within 256 VGPRs (two waves per SIMD, what these block shapes hold anyway).  The swapped table
// -- (8, 12) for the light tiles, (4, 16) for the fused bank above n = 5 -- measured level, 0.97-1.02, interleaved in one process (EXPERIMENTS)
struct MultiTileShape { int wpb, dp; };
constexpr MultiTileShape multi_tile_shape(int n, bool fma, int /* outputs */) { return n > 5 && fma ? MultiTileShape{8, 12} : MultiTileShape{4, 16}; }
struct MultiBank { int n; bool fma, centre; };
struct MultiPlan {
    int      launches;               // 0 = `count` single calls
    int      per[2];                 // outputs of each launch, banks in the caller's order
    size_t   head, body;             // fused: 64 and ticks - 64
    TileGeom geo;                    // the body's tiles ...
    unsigned grid;                   // ... and their grid
    int      wpb, dp;
};
// The fused plan of both storages.  What differs comes as arguments: the bound table, the (waves per block, ring in DMAs) table, and the `misaligned`
// block_form is asked with (form_misaligned).  moment_terms(k): the host fit of bank k's taps, asked only where block_form asks
template <class MaxN, class Shape, class Fit>
inline MultiPlan block_plan_fused(const MultiBank *banks, int count, size_t streams, size_t ticks, unsigned misaligned, unsigned form_misaligned, bool dma_switch,
                                  bool moment_switch, Fit &&moment_terms, MaxN &&max_n, Shape &&tile_shape)
{
    MultiPlan plan = {};
    if (count < 2 || count > STREAM_MULTI_MAX_BANKS) return plan;
    const int per0 = count == 4 ? 2 : count;
    const int n = banks[0].n;
    const bool fma = banks[0].fma;
    for (int k = 1; k < count; ++k)
        if (banks[k].n != n || banks[k].fma != fma) return plan;
    if (n < 1 || n > max_n(fma, per0)) return plan;
    if (!tiles_take(streams, 128, misaligned, ticks, STREAM_DMA_MIN_TICKS) || ticks <= STREAM_DMA_MIN_TICKS) return plan;
    for (int k = 0; k < count; ++k)
        if (block_form(n, fma, streams, ticks, form_misaligned, banks[k].centre, dma_switch, moment_switch, [&] { return moment_terms(k); }) != DMA_TILES) return plan;
    const DmaTileShape twin = dma_tile_shape(DMA_TILES, n, fma, streams);
    TileGeom whole;
    if (!tile_geom(streams, 128, ticks, 32, twin.group, twin.wpb, &whole)) return plan;      // the twin itself would leave the tiles
    const MultiTileShape shape = tile_shape(n, fma, per0);
    plan.head = STREAM_DMA_MIN_TICKS;
    plan.body = ticks - STREAM_DMA_MIN_TICKS;
    plan.wpb = shape.wpb;
    plan.dp = shape.dp;
    plan.grid = tile_geom(streams, 128, plan.body, 32, twin.group, shape.wpb, &plan.geo);
    if (!plan.grid) return plan;
    plan.launches = count == 4 ? 2 : 1;
    plan.per[0] = per0;
    plan.per[1] = count == 4 ? 2 : 0;
    return plan;
}
// fp32 storage: block_form is asked with the call's own `misaligned` (the banks' heads run on the caller's buffers)
template <class Fit>
inline MultiPlan block_plan_multi(const MultiBank *banks, int count, size_t streams, size_t ticks, unsigned misaligned, bool dma_switch, bool moment_switch,
                                  Fit &&moment_terms)
{
    return block_plan_fused(banks, count, streams, ticks, misaligned, misaligned, dma_switch, moment_switch, static_cast<Fit &&>(moment_terms), stream_multi_max_n,
                            multi_tile_shape);
}

// ---- the fused multi-output block push on 16-bit storage (savgol_streambank_push_block_multi_h16).  Decided before anything is enqueued ----
// The conjunction of what block_plan_multi and block_plan_h16 demand.  FUSED needs all of: count >= 2; every bank the same half window n and the same
// SAVGOL_STREAMBANK_FMA flag; n <= stream_multi_h16_max_n(bank kind, outputs per launch); tiles_take(streams, 128, misaligned, ticks, 64) with
// `misaligned` or-ed over the 16-bit sample base, every output base and every ring; ticks > 64; block_form answers DMA_TILES for every bank's twin (the
// fp32 call on aligned buffers: tap by tap, not the block moments); the twin's and the body's tile counts are indexed by 32 bits.  2 or 3 outputs are one
// launch, 4 are two launches of two.  A fused call is a head of 64 ticks -- widened once into fp32 scratch, then per bank its own fp32 tiles on its own
// ring (the twin's bands 0 and 1) and the rounding of their rows --, the body's tiles of all outputs in `launches` launches (sg_stream_dma_multi_h16.hip:
// bands >= 2 of the twins' tile order), then per bank the tail store.
// SINGLE (launches == 0): everything else -- `count` single savgol_streambank_push_block_h16 calls in the caller's order.
// A table of its own, not stream_multi_max_n: the measurement may lower it per (bank kind, outputs per launch).  Shipped bounds: 8 for both bank
// kinds and for 2 and 3 outputs per launch -- at every fused shape the call's median is 1.12-1.52 x ahead of the single 16-bit calls on config 3's shape
// (profiles/stream_multi_h16_time.txt, part 1); nothing above 8 has been measured.
constexpr int stream_multi_h16_max_n(bool fma, int outputs) { return (outputs == 2 || outputs == 3) ? (fma ? 8 : 8) : 0; }   // (fused bank : bit-exact bank)
// (waves per block, ring ROWS) of a launch.  The starting table was multi_tile_shape's waves with the fp32 multi tile's ring depth in rows -- half the
// KiB, a DMA moves four 256-byte rows (as the single 16-bit tiles took launch_bank_dma_shape's): (4, 32), and (8, 24) for the fused bank
// above n = 5.  Interleaved with a second build in one process (profiles/stream_multi_h16_time.txt, second part), (4, 32) is ahead of (8, 24) outside
// the +- 3 % spread on 16 -> 16 bit for the fused bank with three outputs from n = 6 (1.05-1.21 x) and with two outputs from n = 7 (1.05-1.13 x) and
// level to 6 % behind on 16 bit -> fp32; at (fused bank, n = 6, two outputs) and on every light tile the starting table is level or ahead and stays.
struct MultiH16TileShape { int wpb, rows; };
constexpr MultiH16TileShape multi_h16_tile_shape(int n, bool fma, int outputs)
{
    return fma && n == 6 && outputs == 2 ? MultiH16TileShape{8, 24} : MultiH16TileShape{4, 32};
}
// the plan is block_plan_multi's struct; dp counts DMAs of four rows.  block_form is asked with 0: the twin runs on aligned scratch
template <class Fit>
inline MultiPlan block_plan_multi_h16(const MultiBank *banks, int count, size_t streams, size_t ticks, unsigned misaligned, bool dma_switch, bool moment_switch,
                                      Fit &&moment_terms)
{
    return block_plan_fused(banks, count, streams, ticks, misaligned, 0u, dma_switch, moment_switch, static_cast<Fit &&>(moment_terms), stream_multi_h16_max_n,
                            [](int n, bool fma, int outputs) { const MultiH16TileShape s = multi_h16_tile_shape(n, fma, outputs); return MultiTileShape{s.wpb, s.rows / 4}; });
}

// ---- the fused multi-output block push on int16 storage (savgol_streambank_push_block_multi_i16).  Decided before anything is enqueued ----
// block_plan_multi_h16's rule word for word (an int16 row is the same 256 bytes per 128 streams; the twin of bank k takes the single
// savgol_streambank_push_block_i16), with a bound table and a shape table of its own.  A fused call is a head of 64 ticks -- widened once into fp32
// scratch (i16_widen), then per bank its own fp32 tiles on its own ring and the conversion of their rows (i16_round) --, the body's tiles of all outputs in
// `launches` launches (sg_stream_dma_multi_i16.hip), then per bank the tail store.
// SINGLE (launches == 0): everything else -- `count` single savgol_streambank_push_block_i16 calls in the caller's order.
// Shipped bounds: the h16 table's, 8 for both bank kinds and for 2 and 3 outputs per launch; every tile compiles to the register step of its 16-bit float
// twin or a better one (tests/test_stream_multi_i16_host.py).  The shipping rule: a (bank kind, outputs, n) stays fused only where the fused call is not
// behind its single int16 calls by more than the +- 3 % placement spread -- at every fused shape the call's median is 1.09-1.53 x ahead of them on config
// 3's shape (profiles/stream_multi_i16_time.txt), so nothing was lowered; nothing above 8 has been measured.
constexpr int stream_multi_i16_max_n(bool fma, int outputs) { return (outputs == 2 || outputs == 3) ? (fma ? 8 : 8) : 0; }   // (fused bank : bit-exact bank)
// (waves per block, ring ROWS) of a launch: multi_h16_tile_shape's table, the rows are the same bytes
constexpr MultiH16TileShape multi_i16_tile_shape(int n, bool fma, int outputs)
{
    return fma && n == 6 && outputs == 2 ? MultiH16TileShape{8, 24} : MultiH16TileShape{4, 32};
}
template <class Fit>
inline MultiPlan block_plan_multi_i16(const MultiBank *banks, int count, size_t streams, size_t ticks, unsigned misaligned, bool dma_switch, bool moment_switch,
                                      Fit &&moment_terms)
{
    return block_plan_fused(banks, count, streams, ticks, misaligned, 0u, dma_switch, moment_switch, static_cast<Fit &&>(moment_terms), stream_multi_i16_max_n,
                            [](int n, bool fma, int outputs) { const MultiH16TileShape s = multi_i16_tile_shape(n, fma, outputs); return MultiTileShape{s.wpb, s.rows / 4}; });
}

}  // namespace sg
