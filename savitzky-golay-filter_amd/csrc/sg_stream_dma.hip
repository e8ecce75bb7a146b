// sg_stream_dma.hip -- savgol_streambank_push_block, LDS-DMA tile form (round 5).
//
// Reference loop: src/savgol_stream.c:25-38 (the ring dot product) driven by :152-178 (one push per sample) -- here `ticks` pushes of
// every stream in one launch, a convolution down the tick axis of samples[tick][stream].
//
// Why another form.  The walk (sg_bank_roll_kernel) keeps few rows in flight per wave; the register tiles (sg_bank_tile_kernel) load
// TR + 2n rows up front but hold them ALL in VGPRs until the last output is done (212 registers at n = 16: two waves per SIMD), and a
// wave that computes issues no memory traffic -- bare, that access pattern streams at 0.72-0.73 of 8 TB/s, with the arithmetic in it at
// 0.60-0.66 (tools/membench_streamtile.hip, profiles/r05_membench_streamtile.txt).  Here the rows never touch a VGPR on their way in:
//   * a wave owns 128 adjacent streams (a lane 2 = one 8-byte LDS read per row) x TR ticks and a private LDS slab of TR + 2n rows;
//   * it issues every row load up front as LDS-DMA (global_load_lds_dwordx4: 1 KiB = two 512-byte rows per instruction, no VGPR
//     destination), then consumes the rows IN ARRIVAL ORDER behind counted s_waitcnt vmcnt(k): each arriving row is read once from the
//     slab and fed into every accumulator it touches ("input stationary": row r is tap r - m of output m).  The arithmetic overlaps the
//     arrival of the later rows inside ONE wave, registers hold only the TR accumulators, and a finished output row is stored at once;
//   * per output the arithmetic is bank_roll_item's, bit for bit in both banks: reference order = one accumulator from 0, taps ascending,
//     multiply and add rounded separately (rows arrive in ascending tap order for every output); FMA = two chains (even / odd taps);
//   * tiles are dealt like the register tiles': blocks that share an XCD walk down a group of neighbouring strips band by band, so the 2n
//     halo rows a tile shares with the one above are L2 hits.
// Bare, this pattern streams at 0.75-0.76 (the flat copy on the same box: 0.79).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "sg_internal.h"
#include "sg_pk.hpp"
#include "sg_runtime.hpp"
#include "sg_stream_dma.hpp"
#include "sg_stream_roll.hpp"

namespace sg {

#ifndef SG_DMA_MAX_N
#define SG_DMA_MAX_N 32
#endif

template <int N, bool FMA, int TRT, int WPB, int DP, int FCH = 2, int MOM = 0, class TAPS = SRollTaps<N>>
__global__ __launch_bounds__(64 * WPB) void sg_bank_dma_kernel(const BankJob job, const TAPS taps, const TileGeom geo)
{
    typedef SRoll<N> R;
    typedef DmaShape<N, TRT> D;
    typedef DmaQueue<N, TRT, DP> Q;
    constexpr int TR = D::TR, NI = D::NI, RB = D::RB, RING = DP * 1024;
    static_assert(DP >= 2 && DP <= NI, "ring of row pairs");
    extern __shared__ __attribute__((aligned(1024))) char lds[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const TileAt at = tile_of(geo, xcd_block(job.aligned & 2) * WPB + (unsigned)wv);
    if (!at.ok) return;
    const unsigned band = at.band, strip = at.strip;
    const long long t0 = (long long)band * TR;
    const unsigned ring = (unsigned)(uintptr_t)((__attribute__((address_space(3))) char *)lds) + (unsigned)wv * (unsigned)RING;   // LDS byte address, wave-uniform
    const int sub = lane >> 5, chunk = lane & 31;                                                 // row of the pair, 16-byte chunk of the row
    const size_t col = (size_t)strip * 128 + (size_t)chunk * 4;

    f32x2 cen = f32x2{0.0f, 0.0f}, backdt = f32x2{0.0f, 0.0f};       // fused bank, derivative filters: what the tile's rows are centred on (set before the first row is fed)
    // source of row pair i: slab row r = history index t0 - 2N + r (history: ring contents, then this call's samples)
    const bool inside = t0 >= 2 * N && t0 + TR <= (long long)job.ticks;                           // uniform: every row is one of this call's samples
    const float *const p0 = job.samples + (size_t)(inside ? t0 - 2 * N + sub : 0) * job.streams + col;
    const size_t pstep = 2 * job.streams;
    auto issue = [&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const float *src;
        if (inside) {
            src = p0 + (size_t)i * pstep;
        } else {
            src = history_row<R::WS>(job, t0 - 2 * N + 2 * i + sub) + col;
        }
        dma16(src, ring + (unsigned)(i % DP) * 1024u);
    };
    static_for<DP>([&](auto ic) -> bool { issue(ic); return true; });

    // ---- consume the rows in arrival order ----
    const char *mine = lds + (size_t)wv * RING + lane * 8;
    const int row_bytes = (int)(job.streams * 4);
    const unsigned voff = (strip * 128u + 2u * (unsigned)lane) * 4u;                              // byte offset of this lane's streams in a row
    constexpr int CH = MOM ? 1 : (FMA ? FCH : 1);                                                 // FMA bank: two chains (even / odd taps) or one; block moments: one (an output is ~14 terms)
    f32x2 acc[CH][TR];
    f32x2 mom[MOM > 0 ? MOM : 1];                                                                 // block moments of the block being filled (MOM > 0)
    auto row_in = [&](auto rc) -> f32x2 {
        constexpr int r = decltype(rc)::value;
        return *reinterpret_cast<const f32x2 *>(mine + ((r / 2) % DP) * 1024 + (r & 1) * RB);
    };
    auto feed = [&](auto rc, const f32x2 x) {
        constexpr int r = decltype(rc)::value;
#include "sg_stream_dma_feed.hpp"
        if constexpr (r >= 2 * N && r - 2 * N < TR) {                                             // output m = r - 2N has seen its last row
            constexpr int m = r - 2 * N;
            f32x2 a = acc[0][m];
            if constexpr (CH == 2) a = a + acc[1][m];

            const long long tt = t0 + m;
            const bool has_out = tt < (long long)job.ticks && has_output<R::WS>(job, (unsigned long long)tt);                          // uniform
            // fused bank: (a + c * sum_k w_k) * dt_inv in one multiply-add (backdt = c * sum_k w_k * dt_inv, zero unless the tile is centred)
            const f32x2 y = (MOM > 0 || FMA) ? __builtin_elementwise_fma(a, f32x2{job.dt_inv, job.dt_inv}, backdt) : a * f32x2{job.dt_inv, job.dt_inv};
            float *orow = job.out + (size_t)(tt < (long long)job.ticks ? tt : 0) * job.streams;
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(orow, 0, has_out ? row_bytes : 0, 0x00020000);
            // cache policy 2 = nontemporal: written once, never read by this launch (0.392 against 0.412 ms on one box, profiles/r05_stream_dma.txt;
            // nontemporal row LOADS lose 30 %: the halo rows are re-read)
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, y), rs, (int)voff, 0, 2);
        }
    };
    // Step g consumes pair g (already in xa, xb), after it has waited for pair g + 1 and issued its LDS reads (their latency hides behind
    // the arithmetic), and ends by issuing DMA g + DP into the ring slot pair g has just left.  A row without an output still issues its
    // store (into an empty descriptor), so the queue arithmetic above is static.
    // ---- fused bank, derivative filters (job.centre): c = the mean of EIGHT real samples of each stream (a single sample of a zero-mean stream would
    // double what the sums meet).  A tile whose rows are all real takes its first eight rows out of LDS once their four DMA pairs have landed -- no
    // memory request of its own: eight extra 8-byte loads per lane and tile cost config 3 12 % (the kernel lives on its request rate); the few tiles of
    // a bank's first 2N ticks (rows before the first sample: the ring's zeros, feeding only outputs that are not stored) load eight samples spread
    // from the oldest real one to the tile's last row.
    if constexpr (MOM > 0 || FMA) {
        static_assert(DP >= 4 && NI >= 4, "the first four row pairs are in the ring together");
        if (job.centre) {                                    // uniform; smoothing filters keep cen = 0
            f32x2 sum = f32x2{0.0f, 0.0f};
            if (t0 - 2 * N >= -(long long)job.received0) {   // uniform: row 0 is a real sample, and so are the rows behind it
                wait_vm<(Q::younger(3, 0) > 63 ? 63 : Q::younger(3, 0))>();
                static_for<8>([&](auto rc) -> bool { sum = sum + row_in(rc); return true; });
            } else {
                sum = spread_centre<R::WS>(job, t0 - 2 * N, t0 + TR - 1, [&](const float *row) -> f32x2 {
                    return *reinterpret_cast<const f32x2 *>(row + (size_t)strip * 128 + 2 * (size_t)lane);
                });
            }
            cen = centre_guard(sum);
            backdt = cen * f32x2{job.centre_sum * job.dt_inv, job.centre_sum * job.dt_inv};
        }
    }
    wait_vm<(Q::younger(0, 0) > 63 ? 63 : Q::younger(0, 0))>();           // (a smaller count only waits longer: the counter has 6 bits)
    f32x2 xa = row_in(std::integral_constant<int, 0>{}), xb = row_in(std::integral_constant<int, 1>{});
    // The fused bank's tiles -- block moments and tap-by-tap alike, never the bit-exact bank -- run on CENTRED samples (end of round 6, R6.16): sum_k w_k x_k = sum_k w_k (x_k - c) + c sum_k w_k for any c; with c = the stream's own
    // first row of the tile the moments and their block offsets meet the signal's variation over 2N + TR ticks instead of its offset -- a derivative
    // filter (weights summing to ~0: config 3) on a stream riding on a large offset stood at 2.3 x the reference's own error, the blocks' shares
    // cancelling only after each had been rounded at the offset's size.  sum_k w_k comes from the reference's table (taps.sig).
    static_for<NI>([&](auto gc) -> bool {
        constexpr int g = decltype(gc)::value;
        f32x2 na = xa, nb = xb;
        if constexpr (g + 1 < NI) {
            wait_vm<(Q::younger(g + 1, g) > 63 ? 63 : Q::younger(g + 1, g))>();
            na = row_in(std::integral_constant<int, 2 * g + 2>{});
            nb = row_in(std::integral_constant<int, 2 * g + 3>{});
            __builtin_amdgcn_sched_barrier(0);                                                    // keep these reads AHEAD of pair g's arithmetic (left alone, hipcc sinks them to their use)
        }
        if constexpr (MOM > 0 || FMA) {
            feed(std::integral_constant<int, 2 * g>{}, xa - cen);
            feed(std::integral_constant<int, 2 * g + 1>{}, xb - cen);
        } else {
            feed(std::integral_constant<int, 2 * g>{}, xa);
            feed(std::integral_constant<int, 2 * g + 1>{}, xb);
        }
        if constexpr (g + DP < NI) {
            // pair g's slot is free: its two LDS reads were issued a step ago and their data has just been consumed -- but "consumed" is the
            // compiler's business, so drain the LDS queue explicitly before the DMA may overwrite the slot
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            issue(std::integral_constant<int, g + DP>{});
        }
        xa = na; xb = nb;
        return true;
    });
}

// One launch of LDS-DMA tiles (TRT ticks, WPB waves per block, a ring of DP row pairs per wave; group strips per group); 1 = not covered: more tiles
// than 32 bits index, or a launch the runtime refused -- the caller goes on to the next form
template <int TRT, int WPB, int DP, class Kernel, class Taps>
static int launch_dma_tiles(Kernel kernel, unsigned group, BankJob job, const Taps &taps, hipStream_t st)
{
    TileGeom geo;
    const unsigned grid = tile_geom(job.streams, 128, job.ticks, TRT, group, WPB, &geo);
    if (!grid) return 1;
    job.aligned = 1;
    constexpr size_t lds = (size_t)WPB * DP * 1024;
    static_assert(lds <= 160 * 1024, "slabs of one block must fit the CU's LDS");
    // more than 64 KiB of dynamic LDS needs the attribute, and the attribute belongs to the (function, DEVICE) pair: set per launch -- a process-wide
    // static applied it on whichever device launched first only (a block push is >= 0.1 ms, the call is host-side bookkeeping)
    if (lds > 65536 && hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
        (void)hipGetLastError();
        return 1;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * WPB), lds, st, job, taps, geo);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

#ifndef SG_DMA_MOM_BUILD
template <int N, bool FMA, int TRT, int WPB, int DPR, int FCH = 2>
static int launch_bank_dma(const float *center, const BankJob &job, hipStream_t st)
{
    SRollTaps<N> taps;
    memset(&taps, 0, sizeof(taps));
    pack_taps(center, SRoll<N>::WS, taps.w);
    constexpr int DP = DPR < DmaShape<N, TRT>::NI ? DPR : DmaShape<N, TRT>::NI;                   // ring of row pairs (all of the tile's pairs: every load up front)
    return launch_dma_tiles<TRT, WPB, DP>(sg_bank_dma_kernel<N, FMA, TRT, WPB, DP, FCH>, 128u, job, taps, st);      // groups of 128 strips: 64 KiB of a tick row
}

template <int N, bool FMA>
static int launch_bank_dma_shape(const float *center, const BankJob &job, hipStream_t st)
{
    // (waves per block, ring pairs) by half window and bank -- interleaved A/B on config 3's shape (profiles/r05_stream_shapes_ab.txt): light tiles run
    // best on fewer, deeper waves -- fused bank n = 8: (8, 12) 0.387 against (4, 12) 0.414 ms; bit-exact bank n = 8: (4, 16) 0.364 against 0.387.  The whole
    // library before / after this table, both banks: n = 4 / 6 / 8 2.5-6.5 % faster, fused n = 11 8.6 %, n = 2 and 10 level; the bit-exact bank from n = 11
    // (66 instructions per output pair at n = 16) keeps (4, 12): (8, 8) and (4, 16) measured 1-3 % slower there
    if constexpr (N <= 5) return launch_bank_dma<N, FMA, 32, 4, 16>(center, job, st);
    else if constexpr (N <= 11 && FMA) return launch_bank_dma<N, FMA, 32, 8, 12>(center, job, st);
    else if constexpr (N <= 10) return launch_bank_dma<N, FMA, 32, 4, 16>(center, job, st);
    // every other tile: 32 ticks, 4 waves per block (only how waves are dealt to CUs and how LDS is carved), 12 row pairs (KiB) of LDS ring per wave =
    // how far the row loads run ahead of the arithmetic (A/B'd on config 3's shape, profiles/r05_stream_dma.txt -- 8 / 12 / 16 / 24 pairs: FMA bank
    // 0.401 / 0.401 / 0.405 / 0.479 ms, bit-exact bank sustained 0.551 / 0.545-0.555 / 0.579-0.592 / 0.710 on one box: a shallow ring leaves LDS for
    // the waves the bit-exact arithmetic needs)
    return launch_bank_dma<N, FMA, 32, 4, 12>(center, job, st);
}

template <int N>
static int dispatch_bank_dma(int n, int fma, const float *center, const BankJob &job, hipStream_t st)
{
    if (n == N) return fma ? launch_bank_dma_shape<N, true>(center, job, st) : launch_bank_dma_shape<N, false>(center, job, st);
    if constexpr (N < SG_DMA_MAX_N) return dispatch_bank_dma<N + 1>(n, fma, center, job, st);
    else return 1;
}

#ifndef SG_DMA_MIN_N
#define SG_DMA_MIN_N 1
#endif
#ifndef SG_DMA_FN
#define SG_DMA_FN sg_bank_dma_launch_all                     // the Makefile builds two objects (half windows 1..16 and 17..32) with a symbol each
#endif

// 0 = launched; 1 = not covered (launch_dma_tiles), or a half window outside [SG_DMA_MIN_N, SG_DMA_MAX_N].  The call's shape is block_form's business.
int SG_DMA_FN(int n, int fma, const float *center, const BankJob &job, hipStream_t st)
{
    if (n < SG_DMA_MIN_N || n > SG_DMA_MAX_N) return 1;
    return dispatch_bank_dma<SG_DMA_MIN_N>(n, fma, center, job, st);
}

#else      // SG_DMA_MOM_BUILD: the third object, block-moment tiles of the fused bank
template <int N, int M>
static int launch_bank_dma_mom(const StreamMomentFit &fit, const float *center, const BankJob &job, hipStream_t st)
{
    // tiles of 32 ticks, (waves per block, ring pairs) = (8, 16): with a third of the arithmetic gone the block-moment tiles want FEWER resident
    // waves with deeper rings -- 8 waves per CU, 16 KiB in flight each (R5.9)
    constexpr int TRT = 32, WPB = 8, DPR = 16;
    MomTaps<N, M> taps;
    pack_mom_taps(fit, center, &taps);
    // strips per group: 32 KiB of a tick row (64 strips), a quarter of the row for narrow banks.  Measured over FRESH ALLOCATIONS inside one process
    // (tools/placement_stream.py, profiles/r05_placement_stream.txt): with 128-strip groups config 3's launch is 0.363-0.370 ms on most placements of the
    // two buffers and 0.405-0.414 on the rest (3 of 12 to 7 of 12 from call to call); with 64-strip groups 0.373-0.397 on all of them -- the same mean, a
    // third of the spread; 32 768 / 131 072 streams: 0.367 / 0.389 against 0.383 / 0.418; 16 384 streams: 32-strip groups 0.362 against 0.374.  Group sizes
    // that do not divide an XCD's eighth of the tile order (48, 80, 96) cost 10-18 %.  (The tap-by-tap tiles keep 128: the bit-exact bank is 5 % slower on 64.)
    const unsigned want = (unsigned)(job.streams / 128 / 4);
    constexpr int DP = DPR < DmaShape<N, TRT>::NI ? DPR : DmaShape<N, TRT>::NI;
    return launch_dma_tiles<TRT, WPB, DP>(sg_bank_dma_kernel<N, true, TRT, WPB, DP, 1, M, MomTaps<N, M>>, want < 16u ? 16u : (want > 64u ? 64u : want), job, taps, st);
}

template <int N>
static int dispatch_bank_dma_mom(int n, const StreamMomentFit &fit, const float *center, const BankJob &job, hipStream_t st)
{
    if (n == N) {
        if (fit.terms == 1) return launch_bank_dma_mom<N, 1>(fit, center, job, st);
        if (fit.terms == 2) return launch_bank_dma_mom<N, 2>(fit, center, job, st);
        return launch_bank_dma_mom<N, 3>(fit, center, job, st);
    }
    if constexpr (N < STREAM_MOMENT_MAX_N) return dispatch_bank_dma_mom<N + 1>(n, fit, center, job, st);
    else return 1;
}

// 0 = launched; 1 = not covered (launch_dma_tiles), or a half window outside 12..20.  `fit`: the host fit of the bank's taps (block_form asked for it)
int sg_bank_dma_launch_mom(int n, const StreamMomentFit &fit, const float *center, const BankJob &job, hipStream_t st)
{
    if (n < STREAM_MOMENT_MIN_N || n > STREAM_MOMENT_MAX_N) return 1;
    return dispatch_bank_dma_mom<STREAM_MOMENT_MIN_N>(n, fit, center, job, st);
}

#endif

}  // namespace sg
