// sg_stream_dma_st16.hip -- savgol_streambank_push_block_h16 and savgol_streambank_push_block_i16, the body of the tile route: LDS-DMA tiles on 16-bit
// rows.  Compiled once per (storage family, object) by the Makefile: -DSG_FAMILY=h16 (fp16 / bf16 rows) or i16 (int16 rows), and per family three
// objects -- half windows 1..16 and 17..32, tap by tap in both banks, and the fused bank's block-moment form.
//
// The kernel, sg_bank_dma_h16_kernel or sg_bank_dma_i16_kernel, is the body tile (sg_stream_dma_body.inc) with one output.  What the families differ in
// is their policy (StreamFamily, sg_stream_st16.hpp): the converts at the widen and at the store, the order of the two stores and the waves per SIMD
// the registers are allocated for; the DMA queue, the feed, the centre, the one store per output row, the job (BankJobH16: 16-bit words either way)
// and everything in this file -- the tap tables, the (waves per block, ring) table, the dispatch by half window -- are one text.  Only bands >= 2 of a
// call come here (block_plan_h16, sg_stream_host.hpp).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "sg_internal.h"
#include "sg_pk.hpp"
#include "sg_runtime.hpp"
#include "sg_stream_dma.hpp"
#include "sg_stream_dma_body.hpp"
#include "sg_stream_roll.hpp"
#include "sg_stream_st16.hpp"

#if !defined(SG_FAMILY) || !(defined(SG_DMA_MOM_BUILD) || (defined(SG_DMA_MIN_N) && defined(SG_DMA_MAX_N) && defined(SG_DMA_FN)))
#error "compile with -DSG_FAMILY=h16|i16 and -DSG_DMA_MIN_N=.. -DSG_DMA_MAX_N=.. -DSG_DMA_FN=symbol, or -DSG_DMA_MOM_BUILD"
#endif

namespace sg {

// DP: the ring, in DMAs = KiB = four rows each
template <int N, bool FMA, int TRT, int WPB, int DP, int FCH = 2, int MOM = 0, class TAPS = SRollTaps<N>>
__global__ __launch_bounds__(64 * WPB, StreamFamily::tile_min_waves(N, MOM, WPB)) void SG_FAMILY_NAME(sg_bank_dma_, _kernel)(const BankJobH16 job, const TAPS all, const TileGeom geo)
{
    typedef StreamFamily F;
    constexpr int K = 1;
#include "sg_stream_dma_body.inc"
}

// one launch of the body's tiles with the ring of DPQ row quads clamped to the tile; 1 = the runtime refused it
template <int N, bool FMA, int WPB, int DPQ, int FCH = 2, int MOM = 0, class TAPS>
static int launch_bank_dma_st16(const TAPS &taps, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    constexpr int NI = DmaQueue<N, 32, DPQ, 4>::NI, DP = DPQ < NI ? DPQ : NI;
    return launch_body_tiles<WPB, DP>(SG_FAMILY_NAME(sg_bank_dma_, _kernel)<N, FMA, 32, WPB, DP, FCH, MOM, TAPS>, job, taps, geo, grid, st);
}

#ifndef SG_DMA_MOM_BUILD
// (waves per block, ring) by half window and bank: launch_bank_dma_shape's table (dma_tile_shape, sg_stream_host.hpp, restates the waves), the ring as
// deep in ROWS as the fp32 tiles' -- half the KiB
template <int N, bool FMA>
static int launch_bank_dma_st16_shape(const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    SRollTaps<N> taps;
    memset(&taps, 0, sizeof(taps));
    pack_taps(center, SRoll<N>::WS, taps.w);
    if constexpr (N <= 5) return launch_bank_dma_st16<N, FMA, 4, 8>(taps, job, geo, grid, st);
    else if constexpr (N <= 11 && FMA) return launch_bank_dma_st16<N, FMA, 8, 6>(taps, job, geo, grid, st);
    else if constexpr (N <= 10) return launch_bank_dma_st16<N, FMA, 4, 8>(taps, job, geo, grid, st);
    return launch_bank_dma_st16<N, FMA, 4, 6>(taps, job, geo, grid, st);
}

template <int N>
static int dispatch_bank_dma_st16(int n, int fma, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    if (n == N) return fma ? launch_bank_dma_st16_shape<N, true>(center, job, geo, grid, st) : launch_bank_dma_st16_shape<N, false>(center, job, geo, grid, st);
    if constexpr (N < SG_DMA_MAX_N) return dispatch_bank_dma_st16<N + 1>(n, fma, center, job, geo, grid, st);
    else return 1;
}

// the Makefile builds two objects per family (half windows 1..16 and 17..32) with a symbol each
int SG_DMA_FN(int n, int fma, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    if (n < SG_DMA_MIN_N || n > SG_DMA_MAX_N) return 1;
    return dispatch_bank_dma_st16<SG_DMA_MIN_N>(n, fma, center, job, geo, grid, st);
}

#else      // SG_DMA_MOM_BUILD: the third object, block-moment tiles of the fused bank
template <int N, int M>
static int launch_bank_dma_st16_mom(const StreamMomentFit &fit, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    MomTaps<N, M> taps;
    pack_mom_taps(fit, center, &taps);
    return launch_bank_dma_st16<N, true, 8, 8, 1, M>(taps, job, geo, grid, st);          // launch_bank_dma_mom's (8, 16 KiB): the same rows in flight
}

template <int N>
static int dispatch_bank_dma_st16_mom(int n, const StreamMomentFit &fit, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    if (n == N) {
        if (fit.terms == 1) return launch_bank_dma_st16_mom<N, 1>(fit, center, job, geo, grid, st);
        if (fit.terms == 2) return launch_bank_dma_st16_mom<N, 2>(fit, center, job, geo, grid, st);
        return launch_bank_dma_st16_mom<N, 3>(fit, center, job, geo, grid, st);
    }
    if constexpr (N < STREAM_MOMENT_MAX_N) return dispatch_bank_dma_st16_mom<N + 1>(n, fit, center, job, geo, grid, st);
    else return 1;
}

int SG_FAMILY_NAME(sg_bank_dma_, _launch_mom)(int n, const StreamMomentFit &fit, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    if (n < STREAM_MOMENT_MIN_N || n > STREAM_MOMENT_MAX_N) return 1;
    return dispatch_bank_dma_st16_mom<STREAM_MOMENT_MIN_N>(n, fit, center, job, geo, grid, st);
}

#endif

}  // namespace sg
