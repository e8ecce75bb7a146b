// sg_stream_dma_i16.hip -- savgol_streambank_push_block_i16, the body of the tile route: LDS-DMA tiles on int16 rows.
//
// sg_stream_dma_h16.hip with the body tile's other storage: the fragment (sg_stream_dma_body.inc, K = 1) is included with SG_BODY_I16 set, so a lane's
// dword widens through the exact sign-extending convert and an int16 output row is rounded, saturated and packed once (sg_i16.hpp); everything else --
// the DMA queue, the feed, the centre, the one store per output row -- is the text the 16-bit float kernels compile.  The same three objects (half
// windows 1..16, 17..32, the fused bank's block-moment form), the same (waves per block, ring) table, the same job (BankJobH16: its samples are 16-bit
// words either way; out_type SAVGOL_HIP_I16 or _F32, wave-uniform) and the h16 launchers' signatures.  Only bands >= 2 of a call come here
// (block_plan_h16, sg_stream_host.hpp).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "sg_i16.hpp"
#include "sg_internal.h"
#include "sg_pk.hpp"
#include "sg_runtime.hpp"
#include "sg_stream_dma.hpp"
#include "sg_stream_dma_body.hpp"
#include "sg_stream_i16.hpp"
#include "sg_stream_roll.hpp"

namespace sg {

#ifndef SG_DMA_MAX_N
#define SG_DMA_MAX_N 32
#endif

// Waves per SIMD the registers are allocated for.  The block-moment tiles up to half window 15 are held to five, the step their 16-bit float twins
// compile to (at most 96 VGPRs); left alone, the three-moment tile at n = 15 comes out at 98.  Every other tile keeps what a block of WPB waves
// implies by itself, so its code is what it is without the second argument.
constexpr int i16_tile_min_waves(int n, int mom, int wpb) { return mom > 0 && n <= 15 ? 5 : (wpb + 3) / 4; }

// DP: the ring, in DMAs = KiB = four rows each
template <int N, bool FMA, int TRT, int WPB, int DP, int FCH = 2, int MOM = 0, class TAPS = SRollTaps<N>>
__global__ __launch_bounds__(64 * WPB, i16_tile_min_waves(N, MOM, WPB)) void sg_bank_dma_i16_kernel(const BankJobH16 job, const TAPS all, const TileGeom geo)
{
    constexpr int K = 1;
#define SG_BODY_I16
#include "sg_stream_dma_body.inc"
#undef SG_BODY_I16
}

#ifndef SG_DMA_MOM_BUILD
template <int N, bool FMA, int WPB, int DPQ>
static int launch_bank_dma_i16(const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    SRollTaps<N> taps;
    memset(&taps, 0, sizeof(taps));
    pack_taps(center, SRoll<N>::WS, taps.w);
    constexpr int NI = DmaQueue<N, 32, DPQ, 4>::NI, DP = DPQ < NI ? DPQ : NI;            // ring of row quads, clamped to the tile
    return launch_body_tiles<WPB, DP>(sg_bank_dma_i16_kernel<N, FMA, 32, WPB, DP>, job, taps, geo, grid, st);
}

// (waves per block, ring) by half window and bank: launch_bank_dma_h16_shape's table (the rows are the same bytes)
template <int N, bool FMA>
static int launch_bank_dma_i16_shape(const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    if constexpr (N <= 5) return launch_bank_dma_i16<N, FMA, 4, 8>(center, job, geo, grid, st);
    else if constexpr (N <= 11 && FMA) return launch_bank_dma_i16<N, FMA, 8, 6>(center, job, geo, grid, st);
    else if constexpr (N <= 10) return launch_bank_dma_i16<N, FMA, 4, 8>(center, job, geo, grid, st);
    return launch_bank_dma_i16<N, FMA, 4, 6>(center, job, geo, grid, st);
}

template <int N>
static int dispatch_bank_dma_i16(int n, int fma, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    if (n == N) return fma ? launch_bank_dma_i16_shape<N, true>(center, job, geo, grid, st) : launch_bank_dma_i16_shape<N, false>(center, job, geo, grid, st);
    if constexpr (N < SG_DMA_MAX_N) return dispatch_bank_dma_i16<N + 1>(n, fma, center, job, geo, grid, st);
    else return 1;
}

#ifndef SG_DMA_MIN_N
#define SG_DMA_MIN_N 1
#endif
#ifndef SG_DMA_FN
#define SG_DMA_FN sg_bank_dma_i16_launch_all                 // the Makefile builds two objects (half windows 1..16 and 17..32) with a symbol each
#endif

int SG_DMA_FN(int n, int fma, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    if (n < SG_DMA_MIN_N || n > SG_DMA_MAX_N) return 1;
    return dispatch_bank_dma_i16<SG_DMA_MIN_N>(n, fma, center, job, geo, grid, st);
}

#else      // SG_DMA_MOM_BUILD: the third object, block-moment tiles of the fused bank
template <int N, int M>
static int launch_bank_dma_i16_mom(const StreamMomentFit &fit, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    constexpr int WPB = 8, DPQ = 8;                          // launch_bank_dma_h16_mom's
    MomTaps<N, M> taps;
    pack_mom_taps(fit, center, &taps);
    constexpr int NI = DmaQueue<N, 32, DPQ, 4>::NI, DP = DPQ < NI ? DPQ : NI;            // ring of row quads, clamped to the tile
    return launch_body_tiles<WPB, DP>(sg_bank_dma_i16_kernel<N, true, 32, WPB, DP, 1, M, MomTaps<N, M>>, job, taps, geo, grid, st);
}

template <int N>
static int dispatch_bank_dma_i16_mom(int n, const StreamMomentFit &fit, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    if (n == N) {
        if (fit.terms == 1) return launch_bank_dma_i16_mom<N, 1>(fit, center, job, geo, grid, st);
        if (fit.terms == 2) return launch_bank_dma_i16_mom<N, 2>(fit, center, job, geo, grid, st);
        return launch_bank_dma_i16_mom<N, 3>(fit, center, job, geo, grid, st);
    }
    if constexpr (N < STREAM_MOMENT_MAX_N) return dispatch_bank_dma_i16_mom<N + 1>(n, fit, center, job, geo, grid, st);
    else return 1;
}

int sg_bank_dma_i16_launch_mom(int n, const StreamMomentFit &fit, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st)
{
    if (n < STREAM_MOMENT_MIN_N || n > STREAM_MOMENT_MAX_N) return 1;
    return dispatch_bank_dma_i16_mom<STREAM_MOMENT_MIN_N>(n, fit, center, job, geo, grid, st);
}

#endif

}  // namespace sg
