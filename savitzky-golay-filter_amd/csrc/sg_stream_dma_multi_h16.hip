// sg_stream_dma_multi_h16.hip -- savgol_streambank_push_block_multi_h16, the body of a fused call: LDS-DMA tiles on fp16 / bf16 rows with K outputs from
// one read of the samples.
//
// The kernel is the body tile (sg_stream_dma_body.inc) with K = 2 or 3 outputs: the samples cross HBM -> LDS once for K banks, 2 + 2 K bytes per
// stream-tick (16 -> 16 bit) instead of 4 K, 2 + 4 K (16 bit -> fp32) instead of 6 K.  This file holds what is the fused call's own: the K tap tables,
// the shape table as template arguments and the dispatch by half window and output count, one object per bank kind.  Only bands >= 2 of a call come
// here (block_plan_multi_h16, sg_stream_host.hpp).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "sg_h16.hpp"
#include "sg_internal.h"
#include "sg_pk.hpp"
#include "sg_runtime.hpp"
#include "sg_stream_dma.hpp"
#include "sg_stream_dma_body.hpp"
#include "sg_stream_multi_h16.hpp"
#include "sg_stream_roll.hpp"

namespace sg {

#ifndef SG_MULTI_H16_FMA
#define SG_MULTI_H16_FMA 1
#endif

// DP: the ring, in DMAs = KiB = four rows each
template <int N, bool FMA, int K, int TRT, int WPB, int DP, int FCH = 2>
__global__ __launch_bounds__(64 * WPB) void sg_bank_dma_multi_h16_kernel(const BankJobMultiH16 job, const MultiH16Taps<N, K> all, const TileGeom geo)
{
    static_assert(K >= 2 && K <= STREAM_MULTI_PER_LAUNCH, "outputs per launch; one output is sg_bank_dma_h16_kernel");
    constexpr int MOM = 0;
#include "sg_stream_dma_body.inc"
}

// One launch of the body's tiles for K outputs; 1 = the runtime refused it
template <int N, bool FMA, int K, int WPB, int DPQ>
static int launch_bank_dma_multi_h16(const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st)
{
    constexpr int NI = DmaQueue<N, 32, DPQ, 4>::NI, DP = DPQ < NI ? DPQ : NI;                     // ring of row quads, clamped to the tile
    if (plan.wpb != WPB) return 1;                                                                // the grid was laid out for another block shape
    MultiH16Taps<N, K> taps;
    memset(&taps, 0, sizeof(taps));
    for (int k = 0; k < K; ++k) pack_taps(center[k], SRoll<N>::WS, taps.t[k].w);
    return launch_body_tiles<WPB, DP>(sg_bank_dma_multi_h16_kernel<N, FMA, K, 32, WPB, DP>, job, taps, plan.geo, plan.grid, st);
}

// (waves per block, ring rows) by half window, bank and output count: multi_h16_tile_shape (sg_stream_host.hpp) as template arguments
template <int N, bool FMA, int K>
static int launch_bank_dma_multi_h16_shape(const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st)
{
    constexpr MultiH16TileShape s = multi_h16_tile_shape(N, FMA, K);
    static_assert(s.rows % 4 == 0, "a DMA moves four rows");
    return launch_bank_dma_multi_h16<N, FMA, K, s.wpb, s.rows / 4>(center, job, plan, st);
}

template <int N, bool FMA>
static int dispatch_bank_dma_multi_h16(int n, int outputs, const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st)
{
    if (n == N) {
        if constexpr (N <= stream_multi_h16_max_n(FMA, 2)) { if (outputs == 2) return launch_bank_dma_multi_h16_shape<N, FMA, 2>(center, job, plan, st); }
        if constexpr (N <= stream_multi_h16_max_n(FMA, 3)) { if (outputs == 3) return launch_bank_dma_multi_h16_shape<N, FMA, 3>(center, job, plan, st); }
        return 1;
    }
    constexpr int top = stream_multi_h16_max_n(FMA, 2) > stream_multi_h16_max_n(FMA, 3) ? stream_multi_h16_max_n(FMA, 2) : stream_multi_h16_max_n(FMA, 3);
    if constexpr (N < top) return dispatch_bank_dma_multi_h16<N + 1, FMA>(n, outputs, center, job, plan, st);
    else return 1;
}

// the Makefile builds two objects, one per bank kind, so that they compile side by side
#if SG_MULTI_H16_FMA
int sg_bank_dma_multi_h16_launch_fma(int n, int outputs, const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st)
{
    return n < 1 ? 1 : dispatch_bank_dma_multi_h16<1, true>(n, outputs, center, job, plan, st);
}
#else
int sg_bank_dma_multi_h16_launch_ref(int n, int outputs, const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st)
{
    return n < 1 ? 1 : dispatch_bank_dma_multi_h16<1, false>(n, outputs, center, job, plan, st);
}
#endif

}  // namespace sg
