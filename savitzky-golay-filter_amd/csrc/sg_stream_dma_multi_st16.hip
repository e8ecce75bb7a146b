// sg_stream_dma_multi_st16.hip -- savgol_streambank_push_block_multi_h16 and savgol_streambank_push_block_multi_i16, the body of a fused call: LDS-DMA
// tiles on 16-bit rows with K outputs from one read of the samples.  Compiled once per (storage family, bank kind) by the Makefile: -DSG_FAMILY=h16
// (fp16 / bf16 rows) or i16 (int16 rows), -DSG_MULTI_ST16_FMA=1 (the fused bank) or 0 (the bit-exact bank).
//
// The kernel, sg_bank_dma_multi_h16_kernel or sg_bank_dma_multi_i16_kernel, is the body tile (sg_stream_dma_body.inc) with K = 2 or 3 outputs: the
// samples cross HBM -> LDS once for K banks, 2 + 2 K bytes per stream-tick (16 -> 16 bit) instead of 4 K, 2 + 4 K (16 bit -> fp32) instead of 6 K; a
// lane's dword widens ONCE per row for every output and an output row is narrowed once per output.  What the families differ in is their policy
// (StreamFamily, sg_stream_st16.hpp): the converts, the order of the two stores, the waves per SIMD the registers are allocated for, and the bound and
// shape tables the dispatch reads; the job (BankJobMultiH16: 16-bit words either way) and everything in this file -- the K tap tables, the shape table
// as template arguments, the dispatch by half window and output count -- are one text.  Only bands >= 2 of a call come here (block_plan_multi_h16,
// block_plan_multi_i16, sg_stream_host.hpp).
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

#if !defined(SG_FAMILY) || !defined(SG_MULTI_ST16_FMA)
#error "compile with -DSG_FAMILY=h16|i16 -DSG_MULTI_ST16_FMA=1|0"
#endif

namespace sg {

// DP: the ring, in DMAs = KiB = four rows each
template <int N, bool FMA, int K, int TRT, int WPB, int DP, int FCH = 2>
__global__ __launch_bounds__(64 * WPB, StreamFamily::multi_tile_min_waves(N, FMA, K, WPB)) void SG_FAMILY_NAME(sg_bank_dma_multi_, _kernel)(const BankJobMultiH16 job, const MultiH16Taps<N, K> all, const TileGeom geo)
{
    static_assert(K >= 2 && K <= STREAM_MULTI_PER_LAUNCH, "outputs per launch; one output is sg_stream_dma_st16.hip's kernel");
    typedef StreamFamily F;
    constexpr int MOM = 0;
#include "sg_stream_dma_body.inc"
}

// One launch of the body's tiles for K outputs; 1 = the runtime refused it
template <int N, bool FMA, int K, int WPB, int DPQ>
static int launch_bank_dma_multi_st16(const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st)
{
    constexpr int NI = DmaQueue<N, 32, DPQ, 4>::NI, DP = DPQ < NI ? DPQ : NI;                     // ring of row quads, clamped to the tile
    if (plan.wpb != WPB) return 1;                                                                // the grid was laid out for another block shape
    MultiH16Taps<N, K> taps;
    memset(&taps, 0, sizeof(taps));
    for (int k = 0; k < K; ++k) pack_taps(center[k], SRoll<N>::WS, taps.t[k].w);
    return launch_body_tiles<WPB, DP>(SG_FAMILY_NAME(sg_bank_dma_multi_, _kernel)<N, FMA, K, 32, WPB, DP>, job, taps, plan.geo, plan.grid, st);
}

// (waves per block, ring rows) by half window, bank and output count: the family's shape table (sg_stream_host.hpp) as template arguments
template <int N, bool FMA, int K>
static int launch_bank_dma_multi_st16_shape(const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st)
{
    constexpr MultiH16TileShape s = StreamFamily::multi_tile_shape(N, FMA, K);
    static_assert(s.rows % 4 == 0, "a DMA moves four rows");
    return launch_bank_dma_multi_st16<N, FMA, K, s.wpb, s.rows / 4>(center, job, plan, st);
}

template <int N, bool FMA>
static int dispatch_bank_dma_multi_st16(int n, int outputs, const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st)
{
    constexpr int max2 = StreamFamily::multi_max_n(FMA, 2), max3 = StreamFamily::multi_max_n(FMA, 3);
    if (n == N) {
        if constexpr (N <= max2) { if (outputs == 2) return launch_bank_dma_multi_st16_shape<N, FMA, 2>(center, job, plan, st); }
        if constexpr (N <= max3) { if (outputs == 3) return launch_bank_dma_multi_st16_shape<N, FMA, 3>(center, job, plan, st); }
        return 1;
    }
    if constexpr (N < (max2 > max3 ? max2 : max3)) return dispatch_bank_dma_multi_st16<N + 1, FMA>(n, outputs, center, job, plan, st);
    else return 1;
}

// the Makefile builds two objects per family, one per bank kind, so that they compile side by side
#if SG_MULTI_ST16_FMA
int SG_FAMILY_NAME(sg_bank_dma_multi_, _launch_fma)(int n, int outputs, const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st)
{
    return n < 1 ? 1 : dispatch_bank_dma_multi_st16<1, true>(n, outputs, center, job, plan, st);
}
#else
int SG_FAMILY_NAME(sg_bank_dma_multi_, _launch_ref)(int n, int outputs, const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st)
{
    return n < 1 ? 1 : dispatch_bank_dma_multi_st16<1, false>(n, outputs, center, job, plan, st);
}
#endif

}  // namespace sg
