// sg_stream_dma_multi_i16.hip -- savgol_streambank_push_block_multi_i16, the body of a fused call: LDS-DMA tiles on int16 rows with K outputs from one
// read of the samples.
//
// sg_stream_dma_multi_h16.hip with the body tile's other storage: the fragment (sg_stream_dma_body.inc, K = 2 or 3) is included with SG_BODY_I16 set, so
// a lane's dword widens ONCE per row for every output through the exact sign-extending convert and an int16 output row is rounded, saturated and packed
// once per output (sg_i16.hpp); everything else -- the DMA queue, the K feeds, the centre, the K stores per output row -- is the text the 16-bit float
// kernels compile.  The samples cross HBM -> LDS once for K banks: 2 + 2 K bytes per stream-tick (int16 -> int16) instead of 4 K, 2 + 4 K (int16 -> fp32)
// instead of 6 K.  The same job (BankJobMultiH16: its samples are 16-bit words either way; out_type SAVGOL_HIP_I16 or _F32, wave-uniform), the h16
// launchers' signatures, one object per bank kind.  Only bands >= 2 of a call come here (block_plan_multi_i16, sg_stream_host.hpp).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "sg_i16.hpp"
#include "sg_internal.h"
#include "sg_pk.hpp"
#include "sg_runtime.hpp"
#include "sg_stream_dma.hpp"
#include "sg_stream_dma_body.hpp"
#include "sg_stream_multi_i16.hpp"
#include "sg_stream_roll.hpp"

namespace sg {

#ifndef SG_MULTI_I16_FMA
#define SG_MULTI_I16_FMA 1
#endif

// Waves per SIMD the registers are allocated for (as i16_tile_min_waves, sg_stream_dma_i16.hip).  One tile is held to the step its 16-bit float twin
// compiles to: the bit-exact bank's three-output tile at n = 4, 64 VGPRs = eight waves on the twin; left alone it comes out at 66, the int16 narrow's
// second temporary.  Every other tile keeps what a block of WPB waves implies by itself, so its code is what it is without the second
// argument.
constexpr int multi_i16_tile_min_waves(int n, bool fma, int k, int wpb) { return !fma && n == 4 && k == 3 ? 8 : (wpb + 3) / 4; }

// DP: the ring, in DMAs = KiB = four rows each
template <int N, bool FMA, int K, int TRT, int WPB, int DP, int FCH = 2>
__global__ __launch_bounds__(64 * WPB, multi_i16_tile_min_waves(N, FMA, K, WPB)) void sg_bank_dma_multi_i16_kernel(const BankJobMultiH16 job, const MultiH16Taps<N, K> all, const TileGeom geo)
{
    static_assert(K >= 2 && K <= STREAM_MULTI_PER_LAUNCH, "outputs per launch; one output is sg_bank_dma_i16_kernel");
    constexpr int MOM = 0;
#define SG_BODY_I16
#include "sg_stream_dma_body.inc"
#undef SG_BODY_I16
}

// One launch of the body's tiles for K outputs; 1 = the runtime refused it
template <int N, bool FMA, int K, int WPB, int DPQ>
static int launch_bank_dma_multi_i16(const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st)
{
    constexpr int NI = DmaQueue<N, 32, DPQ, 4>::NI, DP = DPQ < NI ? DPQ : NI;                     // ring of row quads, clamped to the tile
    if (plan.wpb != WPB) return 1;                                                                // the grid was laid out for another block shape
    MultiH16Taps<N, K> taps;
    memset(&taps, 0, sizeof(taps));
    for (int k = 0; k < K; ++k) pack_taps(center[k], SRoll<N>::WS, taps.t[k].w);
    return launch_body_tiles<WPB, DP>(sg_bank_dma_multi_i16_kernel<N, FMA, K, 32, WPB, DP>, job, taps, plan.geo, plan.grid, st);
}

// (waves per block, ring rows) by half window, bank and output count: multi_i16_tile_shape (sg_stream_host.hpp) as template arguments
template <int N, bool FMA, int K>
static int launch_bank_dma_multi_i16_shape(const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st)
{
    constexpr MultiH16TileShape s = multi_i16_tile_shape(N, FMA, K);
    static_assert(s.rows % 4 == 0, "a DMA moves four rows");
    return launch_bank_dma_multi_i16<N, FMA, K, s.wpb, s.rows / 4>(center, job, plan, st);
}

template <int N, bool FMA>
static int dispatch_bank_dma_multi_i16(int n, int outputs, const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st)
{
    if (n == N) {
        if constexpr (N <= stream_multi_i16_max_n(FMA, 2)) { if (outputs == 2) return launch_bank_dma_multi_i16_shape<N, FMA, 2>(center, job, plan, st); }
        if constexpr (N <= stream_multi_i16_max_n(FMA, 3)) { if (outputs == 3) return launch_bank_dma_multi_i16_shape<N, FMA, 3>(center, job, plan, st); }
        return 1;
    }
    constexpr int top = stream_multi_i16_max_n(FMA, 2) > stream_multi_i16_max_n(FMA, 3) ? stream_multi_i16_max_n(FMA, 2) : stream_multi_i16_max_n(FMA, 3);
    if constexpr (N < top) return dispatch_bank_dma_multi_i16<N + 1, FMA>(n, outputs, center, job, plan, st);
    else return 1;
}

// the Makefile builds two objects, one per bank kind, so that they compile side by side
#if SG_MULTI_I16_FMA
int sg_bank_dma_multi_i16_launch_fma(int n, int outputs, const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st)
{
    return n < 1 ? 1 : dispatch_bank_dma_multi_i16<1, true>(n, outputs, center, job, plan, st);
}
#else
int sg_bank_dma_multi_i16_launch_ref(int n, int outputs, const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st)
{
    return n < 1 ? 1 : dispatch_bank_dma_multi_i16<1, false>(n, outputs, center, job, plan, st);
}
#endif

}  // namespace sg
