// sg_stream_multi_h16.hpp -- the fused multi-output stream block push on 16-bit storage (savgol_streambank_push_block_multi_h16): the by-value job of its
// LDS-DMA tile kernel and the launchers its objects export.  A job of its own: BankJob, BankJobH16 and BankJobMulti stay as they are.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "sg_stream_h16.hpp"
#include "sg_stream_host.hpp"
#include "sg_stream_multi.hpp"

namespace sg {

// The body of a fused call: ticks band0 * 32 .. ticks - 1 of the call, for `outputs` banks that share the 16-bit samples.  Every row a body tile reads
// is a 16-bit row of this call (band0 * 32 >= 2n) and every tick has an output, so neither the rings nor the counters appear.  One input type and one
// output type serve every output; both are wave-uniform: scalar branches at the widen and at the stores.
struct BankJobMultiH16 {
    const unsigned short *samples;                           // [ticks][streams], fp16 or bf16 words
    void                 *out[STREAM_MULTI_PER_LAUNCH];      // [ticks][streams] of out_type elements each
    size_t                streams, ticks;                    // of the whole call
    unsigned              band0;                             // the twins' band of the body's first tile (2: the head is two bands)
    float                 dt_inv[STREAM_MULTI_PER_LAUNCH];
    float                 centre_sum[STREAM_MULTI_PER_LAUNCH];   // as BankJob's, per bank
    int                   centre[STREAM_MULTI_PER_LAUNCH];
    unsigned              in_type;                           // H16_STORE_F16 or H16_STORE_BF16
    unsigned              out_type;                          // the input's type, or H16_STORE_F32
};

// 0 = launched, 1 = not covered (a refused launch, a half window or an output count outside the object's table).  center[k]: bank k's centre taps;
// `plan`: block_plan_multi_h16's (geometry, grid, waves per block and ring of the body's launches).
int sg_bank_dma_multi_h16_launch_fma(int n, int outputs, const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st);
int sg_bank_dma_multi_h16_launch_ref(int n, int outputs, const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st);

}  // namespace sg
