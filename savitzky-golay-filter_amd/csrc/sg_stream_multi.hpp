// sg_stream_multi.hpp -- the fused multi-output stream block push (savgol_streambank_push_block_multi): the by-value job of its LDS-DMA tile kernel
// and the launchers its objects export.  A job of its own: BankJob is every fp32 block kernel's argument and stays as it is.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "sg_stream_host.hpp"

namespace sg {

constexpr int STREAM_MULTI_PER_LAUNCH = 3;                   // outputs of one launch: 2 or 3 (four banks are two launches of two)

// The body of a fused call: ticks band0 * 32 .. ticks - 1 of the call, for `outputs` banks that share the samples.  Every row a body tile reads is a row
// of this call (band0 * 32 >= 2n) and every tick has an output, so neither the rings nor the counters appear.
struct BankJobMulti {
    const float *samples;                                    // [ticks][streams]
    float       *out[STREAM_MULTI_PER_LAUNCH];               // [ticks][streams] each
    size_t       streams, ticks;                             // of the whole call
    unsigned     band0;                                      // the twins' band of the body's first tile (2: the head is two bands)
    float        dt_inv[STREAM_MULTI_PER_LAUNCH];
    float        centre_sum[STREAM_MULTI_PER_LAUNCH];        // as BankJob's, per bank
    int          centre[STREAM_MULTI_PER_LAUNCH];
};

// 0 = launched, 1 = not covered (a refused launch, a half window or an output count outside the object's table).  center[k]: bank k's centre taps;
// `plan`: block_plan_multi's (geometry, grid, waves per block and ring of the body's launches).
int sg_bank_dma_multi_launch_fma(int n, int outputs, const float *const *center, const BankJobMulti &job, const MultiPlan &plan, hipStream_t st);
int sg_bank_dma_multi_launch_ref(int n, int outputs, const float *const *center, const BankJobMulti &job, const MultiPlan &plan, hipStream_t st);

}  // namespace sg
