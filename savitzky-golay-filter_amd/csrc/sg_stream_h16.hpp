// sg_stream_h16.hpp -- the stream block push on 16-bit storage (savgol_streambank_push_block_h16): the by-value job of its LDS-DMA tile kernel and the
// launchers its objects export.  A job of its own: BankJob is every fp32 block kernel's argument and stays as it is.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "sg_stream_host.hpp"

namespace sg {

// storage types of a device buffer: the values of SAVGOL_HIP_F32 / _F16 / _BF16 (include/savgol_hip.h)
enum : unsigned { H16_STORE_F32 = 0, H16_STORE_F16 = 1, H16_STORE_BF16 = 2 };

// The body of a tile-route call: ticks band0 * 32 .. ticks - 1 of the call.  Every row a body tile reads is a 16-bit row of this call (band0 * 32 >=
// 2n) and every tick has an output, so neither the ring nor the counters appear.  The types are wave-uniform: scalar branches at the widen and the store.
// The per-output fields are arrays of one: the body tile (sg_stream_dma_body.inc) reads this job and BankJobMultiH16 with the same text.
struct BankJobH16 {
    const unsigned short *samples;   // [ticks][streams], fp16 or bf16 words
    void                 *out[1];    // [ticks][streams] of out_type elements
    size_t                streams, ticks;          // of the whole call
    unsigned              band0;     // the twin's band of the body's first tile (2: the head is two bands)
    float                 dt_inv[1];
    float                 centre_sum[1];           // as BankJob's
    int                   centre[1];
    unsigned              in_type;   // H16_STORE_F16 or H16_STORE_BF16
    unsigned              out_type;  // the input's type, or H16_STORE_F32
};

// 0 = launched, 1 = not covered (a refused launch, a half window outside the object's range).  `geo` / `grid`: block_plan_h16's, for the body.
int sg_bank_dma_h16_launch_mom(int n, const StreamMomentFit &fit, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st);   // 12..20
int sg_bank_dma_h16_launch_lo(int n, int fma, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st);                       // 1..16
int sg_bank_dma_h16_launch_hi(int n, int fma, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st);                       // 17..32

}  // namespace sg
