// sg_stream_i16.hpp -- the stream block push on int16 storage (savgol_streambank_push_block_i16): the launchers its objects export.  The job is the
// 16-bit float call's (BankJobH16, sg_stream_h16.hpp): `samples` are 16-bit words either way, in_type is SAVGOL_HIP_I16 and out_type SAVGOL_HIP_I16 or
// SAVGOL_HIP_F32 (= H16_STORE_F32, the one value the body tile compares out_type with on this storage).
#pragma once

#include "sg_stream_h16.hpp"

namespace sg {

// 0 = launched, 1 = not covered (a refused launch, a half window outside the object's range): the h16 launchers' contract and signatures
int sg_bank_dma_i16_launch_mom(int n, const StreamMomentFit &fit, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st);   // 12..20
int sg_bank_dma_i16_launch_lo(int n, int fma, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st);                       // 1..16
int sg_bank_dma_i16_launch_hi(int n, int fma, const float *center, const BankJobH16 &job, const TileGeom &geo, unsigned grid, hipStream_t st);                       // 17..32

}  // namespace sg
