// sg_stream_multi_i16.hpp -- the fused multi-output stream block push on int16 storage (savgol_streambank_push_block_multi_i16): the launchers its
// objects export.  The job is the 16-bit float fused call's (BankJobMultiH16, sg_stream_multi_h16.hpp): `samples` are 16-bit words either way, in_type
// is SAVGOL_HIP_I16 and out_type SAVGOL_HIP_I16 or SAVGOL_HIP_F32 (= H16_STORE_F32, the one value the body tile compares out_type with on this storage).
#pragma once

#include "sg_stream_multi_h16.hpp"

namespace sg {

// 0 = launched, 1 = not covered (a refused launch, a half window or an output count outside the object's table): the h16 launchers' contract and
// signatures.  `plan`: block_plan_multi_i16's
int sg_bank_dma_multi_i16_launch_fma(int n, int outputs, const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st);
int sg_bank_dma_multi_i16_launch_ref(int n, int outputs, const float *const *center, const BankJobMultiH16 &job, const MultiPlan &plan, hipStream_t st);

}  // namespace sg
