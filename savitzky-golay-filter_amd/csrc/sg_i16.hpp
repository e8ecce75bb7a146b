// sg_i16.hpp -- int16 elements <-> fp32, for every kernel on int16 storage (sg_k1d_st16.hpp, sg_stream_dma_st16.hip, sg_stream.hip): the tree's one
// definition.  Widening is the exact sign-extending convert; narrowing converts ONCE: round to nearest with ties to even, saturate to
// [-32768, 32767] (so +-Inf saturate), NaN gives 0 -- the contract of the int16 calls (include/savgol_hip.h).
#pragma once

#include <hip/hip_runtime.h>

#include "sg_pk.hpp"

namespace sg {

typedef short i16x2 __attribute__((ext_vector_type(2)));
typedef short i16x4 __attribute__((ext_vector_type(4)));

// one dword as loaded (element 0 in the low half) -> two fp32, exactly
__device__ __forceinline__ f32x2 widen2_i16(const unsigned raw)
{
    const i16x2 h = __builtin_bit_cast(i16x2, raw);
    return f32x2{(float)h.x, (float)h.y};
}
// four int16 elements as loaded (element 0 in the low half of .x) -> fp32, exactly
__device__ __forceinline__ float4 widen4_i16(const u32x2 raw)
{
    const i16x4 h = __builtin_bit_cast(i16x4, raw);
    return float4{(float)h.x, (float)h.y, (float)h.z, (float)h.w};
}
// fp32 -> int32 with the HARDWARE's convert semantics, which a C++ cast does not promise: NaN gives 0, values beyond the int32 range (+-Inf
// included) saturate.  The argument is already an integer value (rint_i32 below), so the instruction's truncation does not round.
__device__ __forceinline__ int cvt_i32_sat(const float v)
{
    int r;
    asm("v_cvt_i32_f32 %0, %1" : "=v"(r) : "v"(v));
    return r;
}
// fp32 -> the int32 the int16 output is packed from: round to nearest, ties to even, then the saturating convert
__device__ __forceinline__ int rint_i32(const float v) { return cvt_i32_sat(__builtin_rintf(v)); }
// two int32 -> two int16 in one dword, each saturated to [-32768, 32767] (v_cvt_pk_i16_i32); `lo` in the low half
__device__ __forceinline__ unsigned pack2_i16(const int lo, const int hi) { return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pk_i16(lo, hi)); }
// fp32 -> int16: round to nearest even, saturate to [-32768, 32767] (so +-Inf saturate), NaN gives 0
__device__ __forceinline__ unsigned narrow2_i16(const f32x2 v) { return pack2_i16(rint_i32(v.x), rint_i32(v.y)); }
__device__ __forceinline__ u32x2 narrow4_i16(const float4 v)
{
    return u32x2{pack2_i16(rint_i32(v.x), rint_i32(v.y)), pack2_i16(rint_i32(v.z), rint_i32(v.w))};
}
__device__ __forceinline__ short narrow1_i16(const float v) { return (short)(pack2_i16(rint_i32(v), 0) & 0xffffu); }

}  // namespace sg
