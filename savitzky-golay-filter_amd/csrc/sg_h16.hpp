// sg_h16.hpp -- fp16 / bf16 elements <-> fp32, for every kernel on 16-bit float storage (sg_k1d_st16.hpp, sg_stream_dma_st16.hip, sg_stream.hip): the
// tree's one definition.  Widening is exact (fp16 subnormals included: the hardware convert with the kernels' default denormal mode), narrowing rounds
// once to nearest even (NaN stays NaN, overflow into fp16 gives +-Inf).  Where the storage type is an argument it is wave-uniform.
#pragma once

#include <hip/hip_runtime.h>

#include "sg_pk.hpp"

namespace sg {

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16   bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef __bf16   bf16x4 __attribute__((ext_vector_type(4)));

// one dword as loaded (element 0 in the low half) -> two fp32
__device__ __forceinline__ f32x2 widen2(const unsigned raw, const bool bf)
{
    if (bf) return f32x2{__uint_as_float(raw << 16), __uint_as_float(raw & 0xffff0000u)};
    const f16x2 h = __builtin_bit_cast(f16x2, raw);
    return f32x2{(float)h.x, (float)h.y};
}
__device__ __forceinline__ float widen1(const unsigned short raw, const bool bf)
{
    if (bf) return __uint_as_float((unsigned)raw << 16);
    return (float)__builtin_bit_cast(_Float16, raw);
}
__device__ __forceinline__ unsigned narrow2(const f32x2 v, const bool bf)
{
    if (bf) return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2));
}
__device__ __forceinline__ unsigned short narrow1(const float v, const bool bf)
{
    if (bf) return __builtin_bit_cast(unsigned short, (__bf16)v);
    return __builtin_bit_cast(unsigned short, (_Float16)v);
}
// four 16-bit elements as loaded (element 0 in the low half of .x) -> fp32, exactly
__device__ __forceinline__ float4 widen4_f16(const u32x2 raw)
{
    const f16x4 h = __builtin_bit_cast(f16x4, raw);
    return float4{(float)h.x, (float)h.y, (float)h.z, (float)h.w};
}
__device__ __forceinline__ float4 widen4_bf16(const u32x2 raw)
{
    return float4{__uint_as_float(raw.x << 16), __uint_as_float(raw.x & 0xffff0000u), __uint_as_float(raw.y << 16), __uint_as_float(raw.y & 0xffff0000u)};
}
// fp32 -> the 16-bit type, round to nearest even (NaN stays NaN, overflow gives +-Inf)
__device__ __forceinline__ u32x2 narrow4_f16(const float4 v)
{
    const f32x4 f = {v.x, v.y, v.z, v.w};
    return __builtin_bit_cast(u32x2, __builtin_convertvector(f, f16x4));
}
__device__ __forceinline__ u32x2 narrow4_bf16(const float4 v)
{
    const f32x4 f = {v.x, v.y, v.z, v.w};
    return __builtin_bit_cast(u32x2, __builtin_convertvector(f, bf16x4));
}

}  // namespace sg
